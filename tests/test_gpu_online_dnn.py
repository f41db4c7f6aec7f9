"""The online DNN decoder on the GPU (td_fc_online_push, online.OnlineDecoder around a BrainModelDNN): one recording
of 1500 frames cut into pushes every way, the prediction against td_mlp_forward bit for bit and against float64,
everything behind it against the existing kernels bit for bit, the oracle chain at the project's tolerances, as a
bank, in front of the state-space decoder, and end to end against infer.run_reduction_test."""
import numpy as np
import pytest

from tests import host_online
from tests import host_online_dnn as hd
from tests import parity_log

pytestmark = pytest.mark.gpu

FRAMES = hd.FRAMES
SHAPES = hd.SHAPES
WINDOWS = hd.WINDOWS
LDA = hd.LDA


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


class Bank(object):
  """S sessions' inputs and models on the device, and a walk over a cut of the recording."""

  def __init__(self, dev, eeg, env, params, hidden, corr, pre, post, lda=None):
    self.dev, self.h = dev, dev.default_handle()
    h = self.h
    eeg, env = np.asarray(eeg, np.float32), np.asarray(env, np.float32)
    self.s, self.n, self.c = eeg.shape
    self.eeg = h.to_device(eeg.reshape(-1, self.c)).reshape(eeg.shape)
    self.env = h.to_device(env.reshape(-1, 2)).reshape(env.shape)
    params = np.asarray(params, np.float32)
    self.params = h.to_device(params.reshape(-1, params.shape[-1]))
    self.hidden = list(hidden)
    self.corr = h.to_device(np.asarray(corr, np.float64).reshape(-1, 6), np.float64).reshape(self.s, 2, 3)
    self.lda = None if lda is None else h.to_device(np.asarray(lda, np.float64).reshape(self.s, 3), np.float64)
    self.pre, self.post = pre, post

  def run(self, sizes, width, hop, decoder='wta', reduction='first', flush_apart=False):
    """Pushes of the given sizes, the last one flushing (or a flush of its own behind them): everything the
    session gave, concatenated, and the final state blocks."""
    import torch
    dev, h = self.dev, self.h
    nbytes = dev.online_state_bytes(self.c, self.pre, self.post, width)
    state = torch.zeros((self.s, nbytes), dtype=torch.uint8, device=h.device)
    outs, at = [], 0
    sizes = list(sizes) + ([0] if flush_apart else [])
    for i, n in enumerate(sizes):
      flush = i == len(sizes) - 1
      eeg = self.eeg[:, at:at + n] if n else None
      env = self.env[:, at:at + n] if n else None
      out = dev.dnn_online_push(eeg, env, self.params, self.hidden, self.corr, state, at, self.pre, self.post, width,
                                hop, reduction, self.lda if reduction == 'lda' else None, decoder, flush=flush,
                                want_frames=True, handle=h)
      assert out.plan.first_window == sum(int(o.scores.shape[2]) for o in outs)
      outs.append(out)
      at += n
    assert at == self.n
    return dict(scores=torch.cat([o.scores for o in outs], dim=2).cpu().numpy(),
                decisions=torch.cat([o.decisions for o in outs], dim=1).cpu().numpy(),
                pred=torch.cat([o.pred for o in outs], dim=1).cpu().numpy(),
                frame=torch.cat([o.frame for o in outs], dim=2).cpu().numpy(),
                state=state.cpu().numpy())


def _bank_of(dev, rec, lda=None):
  return Bank(dev, rec['eeg'][None], rec['env'][None], hd.packed(rec['weights'])[None], rec['hidden'],
              rec['corr'][None], rec['pre'], rec['post'], lda=None if lda is None else [lda])


def _same(got, want, what):
  for key in ('scores', 'decisions', 'pred', 'frame', 'state'):
    assert got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
    assert got[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize('shape,hidden,window', [s + (w,) for s, w in zip(SHAPES, WINDOWS + [(1, 1), (100, 50)])])
def test_any_cut_of_the_recording_gives_the_same_bits(dev, shape, hidden, window):
  """Scores, decisions, predictions, per-frame scores and the final state block, byte for byte, for pushes of 1
  (1500 of them), of 7, of pre + post - 1 (the tail shifts by less than its length), one push longer than the
  window by 1, seeded random sizes with zeros, and the whole recording; each ended by a flushing last push and by
  a flush of its own; winner-take-all and stepped; all seven shapes."""
  (c, pre, post), (width, hop) = shape, window
  bank = _bank_of(dev, hd.model(shape, hidden))
  cuts = host_online.chunkings(FRAMES, pre, post, width, seed=c)
  assert 0 in cuts['random'] and cuts['width+1'][0] == width + 1
  for decoder in ('wta', 'stepped'):
    whole = bank.run(cuts['whole'], width, hop, decoder)
    assert whole['scores'].shape == (2, 1, (FRAMES - width) // hop + 1)
    assert whole['pred'].shape == (1, FRAMES) and np.isfinite(whole['scores']).all()
    for name, sizes in sorted(cuts.items()):
      # (both ways of ending for the cuts that are quick, one each for the 1500 pushes of one frame)
      for flush_apart in ((decoder == 'stepped',) if name == 'ones' else (False, True)):
        _same(bank.run(sizes, width, hop, decoder, flush_apart=flush_apart), whole, (name, decoder, flush_apart))


@pytest.mark.parametrize('shape,hidden', SHAPES)
def test_prediction_is_the_batch_route_and_close_to_float64(dev, shape, hidden):
  """pred == device.mlp_forward(eeg, [0, 1500], pre, post, hidden, 1, params), byte for byte, with pushes of 1, 6,
  pre + post + 3, 64, 65, 500 and the rest; and against host_dnn.forward in float64
  max|got - want| / max|want| <= 1e-5, the bound of test_inference_matches_float64."""
  c, pre, post = shape
  rec = hd.model(shape, hidden)
  bank = _bank_of(dev, rec)
  sizes = [1, 6, pre + post + 3, 64, 65, 500]
  got = bank.run(sizes + [FRAMES - sum(sizes)], 100, 50)['pred'][0]
  batch = dev.mlp_forward(bank.eeg[0], [0, FRAMES], pre, post, hidden, 1, bank.params[0], handle=bank.h)
  batch = batch.cpu().numpy().reshape(-1)
  assert got.shape == batch.shape == (FRAMES,)
  assert got.tobytes() == batch.tobytes(), int(np.sum(got != batch))
  want = rec['pred64'][:, 0]
  err = np.max(np.abs(got.astype(np.float64) - want)) / np.max(np.abs(want))
  parity_log.record('online dnn pred c%d pre%d post%d %s' % (c, pre, post, hidden), gpu_vs_ref64=err)
  print('online dnn prediction c%d pre%d post%d %s: %.3g' % (c, pre, post, hidden, err))
  assert err <= 1e-5, err


@pytest.mark.parametrize('reduction', ['first', 'mean', 'mean-squared', 'lda'])
def test_behind_the_prediction_it_is_the_existing_kernels(dev, reduction):
  """From the session's own predictions on: per-frame scores == td_frame_scores, window scores ==
  td_window_means of them, decisions == td_decide_wta / td_decide_step, bit for bit."""
  rec = hd.model(*SHAPES[0])
  bank = _bank_of(dev, rec, LDA)
  h = bank.h
  stats = rec['corr'][0]
  kw = dict(lda_w=[LDA[0]], lda_slope=LDA[1], lda_intercept=LDA[2]) if reduction == 'lda' else {}
  for width, hop in WINDOWS:
    for decoder in ('wta', 'stepped'):
      got = bank.run([700, 1, 799], width, hop, decoder, reduction)
      pred = h.to_device(got['pred'].reshape(-1, 1))
      means = []
      for spk in (0, 1):
        frame = dev.frame_scores(bank.env[0, :, spk:spk + 1], pred, reduction, stats[0], stats[1], stats[2],
                                 handle=h, **kw)
        assert frame.cpu().numpy().tobytes() == got['frame'][spk, 0].tobytes(), (reduction, spk)
        means.append(dev.window_means(frame, [0, FRAMES], width, hop, handle=h))
        assert means[spk].cpu().numpy().tobytes() == got['scores'][spk, 0].tobytes(), (reduction, width, spk)
      if decoder == 'wta':
        want = dev.decide_wta(means[0], means[1], handle=h)
      else:
        want, _ = dev.decide_step(means[0], means[1], [0, int(means[0].shape[0])], handle=h)
      assert want.cpu().numpy().tobytes() == got['decisions'][0].tobytes(), (reduction, width, decoder)


@pytest.mark.parametrize('shape,hidden', SHAPES[:2])
def test_window_scores_against_the_oracle_chain(dev, shape, hidden):
  """host_dnn.forward -> Correlator.correlate -> windowed_means -> wta_sequence / step_sequence in float64 on
  dnn_recipe (seed 11): scores within tol = 1e-5 max|want|, decisions equal on every window whose oracle margin
  |s1 - s2| exceeds 2 tol, at most 1 % of the windows set aside by that.  On the CPU the oracle alone sets aside,
  for (100,50) (10,5) (37,11) (1,1) (5,9): 0 of 29, 0 of 299, 0 of 134, 3 of 1500, 0 of 167 windows at
  (5,2,9,[16]) and 0, 0, 0, 1 of 1500, 1 of 167 at (64,0,31,[33,7])."""
  rec = hd.dnn_recipe(host_online.recipe(*shape), hidden)
  bank = _bank_of(dev, rec)
  for width, hop in WINDOWS:
    want, wta, step = host_online.oracle_chain(rec, width, hop)
    tol = 1e-5 * np.max(np.abs(want))
    clear = np.abs(want[:, 0] - want[:, 1]) > 2 * tol
    aside = int(np.sum(~clear))
    for decoder, truth in (('wta', wta), ('stepped', step)):
      got = bank.run([10] * (FRAMES // 10), width, hop, decoder)
      scores = got['scores'][:, 0].T
      err = np.max(np.abs(scores - want))
      parity_log.record('online dnn windows c%d %d/%d %s' % (shape[0], width, hop, decoder),
                        gpu_vs_oracle=err / tol * 1e-5, set_aside=aside, windows=len(clear))
      print('online dnn windows c%d (%d, %d) %s: %.3g tol, %d of %d set aside' %
            (shape[0], width, hop, decoder, err / tol, aside, len(clear)))
      np.testing.assert_allclose(scores, want, rtol=1e-5, atol=tol)
      assert aside <= 0.01 * len(clear)
      np.testing.assert_array_equal(got['decisions'][0][clear].astype(bool), truth[clear])


def test_a_bank_is_its_sessions(dev):
  """Three sessions with their own models and statistics in one call == three calls of one session; one shared
  model (stride 0) == three copies of it."""
  shape, hidden = SHAPES[0]
  c, pre, post = shape
  rec = hd.model(shape, hidden)
  eeg = np.stack([rec['eeg'] * np.float32(s) for s in (1.0, 3.0, 0.25)])
  env = np.stack([rec['env'], rec['env'][:, ::-1], rec['env'] * np.float32(2.0)])
  models = np.stack([hd.packed(hd.glorot_model(c, pre, post, hidden, seed)) for seed in (5, 6, 7)])
  corr = np.stack([rec['corr'] * s for s in (1.0, 0.5, 2.0)])
  corr[1, 1] *= 1.5                     # (the two speakers' statistics need not be the same)
  sizes = [333, 7, 0, 1160]
  for decoder, (width, hop) in (('wta', (37, 11)), ('stepped', (10, 5))):
    bank = Bank(dev, eeg, env, models, hidden, corr, pre, post).run(sizes, width, hop, decoder)
    for i in range(3):
      one = Bank(dev, eeg[i:i + 1], env[i:i + 1], models[i:i + 1], hidden, corr[i:i + 1], pre, post).run(
          sizes, width, hop, decoder)
      for key in ('scores', 'frame'):
        assert bank[key][:, i].tobytes() == one[key][:, 0].tobytes(), (decoder, i, key)
      for key in ('decisions', 'pred', 'state'):
        assert bank[key][i].tobytes() == one[key][0].tobytes(), (decoder, i, key)
    shared = Bank(dev, eeg, env, models[:1], hidden, corr, pre, post).run(sizes, width, hop, decoder)
    copies = Bank(dev, eeg, env, np.stack([models[0]] * 3), hidden, corr, pre, post).run(sizes, width, hop, decoder)
    _same(shared, copies, decoder)
    assert shared['pred'][1].tobytes() != bank['pred'][1].tobytes()


def test_an_online_decoder_bank_shares_equal_models(dev):
  """online.OnlineDecoder: sessions around bitwise-equal parameters read one copy; their results are those of
  sessions of their own."""
  from telluride_decoding_amd import online
  rec = hd.model(*SHAPES[0])
  same = online.OnlineDecoder([hd.decoder_of(rec), hd.decoder_of(rec)], 37, 11)
  assert tuple(same._dev['params'].shape) == (1, hd.packed(rec['weights']).size)
  other = dict(rec, weights=hd.glorot_model(5, 2, 9, [16], 6))
  mixed = online.OnlineDecoder([hd.decoder_of(rec), hd.decoder_of(other)], 37, 11)
  assert int(mixed._dev['params'].shape[0]) == 2
  args = (np.stack([rec['eeg'][:400]] * 2), np.stack([rec['env'][:400, 0]] * 2), np.stack([rec['env'][:400, 1]] * 2))
  a, b = same.push(*args), mixed.push(*args)
  assert a.scores.shape[1] > 0
  assert a.scores[0].tobytes() == a.scores[1].tobytes() == b.scores[0].tobytes()
  assert b.scores[1].tobytes() != b.scores[0].tobytes()


@pytest.mark.parametrize('tuned', [False, True])
def test_state_space_decoder_over_pushes(dev, tuned):
  """'ssd': the windows of each push go into td_decode_ssd_stream; over all pushes that is td_decode_ssd on all
  windows at once, exactly -- untuned and with tuned priors.  Two launches per push."""
  from telluride_decoding_amd import online
  rec = hd.dnn_recipe(host_online.recipe(*SHAPES[0][0]), SHAPES[0][1])
  h = dev.default_handle()
  width, hop = 10, 5
  whole = _bank_of(dev, rec).run([FRAMES], width, hop, 'none')
  assert not whole['decisions'].any()
  s1, s2 = whole['scores'][0, 0], whole['scores'][1, 0]
  dec = online.OnlineDecoder(hd.decoder_of(rec), width, hop, decoder_type='ssd')
  prior = None
  if tuned:
    dec.tune(s1[:140], s2[:140])
    prior = dec._ssd._prior
  want = dev.decode_ssd(h.to_device(s1.reshape(-1, 1), np.float64).reshape(-1),
                        h.to_device(s2.reshape(-1, 1), np.float64).reshape(-1), [0, len(s1)],
                        offset=0.0, prior=prior, handle=h).cpu().numpy()
  got, scores, at = [], [], 0
  h.profile_enable(True)
  h.profile_read()
  for n in [100] * 7 + [3, 0, 797]:
    r = dec.push(rec['eeg'][at:at + n], rec['env'][at:at + n, 0], rec['env'][at:at + n, 1])
    launches = h.profile_read()[0]
    assert launches == (0 if n == 0 else 2 if r.scores.shape[1] else 1), (n, launches)
    assert r.first_window == sum(len(g) for g in got)
    got.append(r.decisions[0]); scores.append(r.scores[0])
    at += n
  r = dec.flush()
  h.profile_enable(False)
  got.append(r.decisions[0]); scores.append(r.scores[0])
  scores = np.concatenate(scores)
  assert scores[:, 0].tobytes() == s1.tobytes() and scores[:, 1].tobytes() == s2.tobytes()
  got = np.concatenate(got)
  assert got.shape == want.shape == (len(s1), 3)
  assert got.tobytes() == want.tobytes()
  assert np.ptp(got[:, 0]) > 0.1                              # (the decoder left its 0.5 start)


def test_one_launch_per_push_and_the_same_bits_twice(dev):
  from telluride_decoding_amd import online
  rec = hd.model(*SHAPES[1])
  h = dev.default_handle()
  runs = []
  for _ in range(2):
    dec = online.OnlineDecoder(hd.decoder_of(rec, 'mean-squared'), 37, 11, decoder_type='stepped')
    out, at = [], 0
    h.profile_enable(True)
    h.profile_read()
    for n in (5, 0, 1, 10, 700, 784):
      r = dec.push(rec['eeg'][at:at + n], rec['env'][at:at + n, 0], rec['env'][at:at + n, 1])
      assert h.profile_read()[0] == (1 if n else 0), n
      out.append(r)
      at += n
    out.append(dec.flush())
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    runs.append((np.concatenate([r.scores[0] for r in out]), np.concatenate([r.decisions[0] for r in out]),
                 dec._dev['state'].cpu().numpy()))
  assert runs[0][0].shape == ((FRAMES - 37) // 11 + 1, 2)
  for a, b in zip(*runs):
    assert a.tobytes() == b.tobytes()
  with pytest.raises(ValueError, match='flushed'):
    dec.flush()
  dec.reset()
  r = dec.push(rec['eeg'][:5], rec['env'][:5, 0], rec['env'][:5, 1])
  assert r.scores.shape == (1, 0, 2) and r.first_window == 0
  # device tensors go in as they are
  x = h.to_device(rec['eeg'])
  e = h.to_device(rec['env'])
  r = dec.push(x[5:500], e[5:500, 0], e[5:500, 1])
  assert r.scores.tobytes() == runs[0][0][:r.scores.shape[1]].tobytes()


def test_invalid_arguments_queue_nothing(dev):
  """Every TD_ERR_INVALID of the header, through the C interface: nothing is launched and the state stays."""
  import ctypes
  import torch
  h = dev.default_handle()
  c, pre, post, width, hop, n = 4, 2, 3, 10, 5, 20
  hidden = [8, 3]
  count = dev.dnn_param_count(6 * c, hidden)
  nbytes = dev.online_state_bytes(c, pre, post, width)
  eeg, env = h.zeros((2, n, c)), h.zeros((2, n, 2))
  params = h.zeros((2, count))
  corr, lda = h.zeros((2, 2, 3), 'float64') + 1.0, h.zeros((2, 3), 'float64')
  state = torch.full((2, nbytes), 7, dtype=torch.uint8, device=h.device)
  scores, decisions = h.zeros((64,), 'float64'), h.zeros((64,), 'uint8')
  p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
  ints = lambda v: (ctypes.c_int * len(v))(*v)
  good = dict(h=h.ptr, sessions=2, eeg=p(eeg), eeg_ld=c, eeg_ss=n * c, env=p(env), env_ld=2, env_ss=n * 2, n=n,
              c=c, pre=pre, post=post, hidden=ints(hidden), num_hidden=2, params=p(params), params_ss=count,
              corr=p(corr), reduction=0, lda=None, width=width, hop=hop, decoder=0, before=0, flush=0,
              state=p(state), state_ss=nbytes, scores=p(scores), decisions=p(decisions), pred=None, frame=None)
  bad = [dict(h=None), dict(sessions=0), dict(eeg=None), dict(env=None), dict(params=None), dict(hidden=None),
         dict(corr=None), dict(state=None), dict(scores=None), dict(decisions=None),
         dict(c=0), dict(c=129), dict(pre=-1), dict(post=-1), dict(pre=40, post=24), dict(n=-1),
         dict(n=(1 << 20) + 1), dict(width=0), dict(width=65537), dict(hop=0), dict(reduction=1),
         dict(reduction=5), dict(reduction=4), dict(decoder=3), dict(decoder=-1), dict(before=-1),
         dict(eeg_ld=c - 1), dict(env_ld=1), dict(eeg_ss=c - 1), dict(env_ss=1), dict(params_ss=count - 1),
         dict(params_ss=-1), dict(state_ss=nbytes - 8), dict(state_ss=nbytes + 4),
         dict(num_hidden=-1), dict(num_hidden=5, hidden=ints([8] * 5)), dict(hidden=ints([8, 0])),
         dict(hidden=ints([65, 3]))]
  h.profile_enable(True)
  h.profile_read()
  for change in bad:
    args = dict(good, **change)
    status = h.lib.td_fc_online_push(*args.values())
    assert status == -1, change
  assert h.profile_read()[0] == 0
  assert bool((state == 7).all())
  # (and the call the changes were made to is a good one; lda only matters for its reduction; no hidden layer
  # takes a NULL list)
  assert h.lib.td_fc_online_push(*good.values()) == 0
  assert h.lib.td_fc_online_push(*dict(good, reduction=4, lda=p(lda), before=n).values()) == 0
  assert h.lib.td_fc_online_push(*dict(good, hidden=None, num_hidden=0, params_ss=6 * c + 1, before=2 * n).values()) == 0
  assert h.profile_read()[0] == 3
  h.profile_enable(False)
  assert not bool((state == 7).all())


@pytest.mark.parametrize('decoder_type', ['wta', 'stepped'])
def test_end_to_end_against_run_reduction_test(dev, decoder_type):
  """A BrainModelDNN fitted for a few epochs on a one-file dataset (1500 frames in batches of 100: the batch route
  drops no frame), a trained LinearRegressionDecoder, then pushes of 10 frames against the details of
  infer.run_reduction_test for windows of 100: scores within 1e-5 max|want|, decisions equal wherever the batch
  route's margin exceeds twice that."""
  from telluride_decoding_amd import brain_data, brain_model, infer, infer_decoder, online
  rec = host_online.recipe(5, 2, 9)
  eeg, env, att = rec['eeg'], rec['env'], rec['att']
  attended = np.where(att > 0.5, env[:, 1:2], env[:, 0:1]).astype(np.float32)
  make = lambda y: brain_data.Dataset([(eeg, y, y, att)], 100, 2, 9)
  fit_data, bd1, bd2 = make(attended), make(env[:, 0:1]), make(env[:, 1:2])
  model = brain_model.BrainModelDNN(fit_data, [16, 4], seed=3)
  model.compile(learning_rate=1e-3)
  model.fit(fit_data, epochs=5)
  decoder = infer_decoder.LinearRegressionDecoder(model, reduction='first')
  decoder.train(make(np.where(att > 0.5, env[:, 0:1], env[:, 1:2]).astype(np.float32)), fit_data)
  details = {}
  infer.run_reduction_test(decoder, bd1, bd2, decoder_type=decoder_type, window_list=[100], details=details)
  want = np.stack([details[100]['d1'], details[100]['d2']], axis=1)
  assert want.shape == (29, 2)
  dec = online.OnlineDecoder(decoder, 100, decoder_type=decoder_type, pre_context=2, post_context=9)
  assert (dec.kind, dec.hidden) == ('dnn', [16, 4])
  out = [dec.push(eeg[at:at + 10], env[at:at + 10, 0], env[at:at + 10, 1]) for at in range(0, FRAMES, 10)]
  out.append(dec.flush())
  scores = np.concatenate([r.scores[0] for r in out])
  decisions = np.concatenate([r.decisions[0] for r in out])
  tol = 1e-5 * np.max(np.abs(want))
  print('online dnn end to end %s: %.3g tol' % (decoder_type, np.max(np.abs(scores - want)) / tol))
  np.testing.assert_allclose(scores, want, rtol=1e-5, atol=tol)
  clear = np.abs(want[:, 0] - want[:, 1]) > 2 * tol
  assert clear.sum() >= 0.99 * len(clear)
  np.testing.assert_array_equal(decisions[clear].astype(bool), details[100]['attention'][clear, 0] >= 0.5)
