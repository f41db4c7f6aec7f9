"""The online CCA decoder on the GPU (td_cca_online_push, online.OnlineDecoder around CCADecoders): one
recording of 1500 frames cut into pushes every way, behind the projections against the existing kernels bit
for bit, the projections against float64, the windows against the oracle chain at the project's tolerances, as
a bank, in front of the state-space decoder, and end to end against infer.run_reduction_test."""
import numpy as np
import pytest

from oracle import lag as o_lag
from tests import host_online_cca as hc
from tests import parity_log

pytestmark = pytest.mark.gpu

FRAMES = hc.FRAMES
SHAPES, WINDOWS = hc.SHAPES, hc.WINDOWS


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


class Bank(object):
  """S sessions' inputs and models on the device, and a walk over a cut of the recording."""

  def __init__(self, dev, view1, view2, eeg, feat, mean_x, rot_x, mean_y, rot_y, corr, lda=None):
    self.dev, self.h = dev, dev.default_handle()
    h = self.h
    (self.c1, self.pre1, self.post1), (self.c2, self.pre2, self.post2) = view1, view2
    eeg, feat = np.asarray(eeg, np.float32), np.asarray(feat, np.float32)       # [S, n, c1], [S, 2, n, c2]
    self.s, self.n, _ = eeg.shape
    up = lambda a, dtype=np.float32: h.to_device(np.ascontiguousarray(a).reshape(-1, a.shape[-1]),
                                                 dtype).reshape(a.shape)
    self.eeg = up(eeg)
    self.feat = [up(feat[:, k]) for k in (0, 1)]
    rot_x, rot_y = np.asarray(rot_x, np.float32), np.asarray(rot_y, np.float32)
    if rot_x.ndim == 2:
      rot_x, rot_y, mean_x, mean_y = rot_x[None], rot_y[None], np.asarray(mean_x)[None], np.asarray(mean_y)[None]
    self.dims = rot_x.shape[2]
    self.rot_x, self.rot_y = up(rot_x), up(rot_y)
    self.mean_x, self.mean_y = up(np.asarray(mean_x, np.float32)), up(np.asarray(mean_y, np.float32))
    self.corr = up(np.asarray(corr, np.float64).reshape(self.s, 2, 3, self.dims), np.float64)
    self.lda = None if lda is None else up(np.asarray(lda, np.float64).reshape(self.s, self.dims + 2), np.float64)

  def state_bytes(self, width):
    return self.dev.cca_online_state_bytes(self.c1, self.pre1, self.post1, self.c2, self.pre2, self.post2, width)

  def run(self, sizes, width, hop, decoder='wta', reduction='first', flush_apart=False):
    """Pushes of the given sizes, the last one flushing (or a flush of its own behind them): everything the
    session gave, concatenated, and the final state blocks."""
    import torch
    dev, h = self.dev, self.h
    state = torch.zeros((self.s, self.state_bytes(width)), dtype=torch.uint8, device=h.device)
    outs, at = [], 0
    sizes = list(sizes) + ([0] if flush_apart else [])
    for i, n in enumerate(sizes):
      flush = i == len(sizes) - 1
      cut = lambda t: t[:, at:at + n] if n else None
      out = dev.cca_online_push(cut(self.eeg), cut(self.feat[0]), cut(self.feat[1]), self.mean_x, self.rot_x,
                                self.mean_y, self.rot_y, self.corr, state, at, self.pre1, self.post1, self.pre2,
                                self.post2, width, hop, reduction, self.lda if reduction == 'lda' else None,
                                decoder, flush=flush, want_frames=True, handle=h)
      assert out.plan.first_window == sum(int(o.scores.shape[2]) for o in outs)
      outs.append(out)
      at += n
    assert at == self.n
    return dict(scores=torch.cat([o.scores for o in outs], dim=2).cpu().numpy(),
                decisions=torch.cat([o.decisions for o in outs], dim=1).cpu().numpy(),
                proj=torch.cat([o.proj for o in outs], dim=1).cpu().numpy(),
                frame=torch.cat([o.frame for o in outs], dim=2).cpu().numpy(),
                state=state.cpu().numpy())


def _bank_of(dev, rec, lda=True):
  return Bank(dev, rec['view1'], rec['view2'], rec['eeg'][None], rec['feat'][None], rec['mean_x'], rec['rot_x'],
              rec['mean_y'], rec['rot_y'], rec['corr'][None], lda=rec['lda'][None] if lda else None)


def _same(got, want, what):
  for key in ('scores', 'decisions', 'proj', 'frame', 'state'):
    assert got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
    assert got[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize('shape,window', list(zip(SHAPES, WINDOWS)))
def test_any_cut_of_the_recording_gives_the_same_bits(dev, shape, window):
  """Scores, decisions, projections, per-frame scores and the final state block, byte for byte, for pushes of
  1, of 7, of one row less than each view's tail, one push longer than the window by 1, seeded random sizes
  with zeros, and the whole recording; each ended by a flushing last push and by a flush of its own;
  winner-take-all and stepped."""
  (view1, view2, dims), (width, hop) = shape, window
  bank = _bank_of(dev, hc.recipe(view1, view2, dims))
  cuts = hc.chunkings(view1, view2, width, seed=view1[0])
  assert 0 in cuts['random'] and cuts['width+1'][0] == width + 1
  for decoder in ('wta', 'stepped'):
    whole = bank.run(cuts['whole'], width, hop, decoder, 'lda')
    assert whole['scores'].shape == (2, 1, (FRAMES - width) // hop + 1)
    assert whole['proj'].shape == (1, FRAMES, 3 * dims) and np.isfinite(whole['scores']).all()
    assert np.ptp(whole['scores']) > 0
    for name, sizes in sorted(cuts.items()):
      # (both ways of ending for the cuts that are quick, one each for the 1500 pushes of one frame)
      for flush_apart in ((decoder == 'stepped',) if name == 'ones' else (False, True)):
        _same(bank.run(sizes, width, hop, decoder, 'lda', flush_apart=flush_apart), whole,
              (name, decoder, flush_apart))


@pytest.mark.parametrize('reduction', hc.REDUCTIONS)
def test_behind_the_projections_it_is_the_existing_kernels(dev, reduction):
  """From the session's own projections on: per-frame scores == td_frame_scores(a, b_s), window scores ==
  td_window_means of them, decisions == td_decide_wta / td_decide_step, bit for bit -- at 2, 5, 16 and (but
  for 'second') 1 dims."""
  for view1, view2, dims in (SHAPES[0], SHAPES[1], SHAPES[5], SHAPES[4]):
    if reduction == 'second' and dims < 2:
      continue
    rec = hc.recipe(view1, view2, dims)
    bank = _bank_of(dev, rec)
    h = bank.h
    stats, lda = rec['corr'][0], rec['lda']
    kw = dict(lda_w=lda[:-2], lda_slope=lda[-2], lda_intercept=lda[-1]) if reduction == 'lda' else {}
    for width, hop in WINDOWS[:5] if dims == 2 else WINDOWS[2:3]:
      for decoder in ('wta', 'stepped'):
        got = bank.run([700, 1, 799], width, hop, decoder, reduction)
        proj = h.to_device(got['proj'][0])
        a = proj[:, :dims].contiguous()
        means = []
        for spk in (0, 1):
          b = proj[:, (1 + spk) * dims:(2 + spk) * dims].contiguous()
          frame = dev.frame_scores(a, b, reduction, stats[0], stats[1], stats[2], handle=h, **kw)
          assert frame.cpu().numpy().tobytes() == got['frame'][spk, 0].tobytes(), (reduction, dims, spk)
          means.append(dev.window_means(frame, [0, FRAMES], width, hop, handle=h))
          assert means[spk].cpu().numpy().tobytes() == got['scores'][spk, 0].tobytes(), (reduction, dims, width)
        if decoder == 'wta':
          want = dev.decide_wta(means[0], means[1], handle=h)
        else:
          want, _ = dev.decide_step(means[0], means[1], [0, int(means[0].shape[0])], handle=h)
        assert want.cpu().numpy().tobytes() == got['decisions'][0].tobytes(), (reduction, dims, width, decoder)


@pytest.mark.parametrize('view1,view2,dims', SHAPES)
def test_projections_against_float64(dev, view1, view2, dims):
  """(lag_matrix(x) - mean) @ rot in float64 for both views, with the inputs of
  test_gpu_online.test_prediction_against_float64: rows 2^-20 .. 2^20 apart in scale, an all-zero row, one huge
  sample.  The error relative to the size of the terms of each sum, |x~ - mean| @ |rot|, stays below that
  test's bound plus 2^-24 for the one correctly rounded subtraction per term: 4.6e-7 (6.6e-7 where a view has
  fewer than four channels).  Measured on an MI355X: 5.4e-8 .. 1.7e-7 for the EEG view, 1.0e-7 .. 2.2e-7 for the feature view (DESIGN section
  26 has the table)."""
  (c1, pre1, post1), (c2, pre2, post2) = view1, view2
  rng = np.random.default_rng(pre1 * 37 + post1 + c1 + 1000 * c2)

  def view(c, pre, post, huge_row):
    k = c * (pre + 1 + post)
    x = rng.standard_normal((FRAMES, c)).astype(np.float32)
    x *= np.exp2(rng.integers(-20, 21, size=(FRAMES, 1))).astype(np.float32)
    x[7] = 0.0
    x[huge_row, min(3, c - 1)] = 3.0e30
    return x, rng.standard_normal(k).astype(np.float32), (rng.standard_normal((k, dims)) / np.sqrt(k)).astype(np.float32)

  x, mean_x, rot_x = view(c1, pre1, post1, 20)
  y1, mean_y, rot_y = view(c2, pre2, post2, 20)
  y2 = view(c2, pre2, post2, 33)[0]
  corr = np.tile(np.array([0.0, 0.0, 1.0]).reshape(1, 3, 1), (2, 1, dims))
  bank = Bank(dev, view1, view2, x[None], np.stack([y1, y2])[None], mean_x, rot_x, mean_y, rot_y, corr[None])
  tails = pre1 + pre2 + 2 * max(post1, post2)
  got = bank.run([1, 6, tails + 3, 64, 65, 500, FRAMES - 639 - tails], 100, 50)['proj'][0].astype(np.float64)
  f64 = lambda a: a.astype(np.float64)
  worst = {}
  for name, rows, pre, post, mean, rot, cols in (('a', x, pre1, post1, mean_x, rot_x, slice(0, dims)),
                                                 ('b1', y1, pre2, post2, mean_y, rot_y, slice(dims, 2 * dims)),
                                                 ('b2', y2, pre2, post2, mean_y, rot_y, slice(2 * dims, 3 * dims))):
    centred = o_lag.lag_matrix(f64(rows), pre, post) - f64(mean)
    want = centred @ f64(rot)
    size = np.abs(centred) @ np.abs(f64(rot))
    worst[name] = float(np.max(np.abs(got[:, cols] - want) / size))
  err1, err2 = worst['a'], max(worst['b1'], worst['b2'])
  parity_log.record('online cca proj %s %s %d' % (view1, view2, dims), gpu_vs_ref64=max(err1, err2))
  print('online cca projections %s | %s | %d: view 1 %.3g, view 2 %.3g' % (view1, view2, dims, err1, err2))
  assert err1 < (4.6e-7 if c1 >= 4 else 6.6e-7), err1
  assert err2 < (4.6e-7 if c2 >= 4 else 6.6e-7), err2


@pytest.mark.parametrize('view1,view2,dims', SHAPES[:2])
def test_window_scores_against_the_oracle_chain(dev, view1, view2, dims):
  """lag_matrix -> cca_transform -> Correlator.correlate -> reduce_correlations ('lda') -> windowed_means ->
  wta_sequence / step_sequence in float64, on the recipe of tests/host_online_cca.py: scores within tol =
  1e-5 max|want|, decisions equal on every window whose oracle margin |s1 - s2| exceeds 2 tol, at most 1 % of
  the windows set aside by that.  On the CPU the oracle sets aside, for (100,50) (10,5) (37,11) (1,1) (5,9):
  0 of 29, 0 of 299, 0 of 134, 0 of 1500, 0 of 167 windows at (5,2,9 | 3,1,4 | 2) and 0, 0, 1 of 134, 0, 0 at
  (64,0,20 | 8,0,15 | 5); the smallest other margin is 3.1 tol ((5,2,9 | 3,1,4 | 2) at (1,1))."""
  rec = hc.recipe(view1, view2, dims)
  bank = _bank_of(dev, rec)
  for width, hop in WINDOWS[:5]:
    want, wta, step = hc.oracle_chain(rec, width, hop, 'lda')
    tol = 1e-5 * np.max(np.abs(want))
    clear = np.abs(want[:, 0] - want[:, 1]) > 2 * tol
    aside = int(np.sum(~clear))
    for decoder, truth in (('wta', wta), ('stepped', step)):
      got = bank.run([10] * (FRAMES // 10), width, hop, decoder, 'lda')
      scores = got['scores'][:, 0].T
      err = np.max(np.abs(scores - want))
      parity_log.record('online cca windows c%d %d/%d %s' % (view1[0], width, hop, decoder),
                        gpu_vs_oracle=err / tol * 1e-5, set_aside=aside, windows=len(clear))
      print('online cca windows c%d (%d, %d) %s: %.3g tol, %d of %d set aside' %
            (view1[0], width, hop, decoder, err / tol, aside, len(clear)))
      np.testing.assert_allclose(scores, want, rtol=1e-5, atol=tol)
      assert aside <= 0.01 * len(clear)
      np.testing.assert_array_equal(got['decisions'][0][clear].astype(bool), truth[clear])


def test_a_bank_is_its_sessions(dev):
  """Three sessions with their own models and statistics in one call == three calls of one session; one shared
  model (stride 0) == three copies of it."""
  view1, view2, dims = SHAPES[0]
  rec = hc.recipe(view1, view2, dims)
  scales = (1.0, 0.5, 2.0)
  eeg = np.stack([rec['eeg'] * np.float32(s) for s in (1.0, 3.0, 0.25)])
  feat = np.stack([rec['feat'], rec['feat'][::-1], rec['feat'] * np.float32(2.0)])
  models = [[rec[k] * np.float32(s) for s in scales] for k in ('mean_x', 'rot_x', 'mean_y', 'rot_y')]
  corr = np.stack([rec['corr'] * s for s in scales])
  corr[1, 1] *= 1.5                     # (the two speakers' statistics need not be the same)
  lda = np.stack([rec['lda'] * s for s in scales])
  sizes = [333, 7, 0, 1160]
  for decoder, (width, hop) in (('wta', (37, 11)), ('stepped', (10, 5))):
    stacked = [np.stack(m) for m in models]
    bank = Bank(dev, view1, view2, eeg, feat, *stacked, corr, lda).run(sizes, width, hop, decoder, 'lda')
    for i in range(3):
      one = Bank(dev, view1, view2, eeg[i:i + 1], feat[i:i + 1], *[m[i] for m in models], corr[i:i + 1],
                 lda[i:i + 1]).run(sizes, width, hop, decoder, 'lda')
      for key in ('scores', 'frame'):
        assert bank[key][:, i].tobytes() == one[key][:, 0].tobytes(), (decoder, i, key)
      for key in ('decisions', 'proj', 'state'):
        assert bank[key][i].tobytes() == one[key][0].tobytes(), (decoder, i, key)
    shared = Bank(dev, view1, view2, eeg, feat, *[m[0] for m in models], corr, lda).run(sizes, width, hop, decoder,
                                                                                      'lda')
    copies = Bank(dev, view1, view2, eeg, feat, *[np.stack([m[0]] * 3) for m in models], corr, lda).run(
        sizes, width, hop, decoder, 'lda')
    _same(shared, copies, decoder)
    assert shared['proj'][1].tobytes() != bank['proj'][1].tobytes()


def _push(dec, rec, lo, hi):
  return dec.push(rec['eeg'][lo:hi], rec['feat'][0, lo:hi], rec['feat'][1, lo:hi])


@pytest.mark.parametrize('tuned', [False, True])
def test_state_space_decoder_over_pushes(dev, tuned):
  """'ssd': the windows of each push go into td_decode_ssd_stream; over all pushes that is td_decode_ssd on all
  windows at once, exactly -- untuned and with tuned priors.  Two launches per push that completes windows."""
  from telluride_decoding_amd import online
  rec = hc.recipe(*SHAPES[0])
  h = dev.default_handle()
  width, hop = 10, 5
  whole = _bank_of(dev, rec).run([FRAMES], width, hop, 'none', 'lda')
  assert not whole['decisions'].any()
  s1, s2 = whole['scores'][0, 0], whole['scores'][1, 0]
  dec = online.OnlineDecoder(hc.decoder_of(rec, 'lda'), width, hop, decoder_type='ssd')
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
    r = _push(dec, rec, at, at + n)
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
  rec = hc.recipe(*SHAPES[0])
  h = dev.default_handle()
  runs = []
  for _ in range(2):
    dec = online.OnlineDecoder(hc.decoder_of(rec, 'mean-squared'), 37, 11, decoder_type='stepped')
    out, at = [], 0
    h.profile_enable(True)
    h.profile_read()
    for n in (5, 0, 1, 10, 700, 784):
      r = _push(dec, rec, at, at + n)
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
  r = _push(dec, rec, 0, 5)
  assert r.scores.shape == (1, 0, 2) and r.first_window == 0
  # device tensors go in as they are
  x = h.to_device(rec['eeg'])
  f1, f2 = h.to_device(rec['feat'][0]), h.to_device(rec['feat'][1])
  r = dec.push(x[5:500], f1[5:500], f2[5:500])
  assert r.scores.tobytes() == runs[0][0][:r.scores.shape[1]].tobytes()


def test_invalid_arguments_queue_nothing(dev):
  """Every TD_ERR_INVALID of the header's td_cca_online_* entries, through the C interface: nothing is launched
  and the state stays."""
  import ctypes
  import torch
  h = dev.default_handle()
  c1, pre1, post1, c2, pre2, post2, dims, width, hop, n = 4, 2, 3, 3, 1, 2, 2, 10, 5, 20
  k1, k2 = c1 * 6, c2 * 4
  nbytes = dev.cca_online_state_bytes(c1, pre1, post1, c2, pre2, post2, width)
  eeg, f1, f2 = h.zeros((2, n, c1)), h.zeros((2, n, c2)), h.zeros((2, n, c2))
  mean_x, rot_x, mean_y, rot_y = h.zeros((2, k1)), h.zeros((2, k1 * dims)), h.zeros((2, k2)), h.zeros((2, k2 * dims))
  corr, lda = h.zeros((2, 6 * dims), 'float64') + 1.0, h.zeros((2, dims + 2), 'float64')
  state = torch.full((2, nbytes), 7, dtype=torch.uint8, device=h.device)
  scores, decisions = h.zeros((64,), 'float64'), h.zeros((64,), 'uint8')
  p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
  good = dict(h=h.ptr, sessions=2, eeg=p(eeg), eeg_ld=c1, eeg_ss=n * c1, f1=p(f1), f2=p(f2), f_ld=c2, f_ss=n * c2,
              n=n, c1=c1, pre1=pre1, post1=post1, c2=c2, pre2=pre2, post2=post2, dims=dims, mean_x=p(mean_x),
              rot_x=p(rot_x), mean_y=p(mean_y), rot_y=p(rot_y), model_ss=1, corr=p(corr), reduction=0, lda=None,
              width=width, hop=hop, decoder=0, before=0, flush=0, state=p(state), state_ss=nbytes,
              scores=p(scores), decisions=p(decisions), proj=None, frame=None)
  bad = [dict(h=None), dict(sessions=0), dict(eeg=None), dict(f1=None), dict(f2=None), dict(mean_x=None),
         dict(rot_x=None), dict(mean_y=None), dict(rot_y=None), dict(corr=None), dict(state=None),
         dict(scores=None), dict(decisions=None), dict(c1=0), dict(c1=129), dict(c2=0), dict(c2=33),
         dict(pre1=-1), dict(post1=-1), dict(pre1=40, post1=24), dict(pre2=-1), dict(post2=-1),
         dict(pre2=40, post2=24), dict(dims=0), dict(dims=17), dict(c1=128, pre1=31, post1=32, dims=16),
         dict(n=-1), dict(n=(1 << 20) + 1), dict(width=0), dict(width=65537), dict(hop=0), dict(reduction=-1),
         dict(reduction=5), dict(reduction=4), dict(reduction=1, dims=1), dict(decoder=3), dict(decoder=-1),
         dict(before=-1), dict(eeg_ld=c1 - 1), dict(f_ld=c2 - 1), dict(eeg_ss=c1 - 1), dict(f_ss=c2 - 1),
         dict(model_ss=2), dict(model_ss=-1), dict(state_ss=nbytes - 8), dict(state_ss=nbytes + 4)]
  h.profile_enable(True)
  h.profile_read()
  for change in bad:
    args = dict(good, **change)
    status = h.lib.td_cca_online_push(*args.values())
    assert status == -1, change
  n64, pass_ = ctypes.c_int64(0), ctypes.c_int(0)
  for change in (dict(c1=0), dict(c1=129), dict(c2=33), dict(pre1=-1), dict(pre1=40, post1=24), dict(post2=-1),
                 dict(pre2=32, post2=32), dict(width=0), dict(width=65537)):
    a = dict(good, **change)
    assert h.lib.td_cca_online_state_bytes(a['c1'], a['pre1'], a['post1'], a['c2'], a['pre2'], a['post2'],
                                           a['width'], ctypes.byref(n64)) == -1, change
  assert h.lib.td_cca_online_state_bytes(c1, pre1, post1, c2, pre2, post2, width, None) == -1
  for change in (dict(c1=129), dict(dims=0), dict(dims=17), dict(c1=128, pre1=31, post1=32, dims=16), dict(n=-1)):
    a = dict(good, **change)
    assert h.lib.td_cca_online_lds_bytes(a['c1'], a['pre1'], a['post1'], a['c2'], a['pre2'], a['post2'], a['dims'],
                                         a['n'], ctypes.byref(pass_), ctypes.byref(n64)) == -1, change
  assert h.lib.td_cca_online_lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, n, None, ctypes.byref(n64)) == -1
  assert h.profile_read()[0] == 0
  assert bool((state == 7).all())
  # (and the call the changes were made to is a good one; lda only matters for its reduction)
  assert h.lib.td_cca_online_push(*good.values()) == 0
  assert h.lib.td_cca_online_push(*dict(good, reduction=4, lda=p(lda), before=n).values()) == 0
  assert h.profile_read()[0] == 2
  h.profile_enable(False)
  assert not bool((state == 7).all())


@pytest.mark.parametrize('decoder_type', ['wta', 'stepped'])
def test_end_to_end_against_run_reduction_test(dev, decoder_type, tmp_path):
  """A BrainModelCCA (3 dims, lambda 0.1) fitted on a one-file dataset (1500 frames in batches of 100: the
  batch route drops no frame) with (5,2,9 | 3,1,4), a CCADecoder trained with the LDA, then pushes of 10 frames
  against the details of infer.run_reduction_test for windows of 100: scores within 1e-5 max|want|, decisions
  equal wherever the batch route's margin exceeds twice that (at least 99 % of the windows).  The saved model
  directory gives a session with the same bytes."""
  from telluride_decoding_amd import brain_data, cca, infer, infer_decoder, online
  view1, view2, _ = SHAPES[0]
  rec = hc.recipe(view1, view2, 2)
  eeg, feat, att = rec['eeg'], rec['feat'], rec['att']
  pick = att.reshape(-1, 1) > 0.5
  attended, unattended = np.where(pick, feat[1], feat[0]), np.where(pick, feat[0], feat[1])
  make = lambda y: brain_data.Dataset([(eeg, y, y[:, :1], att)], 100, view1[1], view1[2], view2[1], view2[2])
  fit_data, bd1, bd2 = make(attended), make(feat[0]), make(feat[1])
  model = cca.BrainModelCCA(fit_data, cca_dims=3, regularization_lambda=0.1)
  model.fit(fit_data)
  model.add_metadata(hc.context_of(view1, view2))
  decoder = infer_decoder.CCADecoder(model, reduction='lda')
  decoder.train(make(unattended), fit_data)
  details = {}
  infer.run_reduction_test(decoder, bd1, bd2, decoder_type=decoder_type, window_list=[100], details=details)
  want = np.stack([details[100]['d1'], details[100]['d2']], axis=1)
  assert want.shape == (29, 2)
  dec = online.OnlineDecoder(decoder, 100, decoder_type=decoder_type)
  assert (dec.kind, dec.dims, dec.delay) == ('cca', 3, 9)

  def walk(session):
    out = [_push(session, rec, at, at + 10) for at in range(0, FRAMES, 10)]
    out.append(session.flush())
    return np.concatenate([r.scores[0] for r in out]), np.concatenate([r.decisions[0] for r in out])

  scores, decisions = walk(dec)
  tol = 1e-5 * np.max(np.abs(want))
  print('online cca end to end %s: %.3g tol' % (decoder_type, np.max(np.abs(scores - want)) / tol))
  np.testing.assert_allclose(scores, want, rtol=1e-5, atol=tol)
  clear = np.abs(want[:, 0] - want[:, 1]) > 2 * tol
  assert clear.sum() >= 0.99 * len(clear)
  np.testing.assert_array_equal(decisions[clear].astype(bool), details[100]['attention'][clear, 0] >= 0.5)
  # most windows away from the switch are decoded for the attended speaker
  labels = details[100]['labels']
  pure = (labels == 0) | (labels == 1)
  assert np.mean((decisions[pure] == 1) == (labels[pure] == 0)) > 0.8
  # the saved experiment: model and decoder parameters in one directory
  model_dir = tmp_path / 'cca_model'
  model.save(str(model_dir))
  decoder.save_parameters(str(model_dir / infer_decoder.DECODER_PARAM_FILE_NAME))
  loaded = online.OnlineDecoder.from_model_dir(str(model_dir), 'lda', 100, decoder_type=decoder_type)
  again = walk(loaded)
  assert again[0].tobytes() == scores.tobytes() and again[1].tobytes() == decisions.tobytes()
  assert loaded._dev['state'].cpu().numpy().tobytes() == dec._dev['state'].cpu().numpy().tobytes()
