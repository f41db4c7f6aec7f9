"""The online calibration on the GPU (td_calib_online_push / _sums / _finish, online.OnlineCalibration,
OnlineDecoder.set_statistics): labelled white-noise stretches of 300 frames (130 for the two large shapes) at the
shapes where the kernel can go wrong -- no tail at all, one channel, a tail longer than a short push, K = 1344 (five
full rounds of the four prediction accumulators and a remainder), the limit of 128 channels x 64 lags -- and windows of
1, 7 and 100 frames.  The sums bit for bit against the NumPy twin fed with td_online_push's own predictions, every cut
byte for byte, finish against the two-pass float64 route and against the batch route, a padded bank against its
sessions, one launch per push, the calibrator following set_weights, and a running bank after set_statistics against
a fresh one."""
import numpy as np
import pytest

from oracle import attention as o_att
from tests import host_online
from tests import host_online_calib as hoc
from tests import parity_log

pytestmark = pytest.mark.gpu

# (c, pre, post, frames)
SHAPES = [(3, 0, 0, 300), (1, 0, 0, 300), (5, 2, 9, 300), (64, 0, 20, 130), (128, 31, 32, 130)]
IDS = ['c%d_pre%d_post%d_n%d' % s for s in SHAPES]
WIDTHS = (1, 7, 100)
# (shape, width) with at least 6 windows per class, as the distances' bars ask: every shape at 1 and 7, and 100 on a
# longer stretch of the shape with both tails
DISTANCES = [(s, w) for s in SHAPES for w in (1, 7)] + [((5, 2, 9, 700), 100)]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _up(a):
  import torch
  return torch.from_numpy(np.array(a, order='C')).to('cuda')       # (a copy: the shared stretches are read-only)


def _bank(st, sessions=1, reduction='first', lda=None, width=20, hop=10, kind='wta', stats=(0.1, 0.2, 0.9)):
  from telluride_decoding_amd import online
  decs = [host_online.linear_decoder(st['c'], st['pre'], st['post'], st['w'], st['b'], stats, reduction, lda)
          for _ in range(sessions)]
  return online.OnlineDecoder(decs, width, hop, decoder_type=kind)


_PRED = {}


def _device_pred(dev, st, w=None, b=None):
  """td_online_push's float32 prediction of every frame of a stretch (one push and the flush, want_frames), for the
  stretch's own model or the one given: once per key, read-only."""
  import torch
  w = st['w'] if w is None else w
  b = st['b'] if b is None else b
  key = (id(st['eeg']), st['pre'], st['post'], w.tobytes(), float(b))      # (hoc.stretch keeps its arrays alive)
  if key not in _PRED:
    c, pre, post = st['c'], st['pre'], st['post']
    eeg = _up(st['eeg'])[None]
    env = torch.stack([_up(st['att']), _up(st['unatt'])], dim=1)[None]
    state = torch.zeros((1, dev.online_state_bytes(c, pre, post, 4)), dtype=torch.uint8, device='cuda')
    corr = torch.tensor([[[0.0, 0.0, 1.0]] * 2], dtype=torch.float64, device='cuda')
    wd, bd = _up(w)[None], _up(np.array([b], np.float32))
    first = dev.online_push(eeg, env, wd, bd, corr, state, 0, pre, post, 4, 4, want_frames=True)
    last = dev.online_push(None, None, wd, bd, corr, state, st['frames'], pre, post, 4, 4, flush=True,
                           want_frames=True)
    pred = torch.cat([first.pred[0], last.pred[0]]).cpu().numpy()
    assert pred.shape == (st['frames'],) and pred.dtype == np.float32
    _PRED[key] = pred
  return _PRED[key]


def _tensors(st):
  return _up(st['eeg']), _up(st['att']), _up(st['unatt'])


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_sums_are_the_twins_bits_after_every_push(dev, shape, width):
  """sums() == twin_sums(pred of device.online_push(..., want_frames=True), att, unatt, W) with np.array_equal after
  every push (one of them shorter than the tails, one empty) and after the flush: the prediction's order and the
  sums' order at once."""
  from telluride_decoding_amd import online
  c, pre, post, frames = shape
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  pred = _device_pred(dev, st)
  assert dev.gpu_available()
  calib = online.OnlineCalibration(_bank(st), width)
  eeg, att, unatt = _tensors(st)

  def check(at, flushed=False):
    m = at if flushed else max(0, at - post)
    got = calib.sums()
    assert got.is_cuda and tuple(got.shape) == (1, 29) and str(got.dtype) == 'torch.float64'
    want = hoc.twin_sums(pred[:m], st['att'][:m], st['unatt'][:m], width)
    assert np.array_equal(got[0].cpu().numpy(), want), (at, flushed)

  hoc.run(calib, eeg, att, unatt, [frames // 3, 1, 0, 5, frames - frames // 3 - 6], after_push=check)
  check(frames, True)
  assert calib.windows == frames // width


_WHOLE = {}


def _whole(shape, width):
  """(state bytes, sums) after the whole stretch in one push and an empty flush: once per (shape, W), read-only."""
  from telluride_decoding_amd import online
  key = (shape, width)
  if key not in _WHOLE:
    c, pre, post, frames = shape
    st = hoc.stretch(c, pre, post, frames, offset=1.0)
    calib = online.OnlineCalibration(_bank(st), width)
    hoc.run(calib, *_tensors(st), [frames])
    _WHOLE[key] = (calib._dev['state'].clone(), calib.sums().clone())
  return _WHOLE[key]


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_any_cut_of_the_stretch_gives_the_same_state_bytes(dev, shape, width):
  """Pushes of 1 (shorter than the tails), W - 1, W, W + 1, random 0 .. 40 with empty pushes, whole, an empty push in
  the middle; flushed by a flushing last push and by an empty flushing push: the state block byte for byte -- sums,
  EEG tail and envelope tail."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, frames = shape
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  want_state, want_sums = _whole(shape, width)
  calib = online.OnlineCalibration(_bank(st), width)
  eeg, att, unatt = _tensors(st)
  for name, sizes in hoc.cuts(frames, width).items():
    for flush_last in (False, True):
      hoc.run(calib, eeg, att, unatt, sizes, flush_last=flush_last)
      assert torch.equal(calib._dev['state'], want_state), (name, flush_last)
  assert torch.equal(calib.sums(), want_sums)
  tail = calib._dev['state'][0, 8 * 29:].view(torch.float32)
  tl = pre + post
  assert torch.equal(tail[:tl * c].reshape(tl, c), eeg[frames - tl:])
  assert torch.equal(tail[tl * c:tl * c + 2 * post].reshape(post, 2), torch.stack([att, unatt], dim=1)[frames - post:])


def _result(r, i=0):
  return dict(corr=tuple(r.corr[i, 0].cpu().numpy()), lda=tuple(r.lda[i].cpu().numpy()),
              dprime=float(r.dprime[i].cpu()))


@pytest.mark.parametrize('shape,width', DISTANCES, ids=['%s_w%d' % ('c%d_pre%d_post%d_n%d' % s, w)
                                                       for s, w in DISTANCES])
def test_finish_against_the_two_pass_route_and_the_batch_route(dev, shape, width):
  """finish against Decoder.train's two passes in float64 on the same float32 predictions (oracle Correlator,
  average_data, scaled_lda_fit, calculate_dprime) at the CPU test's bars -- <= 1e-10 on the statistics and the LDA,
  <= 1e-9 on d' --, and for W >= 2 against the route the library had: device.window_sums per class into
  Decoder._add_sums, device.window_class_moments per class, fit_class_moments, at the same bars."""
  import torch
  from telluride_decoding_amd import infer_decoder, online, scaled_lda
  c, pre, post, frames = shape
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  assert frames // width >= 6
  pred = _device_pred(dev, st)
  calib = online.OnlineCalibration(_bank(st), width)
  hoc.run(calib, *_tensors(st), [frames // 2, frames - frames // 2])
  r = calib.finish()
  assert r.corr.is_cuda and tuple(r.corr.shape) == (1, 2, 3) and tuple(r.lda.shape) == (1, 3)
  assert torch.equal(r.corr[0, 0], r.corr[0, 1]) and float(r.lda[0, 0]) == 1.0
  got = _result(r)
  err, err_d = hoc.distances(got, hoc.two_pass(pred, st['att'], st['unatt'], width))
  print('%s W = %d: two-pass corr / lda %.3g, d\' %.3g' % (shape, width, err, err_d))
  record = dict(two_pass=err, two_pass_dprime=err_d)
  batch = batch_d = None
  if width >= 2:
    pd = _up(pred).reshape(-1, 1)
    streams = [(_up(st[key]).reshape(-1, 1), pd) for key in ('unatt', 'att')]
    dec = infer_decoder.Decoder()
    for x, y in streams:
      dec._add_sums(frames, dev.window_sums(x, y, [0, frames], frames, frames).cpu().numpy()[0])
    mx, my, pw = dec._stat_vectors(1)
    moments = [dev.window_class_moments(x, y, width, mx, my, pw).cpu().numpy() for x, y in streams]
    lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    lda.fit_class_moments(moments)
    (m1, v1), (m2, v2) = lda.projected_class_stats()
    want = dict(corr=(mx[0], my[0], pw[0]), lda=(1.0, lda.slope, lda.intercept),
                dprime=(m2 - m1) / np.sqrt((v1 + v2) / 2.0))
    batch, batch_d = hoc.distances(got, want)
    print('%s W = %d: batch route corr / lda %.3g, d\' %.3g' % (shape, width, batch, batch_d))
    record.update(batch=batch, batch_dprime=batch_d)
  parity_log.record('online_calib_c%d_pre%d_post%d_n%d_w%d' % (shape + (width,)), **record)
  # update_decoder evaluates the same closed form on the host: the parameters a saved decoder gets are finish's
  dec = host_online.linear_decoder(c, pre, post, st['w'], st['b'], (0.0, 0.0, 1.0), 'lda', (1.0, 1.0, 0.0))
  dprime = calib.update_decoder(dec)
  p = online.session_parameters(dec)
  host = dict(corr=tuple(p['corr'][0]), lda=tuple(p['lda']), dprime=dprime)
  assert max(hoc.distances(host, got)) <= 1e-12
  assert err <= 1e-10
  assert err_d <= 1e-9
  if width >= 2:
    assert batch <= 1e-10
    assert batch_d <= 1e-9


def test_a_padded_bank_is_its_sessions(dev):
  """Three sessions with different rows and different weights, every stride padded (rows wider and longer than the
  bank reads, a state row longer than a block), against three single sessions: state bytes and finish exactly."""
  import torch
  c, pre, post, frames, width = 5, 2, 9, 300, 7
  sts = [hoc.stretch(c, pre, post, frames, seed=s, offset=0.5 * s) for s in range(3)]
  k = (pre + 1 + post) * c
  nbytes = dev.online_calib_state_bytes(c, pre, post)
  eeg = torch.zeros((3, frames + 5, c + 3), device='cuda')
  env = torch.zeros((3, frames + 2, 3), device='cuda')
  w = torch.zeros((3, k), device='cuda')
  b = torch.zeros((3,), device='cuda')
  for i, s in enumerate(sts):
    eeg[i, :frames, :c], env[i, :frames, 0], env[i, :frames, 1] = _up(s['eeg']), _up(s['att']), _up(s['unatt'])
    w[i], b[i] = _up(s['w']), float(s['b'])
  eeg, env = eeg[:, :frames, :c], env[:, :frames, :2]
  state = torch.zeros((3, nbytes + 16), dtype=torch.uint8, device='cuda')[:, :nbytes]
  at = 0
  for n in (130, 1, 0, 169):
    at = dev.online_calib_push(eeg[:, at:at + n], env[:, at:at + n], w, b, state, at, pre, post, width)
  assert dev.online_calib_push(None, None, w, b, state, at, pre, post, width, c=c, flush=True) == frames
  sums = dev.online_calib_sums(state)
  out = dev.online_calib_finish(state, frames, width)
  assert not bool(out.status.any())
  for i, s in enumerate(sts):
    single = torch.zeros((1, nbytes), dtype=torch.uint8, device='cuda')
    se = _up(s['eeg'])[None]
    sv = torch.stack([_up(s['att']), _up(s['unatt'])], dim=1)[None]
    dev.online_calib_push(se, sv, w[i:i + 1], b[i:i + 1], single, 0, pre, post, width, flush=True)
    assert torch.equal(state[i], single[0]), i
    assert torch.equal(sums[i], dev.online_calib_sums(single)[0])
    one = dev.online_calib_finish(single, frames, width)
    for a, o in zip(out, one):
      assert torch.equal(a[i], o[0]), i
    pred = _device_pred(dev, s)
    assert np.array_equal(sums[i].cpu().numpy(), hoc.twin_sums(pred, s['att'], s['unatt'], width))
  assert not torch.equal(sums[0], sums[1])


def test_one_launch_per_push_and_one_for_finish(dev):
  """td_profile_read counts ONE launch for a push with rows (also one that emits nothing), none for an empty push,
  one for the flush, one for finish; two identical runs give the same bytes."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, frames, width = 64, 0, 20, 130, 7
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  eeg, att, unatt = _tensors(st)
  h = dev.default_handle()
  calib = online.OnlineCalibration(_bank(st), width)
  runs = []
  for attempt in range(2):
    calib.reset()
    h.profile_enable(True)
    h.profile_read()
    at = 0
    for n in (5, 0, 1, 37, 87):                              # (the first push emits nothing: 5 <= post)
      calib.push(eeg[at:at + n], att[at:at + n], unatt[at:at + n])
      assert h.profile_read()[0] == (1 if n else 0), n
      at += n
    assert calib.frames_emitted == frames - post
    calib.flush()
    assert h.profile_read()[0] == 1
    r = calib.finish()
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    assert r.corr.is_cuda and r.lda.is_cuda and r.dprime.is_cuda
    runs.append([calib._dev['state'].clone()] + [t.clone() for t in r])
  for first, second in zip(*runs):
    assert torch.equal(first, second)
  assert torch.equal(runs[0][0], _whole((c, pre, post, frames), width)[0])


def test_the_calibrator_follows_set_weights(dev):
  """After decoder.set_weights the next push predicts with the new weights: the sums are the twin's, fed the old
  model's predictions up to the swap and the new model's behind it."""
  from telluride_decoding_amd import online
  c, pre, post, frames, width = 5, 2, 9, 300, 7
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  other = hoc.stretch(c, pre, post, frames, seed=1)
  eeg, att, unatt = _tensors(st)
  bank = _bank(st)
  calib = online.OnlineCalibration(bank, width)
  cut = 130
  calib.push(eeg[:cut], att[:cut], unatt[:cut])
  bank.set_weights(_up(other['w']), _up(np.array([0.75], np.float32)))
  calib.push(eeg[cut:], att[cut:], unatt[cut:])
  calib.flush()
  k = cut - post                                             # frames counted before the swap
  pred = np.concatenate([_device_pred(dev, st)[:k], _device_pred(dev, st, other['w'], np.float32(0.75))[k:]])
  assert np.array_equal(calib.sums()[0].cpu().numpy(), hoc.twin_sums(pred, st['att'], st['unatt'], width))
  assert not np.array_equal(pred, _device_pred(dev, st))


def _windows(dec, tensors, lo, hi):
  r = dec.push(*[t[lo:hi] for t in tensors])
  return r.scores[0], r.decisions[0]


@pytest.mark.parametrize('kind', ['wta', 'stepped'])
@pytest.mark.parametrize('reduction', ['first', 'lda'])
def test_a_running_bank_after_set_statistics(dev, reduction, kind):
  """A bank trained with other statistics is pushed 130 rows, takes OnlineCalibration.finish's corr and lda device to
  device, and is pushed the rest: from the first window that lies wholly behind the swap its scores are byte for byte
  those of a fresh bank built with those parameters and pushed the same rows.  Winner-take-all
  decisions too.  The stepped decoder's state is untouched by the swap, so its decisions are the step sequence of the
  bank's OWN scores (old before the swap, new behind it) throughout -- and those of the fresh bank from the first
  window behind the swap at which the two step states meet at a limit.  A push is still one launch."""
  from telluride_decoding_amd import online
  c, pre, post, frames = 5, 2, 9, 600
  width, hop = 20, 10
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  tensors = _tensors(st)
  old_lda = (1.0, 2.0, -0.5) if reduction == 'lda' else None
  dec = _bank(st, reduction=reduction, lda=old_lda, width=width, hop=hop, kind=kind, stats=(0.3, -0.4, 2.0))
  calib = online.OnlineCalibration(dec, 20)
  hoc.run(calib, *tensors, [frames])
  r = calib.finish()
  trained = host_online.linear_decoder(c, pre, post, st['w'], st['b'], tuple(r.corr[0, 0].cpu().numpy()), reduction,
                                       tuple(r.lda[0].cpu().numpy()) if reduction == 'lda' else None)
  fresh = online.OnlineDecoder(trained, width, hop, decoder_type=kind)
  assert np.array_equal(fresh._dev['corr'].cpu().numpy(), r.corr.cpu().numpy())
  if reduction == 'lda':
    assert np.array_equal(fresh._dev['lda'].cpu().numpy(), r.lda.cpu().numpy())
  cut = 130
  h = dev.default_handle()
  head = _windows(dec, tensors, 0, cut)
  weights = dec._dev['w'].clone()
  dec.set_statistics(r.corr, r.lda)
  assert dec._dev['corr'].data_ptr() != r.corr.data_ptr() and np.array_equal(dec._dev['w'].cpu().numpy(),
                                                                             weights.cpu().numpy())
  h.profile_enable(True)
  h.profile_read()
  rest = _windows(dec, tensors, cut, frames)
  assert h.profile_read()[0] == 1
  h.profile_enable(False)
  last = dec.flush()
  got_s = np.concatenate([head[0], rest[0], last.scores[0]])
  got_d = np.concatenate([head[1], rest[1], last.decisions[0]])
  parts = [_windows(fresh, tensors, 0, cut), _windows(fresh, tensors, cut, frames)]
  last = fresh.flush()
  want_s = np.concatenate([parts[0][0], parts[1][0], last.scores[0]])
  want_d = np.concatenate([parts[0][1], parts[1][1], last.decisions[0]])
  assert got_s.shape == want_s.shape == ((frames - width) // hop + 1, 2)
  first = -(-(cut - post) // hop)                            # the first window that begins at or behind the swap
  assert 0 < first < got_s.shape[0] - 20
  assert got_s[first:].tobytes() == want_s[first:].tobytes()
  assert got_s[:first].tobytes() != want_s[:first].tobytes()
  if kind == 'wta':
    assert got_d[first:].tobytes() == want_d[first:].tobytes()
    return
  own, _ = o_att.step_sequence(got_s[:, 0], got_s[:, 1])
  assert np.array_equal(got_d.astype(bool), own)

  def states(scores):
    out, state = [], 0.5
    for a, b in scores:
      state = min(0.9, state + 0.1) if a > b else max(0.1, state - 0.1)
      out.append(state)
    return np.array(out)

  met = np.nonzero((states(got_s) == states(want_s))[first:])[0]
  assert met.size and first + met[0] < got_s.shape[0] - 10
  assert got_d[first + met[0]:].tobytes() == want_d[first + met[0]:].tobytes()


def test_refusals_leave_the_state_and_the_next_finish_is_served(dev):
  """Each status by name -- no completed window, zero power, equal class means, in one bank --, the state untouched,
  the next finish served; the refusals the device calls make."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, frames, width = 4, 1, 2, 80, 10
  st = hoc.stretch(c, pre, post, frames)
  eeg, att, unatt = _tensors(st)
  calib = online.OnlineCalibration(_bank(st), width)
  calib.push(eeg[:11], att[:11], unatt[:11])                 # 9 frames counted: no window of 10
  before = calib._dev['state'].clone()
  with pytest.raises(ValueError, match='session 0: No data for class 0'):
    calib.finish()
  assert torch.equal(calib._dev['state'], before)
  calib.push(eeg[11:], att[11:], unatt[11:])
  calib.flush()
  served = calib.finish()
  assert float(served.dprime[0]) > 0 and np.array_equal(
      calib.sums()[0].cpu().numpy(), hoc.twin_sums(_device_pred(dev, st), st['att'], st['unatt'], width))
  # session 1: zero weights, so every prediction is the bias 0.5 and every sum exact; session 2: one envelope twice
  bank = _bank(st, sessions=3)
  w = np.stack([st['w'], np.zeros_like(st['w']), st['w']])
  bank.set_weights(w, np.array([st['b'], 0.5, st['b']], np.float32))
  calib = online.OnlineCalibration(bank, width)
  calib.push(torch.stack([eeg] * 3), torch.stack([att] * 3), torch.stack([unatt, unatt, att]))
  state = calib._dev['state']
  before = state.clone()
  out = dev.online_calib_finish(state, calib.frames_emitted, width)
  assert out.status.cpu().tolist() == [dev.CALIB_OK, dev.CALIB_NO_POWER, dev.CALIB_SAME_MEANS]
  assert bool(torch.isnan(out.dprime[1:]).all()) and bool(torch.isnan(out.corr[1]).all())
  with pytest.raises(ValueError, match='session 1: the correlation power'):
    calib.finish()
  bank.set_weights(w[[0, 0, 0]], np.array([st['b']] * 3, np.float32))
  with pytest.raises(ValueError, match='session 1: the correlation power'):       # (the sums are what was pushed)
    calib.finish()
  assert torch.equal(state, before)
  zeros = torch.zeros((3, 50, c), device='cuda')
  env = torch.zeros((3, 50, 2), device='cuda')
  wd, bd = bank._dev['w'], bank._dev['b']
  for kwargs, match in ((dict(width=0), 'window of 0'), (dict(width=65537), 'window of 65537'),
                        (dict(frames_before=-1), 'frames before'), (dict(pre=40, post=40), 'lags')):
    args = dict(frames_before=50, pre=pre, post=post, width=width)
    args.update(kwargs)
    w_use = wd if 'pre' not in kwargs else torch.zeros((3, 81 * c), device='cuda')
    with pytest.raises(ValueError, match=match):
      dev.online_calib_push(zeros, env, w_use, bd, state, args['frames_before'], args['pre'], args['post'],
                            args['width'])
  with pytest.raises(ValueError, match='state stride'):
    dev.online_calib_push(zeros[:1], env[:1], wd[:1], bd[:1], state[:1, :-8], 50, pre, post, width)
  with pytest.raises(ValueError, match='state stride'):
    dev.online_calib_finish(state[:1, :8 * 28], 50, width)
  with pytest.raises(ValueError, match='window of 0'):
    dev.online_calib_finish(state, 50, 0)
  with pytest.raises(ValueError, match='weights for'):
    dev.online_calib_push(zeros, env, wd[:, :-1], bd, state, 50, pre, post, width)
  assert torch.equal(state, before)
  calib.push(torch.stack([eeg[:5]] * 3), torch.stack([att[:5]] * 3), torch.stack([unatt[:5], att[:5], unatt[:5]]))
  assert not torch.equal(state, before)
