"""The online DNN calibration on the GPU (td_fccalib_online_push, online.OnlineDNNCalibration, closed through
td_calib_online_sums / td_calib_online_finish and OnlineDecoder.set_statistics): labelled white-noise stretches of 130
to 300 frames with means of about one standard deviation, host_online_dnn.glorot_model networks, at the shapes where
the forward or the walk can go wrong -- K 60 in 15 slices with both tails; no hidden layer and no tail (the layer-1
sum is the prediction); a first layer of 33 units (the scalar chunk path); the largest head with a last slice of 18
rows; the limit of 128 channels x 64 lags (the 2 MB W1); and that input under the largest head, whose pass the LDS
budget halves to 32 frames -- and windows of 1, 7 and 100 frames.  The sums bit for bit against the NumPy twin fed with
td_fc_online_push's own predictions, every cut byte for byte, finish against the two-pass float64 route, padded and
shared-model banks against their sessions, one launch per push, a running bank after set_statistics against a fresh
one, every status by name, every invalid argument refused with the state untouched."""
import ctypes

import numpy as np
import pytest

from tests import host_online_calib as hoc
from tests import host_online_dnn as hd
from tests import host_online_dnn_calib as hdc
from tests import parity_log

pytestmark = pytest.mark.gpu

# ((c, pre, post), hidden, frames)
SHAPES = [((5, 2, 9), [16], 300), ((3, 0, 0), [], 300), ((64, 0, 31), [33, 7], 130),
          ((63, 40, 5), [64, 64, 64, 64], 130), ((128, 31, 32), [64], 130), ((128, 31, 32), [64, 64, 64, 64], 130)]
IDS = ['c%d_pre%d_post%d_h%s_n%d' % (s[0] + ('x'.join(str(u) for u in s[1]) or '0', s[2])) for s in SHAPES]
WIDTHS = (1, 7, 100)
# (shape, width) with at least 6 windows per class, as the distances' bars ask: every shape at 1 and 7, and 100 on a
# longer stretch of the first shape
DISTANCES = [(s, w) for s in SHAPES for w in (1, 7)] + [(((5, 2, 9), [16], 700), 100)]
DISTANCE_IDS = ['%s_w%d' % ('c%d_pre%d_post%d_h%s_n%d' % (s[0] + ('x'.join(str(u) for u in s[1]) or '0', s[2])), w)
                for s, w in DISTANCES]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _up(a):
  import torch
  return torch.from_numpy(np.array(a, order='C')).to('cuda')       # (a copy: the shared stretches are read-only)


def _tensors(st):
  return _up(st['eeg']), _up(st['att']), _up(st['unatt'])


_PRED = {}


def _device_pred(dev, st, weights=None):
  """td_fc_online_push's float32 prediction of every frame of a stretch (one push and the flush, want_frames), for
  the stretch's own network or the one given: once per key, read-only."""
  import torch
  weights = st['weights'] if weights is None else weights
  params = hd.packed(weights)
  key = (id(st['eeg']), st['pre'], st['post'], params.tobytes())     # (hdc.stretch keeps its arrays alive)
  if key not in _PRED:
    c, pre, post = st['c'], st['pre'], st['post']
    eeg = _up(st['eeg'])[None]
    env = torch.stack([_up(st['att']), _up(st['unatt'])], dim=1)[None]
    state = torch.zeros((1, dev.online_state_bytes(c, pre, post, 4)), dtype=torch.uint8, device='cuda')
    corr = torch.tensor([[[0.0, 0.0, 1.0]] * 2], dtype=torch.float64, device='cuda')
    pd = _up(params)[None]
    first = dev.dnn_online_push(eeg, env, pd, st['hidden'], corr, state, 0, pre, post, 4, 4, want_frames=True)
    last = dev.dnn_online_push(None, None, pd, st['hidden'], corr, state, st['frames'], pre, post, 4, 4, flush=True,
                               want_frames=True)
    pred = torch.cat([first.pred[0], last.pred[0]]).cpu().numpy()
    assert pred.shape == (st['frames'],) and pred.dtype == np.float32
    _PRED[key] = pred
  return _PRED[key]


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_sums_are_the_twins_bits_after_every_push(dev, shape, width):
  """sums() == twin_sums(pred of device.dnn_online_push(..., want_frames=True), att, unatt, W) with np.array_equal
  after every push (one of them shorter than the tails, one empty) and after the flush: the forward's order and the
  walk's order at once."""
  from telluride_decoding_amd import online
  st = hdc.stretch(*shape)
  post, frames = st['post'], st['frames']
  pred = _device_pred(dev, st)
  assert dev.gpu_available()
  assert np.max(np.abs(pred - st['pred64'])) <= 1e-3 * np.max(np.abs(st['pred64']))   # (the network, not noise)
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
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
  """(state bytes, sums) after the whole stretch in one push -- more than 64 emitted frames: several passes -- and an
  empty flush: once per (shape, W), read-only."""
  from telluride_decoding_amd import online
  key = (shape[0], tuple(shape[1]), shape[2], width)
  if key not in _WHOLE:
    st = hdc.stretch(*shape)
    calib = online.OnlineDNNCalibration(hdc.bank(st), width)
    hoc.run(calib, *_tensors(st), [st['frames']])
    _WHOLE[key] = (calib._dev['state'].clone(), calib.sums().clone())
  return _WHOLE[key]


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_any_cut_of_the_stretch_gives_the_same_state_bytes(dev, shape, width):
  """Pushes of 1 (shorter than the tails), W - 1, W, W + 1, random 0 .. 40 with empty pushes, whole (several passes),
  an empty push in the middle; flushed by a flushing last push and by an empty flushing push: the state block byte for
  byte -- sums, EEG tail and envelope tail."""
  import torch
  from telluride_decoding_amd import online
  st = hdc.stretch(*shape)
  c, pre, post, frames = st['c'], st['pre'], st['post'], st['frames']
  want_state, want_sums = _whole(shape, width)
  assert tuple(want_state.shape) == (1, dev.online_calib_state_bytes(c, pre, post))
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
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


@pytest.mark.parametrize('shape,width', DISTANCES, ids=DISTANCE_IDS)
def test_finish_against_the_two_pass_route(dev, shape, width):
  """finish against Decoder.train's two passes in float64 on the device's own float32 predictions (oracle Correlator,
  average_data, scaled_lda_fit, calculate_dprime) at DESIGN section 35's bars: <= 1e-10 on the statistics and the
  LDA, <= 1e-9 on d'.  update_decoder evaluates the same closed form on the host."""
  import torch
  from telluride_decoding_amd import online
  st = hdc.stretch(*shape)
  frames = st['frames']
  assert frames // width >= 6
  pred = _device_pred(dev, st)
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
  hoc.run(calib, *_tensors(st), [frames // 2, frames - frames // 2])
  r = calib.finish()
  assert r.corr.is_cuda and tuple(r.corr.shape) == (1, 2, 3) and tuple(r.lda.shape) == (1, 3)
  assert torch.equal(r.corr[0, 0], r.corr[0, 1]) and float(r.lda[0, 0]) == 1.0
  got = _result(r)
  err, err_d = hoc.distances(got, hoc.two_pass(pred, st['att'], st['unatt'], width))
  print('%s W = %d: two-pass corr / lda %.3g, d\' %.3g (d\' = %.4g)' % (shape, width, err, err_d, got['dprime']))
  parity_log.record('online_dnn_calib_%s' % DISTANCE_IDS[DISTANCES.index((shape, width))], two_pass=err,
                    two_pass_dprime=err_d)
  dec = hd.dnn_decoder(st['c'], st['pre'], st['post'], st['hidden'], st['weights'], (0.0, 0.0, 1.0), 'lda',
                       (1.0, 1.0, 0.0))
  dprime = calib.update_decoder(dec)
  p = online.session_parameters(dec)
  host = dict(corr=tuple(p['corr'][0]), lda=tuple(p['lda']), dprime=dprime)
  assert max(hoc.distances(host, got)) <= 1e-12
  assert err <= 1e-10
  assert err_d <= 1e-9


def test_padded_and_shared_banks_are_their_sessions(dev):
  """Three sessions with different rows and different networks, every stride padded (rows wider and longer than the
  bank reads, a state row longer than a block, a parameter row of an odd length, so that two models are not 16-byte
  aligned) against three single sessions: state bytes exactly, and the twin's sums.  Then one shared model
  (params_session_stride 0) against three copies of it."""
  import torch
  shape, hidden = (5, 2, 9), [16]
  c, pre, post = shape
  frames, width = 300, 7
  sts = [hdc.stretch(shape, hidden, frames, seed=s, offset=0.5 + 0.5 * s) for s in range(3)]
  count = dev.dnn_param_count(c * (pre + 1 + post), hidden)
  nbytes = dev.online_dnn_calib_state_bytes(c, pre, post)
  eeg = torch.zeros((3, frames + 5, c + 3), device='cuda')
  env = torch.zeros((3, frames + 2, 3), device='cuda')
  params = torch.zeros((3, count + 1 + count % 2), device='cuda')          # (an odd row length)
  assert params.shape[1] % 2 == 1
  for i, s in enumerate(sts):
    eeg[i, :frames, :c], env[i, :frames, 0], env[i, :frames, 1] = _up(s['eeg']), _up(s['att']), _up(s['unatt'])
    params[i, :count] = _up(hd.packed(s['weights']))
  eeg, env, params = eeg[:, :frames, :c], env[:, :frames, :2], params[:, :count]

  def run(rows, side, model, sessions):
    state = torch.zeros((sessions, nbytes + 16), dtype=torch.uint8, device='cuda')[:, :nbytes]
    at = 0
    for n in (130, 1, 0, 169):
      at = dev.online_dnn_calib_push(rows[:, at:at + n], side[:, at:at + n], model, hidden, state, at, pre, post, width)
    assert dev.online_dnn_calib_push(None, None, model, hidden, state, at, pre, post, width, flush=True) == frames
    return state

  state = run(eeg, env, params, 3)
  sums = dev.online_calib_sums(state)
  out = dev.online_calib_finish(state, frames, width)
  assert not bool(out.status.any())
  for i, s in enumerate(sts):
    single = torch.zeros((1, nbytes), dtype=torch.uint8, device='cuda')
    se = _up(s['eeg'])[None]
    sv = torch.stack([_up(s['att']), _up(s['unatt'])], dim=1)[None]
    dev.online_dnn_calib_push(se, sv, _up(hd.packed(s['weights']))[None], hidden, single, 0, pre, post, width,
                              flush=True)
    assert torch.equal(state[i], single[0]), i
    one = dev.online_calib_finish(single, frames, width)
    for a, o in zip(out, one):
      assert torch.equal(a[i], o[0]), i
    assert np.array_equal(sums[i].cpu().numpy(), hoc.twin_sums(_device_pred(dev, s), s['att'], s['unatt'], width))
  assert not torch.equal(sums[0], sums[1])
  # one model for every session: a stride of 0 against three copies of the model
  shared = run(eeg, env, params[1:2], 3)
  copies = run(eeg, env, params[1:2].expand(3, count).contiguous(), 3)
  assert torch.equal(shared, copies) and torch.equal(shared[1], state[1]) and not torch.equal(shared[0], state[0])


def test_one_launch_per_push_and_one_for_finish(dev):
  """td_profile_read counts ONE launch for a push with rows (also one that emits nothing), none for an empty push,
  one for the flush, one for finish; two identical runs give the same bytes."""
  import torch
  from telluride_decoding_amd import online
  shape, width = SHAPES[2], 7
  st = hdc.stretch(*shape)
  post, frames = st['post'], st['frames']
  eeg, att, unatt = _tensors(st)
  h = dev.default_handle()
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
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
    assert at == frames and calib.frames_emitted == frames - post
    calib.flush()
    assert h.profile_read()[0] == 1
    r = calib.finish()
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    assert r.corr.is_cuda and r.lda.is_cuda and r.dprime.is_cuda
    runs.append([calib._dev['state'].clone()] + [t.clone() for t in r])
  for first, second in zip(*runs):
    assert torch.equal(first, second)
  assert torch.equal(runs[0][0], _whole(shape, width)[0])


def _windows(dec, tensors, lo, hi):
  r = dec.push(*[t[lo:hi] for t in tensors])
  return r.scores[0], r.decisions[0]


@pytest.mark.parametrize('reduction', ['first', 'lda'])
def test_a_running_dnn_bank_after_set_statistics(dev, reduction):
  """A DNN bank trained with other statistics is pushed 130 rows, takes OnlineDNNCalibration.finish's corr and lda
  device to device, and is pushed the rest: from the first window that lies wholly behind the swap its scores and its
  winner-take-all decisions are byte for byte those of a fresh bank built with those parameters and pushed the same
  rows.  A push is still one launch."""
  from telluride_decoding_amd import online
  frames, width, hop, cut = 600, 20, 10, 130
  st = hdc.stretch((5, 2, 9), [16], frames)
  post = st['post']
  tensors = _tensors(st)
  old_lda = (1.0, 2.0, -0.5) if reduction == 'lda' else None
  dec = hdc.bank(st, reduction=reduction, lda=old_lda, width=width, hop=hop, stats=(0.3, -0.4, 2.0))
  calib = online.OnlineDNNCalibration(dec, 20)
  hoc.run(calib, *tensors, [frames])
  r = calib.finish()
  fresh = hdc.bank(st, reduction=reduction, lda=tuple(r.lda[0].cpu().numpy()) if reduction == 'lda' else None,
                   width=width, hop=hop, stats=tuple(r.corr[0, 0].cpu().numpy()))
  assert np.array_equal(fresh._dev['corr'].cpu().numpy(), r.corr.cpu().numpy())
  if reduction == 'lda':
    assert np.array_equal(fresh._dev['lda'].cpu().numpy(), r.lda.cpu().numpy())
  h = dev.default_handle()
  head = _windows(dec, tensors, 0, cut)
  params = dec._dev['params'].clone()
  dec.set_statistics(r.corr, r.lda)
  assert dec._dev['corr'].data_ptr() != r.corr.data_ptr() and np.array_equal(dec._dev['params'].cpu().numpy(),
                                                                             params.cpu().numpy())
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
  assert got_d[first:].tobytes() == want_d[first:].tobytes()


def test_refusals_leave_the_state_and_the_next_finish_is_served(dev):
  """Each status by name -- no completed window, zero power, equal class means, in one bank --, the state untouched,
  the next finish served."""
  import torch
  from telluride_decoding_amd import online
  frames, width = 80, 10
  st = hdc.stretch((5, 2, 9), [16], frames)
  post = st['post']
  eeg, att, unatt = _tensors(st)
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
  calib.push(eeg[:18], att[:18], unatt[:18])                 # 9 frames counted: no window of 10
  before = calib._dev['state'].clone()
  with pytest.raises(ValueError, match='OnlineDNNCalibration.finish: session 0: No data for class 0'):
    calib.finish()
  assert torch.equal(calib._dev['state'], before)
  calib.push(eeg[18:], att[18:], unatt[18:])
  calib.flush()
  served = calib.finish()
  assert float(served.dprime[0]) > 0 and np.array_equal(
      calib.sums()[0].cpu().numpy(), hoc.twin_sums(_device_pred(dev, st), st['att'], st['unatt'], width))
  # session 1: zero weights, so every prediction is the output bias 0.5 and every sum exact; session 2: one envelope
  # twice
  bank = hdc.bank(st, weights=[st['weights'], hdc.constant_model(st), st['weights']])
  calib = online.OnlineDNNCalibration(bank, width)
  calib.push(torch.stack([eeg] * 3), torch.stack([att] * 3), torch.stack([unatt, unatt, att]))
  state = calib._dev['state']
  before = state.clone()
  assert float(calib.sums()[1, 0]) == 0.5 * (frames - post)
  out = dev.online_calib_finish(state, calib.frames_emitted, width)
  assert out.status.cpu().tolist() == [dev.CALIB_OK, dev.CALIB_NO_POWER, dev.CALIB_SAME_MEANS]
  assert bool(torch.isnan(out.dprime[1:]).all()) and bool(torch.isnan(out.corr[1]).all())
  with pytest.raises(ValueError, match='session 1: the correlation power'):
    calib.finish()
  assert torch.equal(state, before)
  calib.push(torch.stack([eeg[:5]] * 3), torch.stack([att[:5]] * 3), torch.stack([unatt[:5], att[:5], unatt[:5]]))
  assert not torch.equal(state, before)


def test_invalid_arguments_queue_nothing(dev):
  """Every bad argument of td_fccalib_online_push returns TD_ERR_INVALID, by the entry point's name, with no launch
  and the state bytes unchanged; the good arguments are then served.  The wrapper's own refusals too."""
  import torch
  from telluride_decoding_amd import _lib
  shape, hidden = (5, 2, 9), [16]
  c, pre, post = shape
  st = hdc.stretch(shape, hidden, 80)
  sessions, n, width = 2, 50, 10
  h = dev.default_handle()
  nbytes = dev.online_dnn_calib_state_bytes(c, pre, post)
  count = dev.dnn_param_count(c * (pre + 1 + post), hidden)
  eeg = torch.stack([_up(st['eeg'][:n])] * sessions)
  env = torch.stack([torch.stack([_up(st['att'][:n]), _up(st['unatt'][:n])], dim=1)] * sessions)
  params = torch.stack([_up(hd.packed(st['weights']))] * sessions)
  state = torch.zeros((sessions, nbytes), dtype=torch.uint8, device='cuda')
  dev.online_dnn_calib_push(eeg, env, params, hidden, state, 0, pre, post, width)
  before = state.clone()
  hid = np.array(hidden, np.int32)
  hid_p = hid.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
  bad_hidden = [np.array(v, np.int32) for v in ([0], [65], [16] * 5)]
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())
  null = ctypes.c_void_p(0)
  good = dict(h=h.ptr, sessions=sessions, eeg=ptr(eeg), eeg_ld=c, eeg_ss=n * c, env=ptr(env), env_ld=2, env_ss=2 * n,
              n=n, frames_before=n, c=c, pre=pre, post=post, hidden=hid_p, num_hidden=1, params=ptr(params),
              params_ss=count, width=width, flush=0, state=ptr(state), state_ss=nbytes)
  as_p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
  bad = [dict(h=None), dict(sessions=0), dict(sessions=65536), dict(eeg=null), dict(env=null), dict(eeg_ld=c - 1),
         dict(env_ld=1), dict(eeg_ss=c - 1), dict(env_ss=1), dict(n=-1), dict(n=1048577), dict(frames_before=-1),
         dict(c=0), dict(c=129), dict(pre=-1), dict(post=-1), dict(pre=32, post=32), dict(num_hidden=-1),
         dict(num_hidden=5, hidden=as_p(bad_hidden[2])), dict(hidden=ctypes.POINTER(ctypes.c_int)()),
         dict(hidden=as_p(bad_hidden[0])), dict(hidden=as_p(bad_hidden[1])), dict(params=null),
         dict(params_ss=count - 1), dict(params_ss=-1), dict(width=0), dict(width=65537), dict(state=null),
         dict(state_ss=nbytes - 8), dict(state_ss=nbytes + 4)]
  h.profile_enable(True)
  h.profile_read()
  for change in bad:
    args = dict(good)
    args.update(change)
    status = h.lib.td_fccalib_online_push(*args.values())
    assert status == _lib.TD_ERR_INVALID, change
    if 'h' not in change:
      with pytest.raises(ValueError, match='td_fccalib_online_push'):
        h.check(status)
  assert h.profile_read()[0] == 0
  assert h.lib.td_fccalib_online_push(*dict(good, n=0).values()) == 0 and h.profile_read()[0] == 0   # an empty push
  assert torch.equal(state, before)
  assert h.lib.td_fccalib_online_push(*good.values()) == 0 and h.profile_read()[0] == 1
  h.profile_enable(False)
  assert not torch.equal(state, before)
  before = state.clone()
  for call, match in ((lambda: dev.online_dnn_calib_push(eeg, env, params[:, :-1], hidden, state, n, pre, post, width),
                       'parameters for hidden layers'),
                      (lambda: dev.online_dnn_calib_push(eeg[:, :, :4], env, params, hidden, state, n, pre, post, width),
                       'eeg of'),
                      (lambda: dev.online_dnn_calib_push(eeg, env, params, hidden, state, n, pre, post, 0),
                       'window of 0'),
                      (lambda: dev.online_dnn_calib_push(eeg[:1], env[:1], params[:1], hidden, state[:1, :-8], n, pre,
                                                         post, width), 'state stride'),
                      (lambda: dev.online_calib_finish(state[:1, :8 * 28], n, width), 'state stride')):
    with pytest.raises(ValueError, match=match):
      call()
  assert torch.equal(state, before)
