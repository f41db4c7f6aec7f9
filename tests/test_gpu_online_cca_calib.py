"""The online CCA calibration on the GPU (td_ccacalib_online_push / _sums / _finish, online.OnlineCCACalibration,
OnlineDecoder.set_cca_statistics): labelled stretches of 300 frames (130 for the two large shapes) at the shapes where
the kernel can go wrong -- no tails at all, both tails with either view's post the longer, dims that are no multiple of
the projection's block of 4, k1 = 1344 (five rounds of the four accumulators and a remainder), 16 dims (2624 state
doubles, more than a workgroup's threads), the largest LDS, a pass that is halved -- and windows of 1, 7 and 100 frames.
The sums bit for bit against the NumPy twin fed with td_cca_online_push's own projections, every cut byte for byte,
finish against the two-pass float64 route and against the batch route, the host evaluation against finish, a padded
bank against its sessions, one launch per push, the calibrator following set_cca_model, and a running bank after
set_cca_statistics against a fresh one."""
import numpy as np
import pytest

from tests import host_online_cca_calib as hcal
from tests import parity_log

pytestmark = pytest.mark.gpu

# (view 1, view 2, dims, frames)
SHAPES = [((3, 0, 0), (2, 0, 0), 1, 300), ((5, 2, 9), (3, 1, 4), 2, 300), ((3, 1, 2), (2, 0, 6), 3, 300),
          ((64, 0, 20), (8, 0, 15), 5, 130), ((5, 0, 0), (16, 0, 0), 16, 300), ((128, 3, 12), (32, 0, 0), 8, 130)]
# beside the issue's: the largest rotations in 16 dims, where the pass of 64 frames is halved
HALVED = ((128, 3, 12), (32, 0, 0), 16, 130)


def _id(shape):
  (c1, pre1, post1), (c2, pre2, post2), dims, frames = shape
  return 'v%d_%d_%d_v%d_%d_%d_d%d_n%d' % (c1, pre1, post1, c2, pre2, post2, dims, frames)


IDS = [_id(s) for s in SHAPES]
WIDTHS = (1, 7, 100)
# (shape, width): every shape at 1 and 7 (at least 2 dims windows per class), and the 16-dim shape at 100 on a stretch
# of 3000 frames (30 windows per class)
DISTANCES = [(s, w) for s in SHAPES for w in (1, 7)] + [(((5, 0, 0), (16, 0, 0), 16, 3000), 100)]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _up(a):
  import torch
  return torch.from_numpy(np.array(a, order='C')).to('cuda')       # (a copy: the shared stretches are read-only)


def _stretch(shape, seed=0):
  view1, view2, dims, frames = shape
  return hcal.stretch(view1, view2, dims, frames, seed)


def _bank(st, sessions=1, reduction='first', lda=None, width=20, hop=10, kind='wta', stats=None):
  from telluride_decoding_amd import online
  decs = [hcal.decoder_of(st, reduction, lda, stats) for _ in range(sessions)]
  return online.OnlineDecoder(decs, width, hop, decoder_type=kind)


def _tensors(st):
  return _up(st['eeg']), _up(st['att']), _up(st['unatt'])


_PROJ = {}


def _device_proj(dev, st, model=None):
  """td_cca_online_push's float32 projections (a, b1, b0) of every frame of a stretch (one push and the flush,
  want_frames; the attended block as speaker 1), with the stretch's own model or the one given: once per key,
  read-only."""
  import torch
  model = model or st
  key = (id(st['eeg']), id(model['rot_x']))                       # (hcal.stretch keeps its arrays alive)
  if key not in _PROJ:
    (c1, pre1, post1), (c2, pre2, post2), dims, frames = st['view1'], st['view2'], st['dims'], st['frames']
    eeg, att, unatt = (t[None] for t in _tensors(st))
    state = torch.zeros((1, dev.cca_online_state_bytes(c1, pre1, post1, c2, pre2, post2, 4)), dtype=torch.uint8,
                        device='cuda')
    corr = torch.ones((1, 2, 3, dims), dtype=torch.float64, device='cuda')
    m = [_up(model[k])[None] for k in ('mean_x', 'rot_x', 'mean_y', 'rot_y')]
    first = dev.cca_online_push(eeg, att, unatt, *m, corr, state, 0, pre1, post1, pre2, post2, 4, 4,
                                want_frames=True)
    last = dev.cca_online_push(None, None, None, *m, corr, state, frames, pre1, post1, pre2, post2, 4, 4, flush=True,
                               want_frames=True)
    proj = torch.cat([first.proj[0], last.proj[0]]).cpu().numpy()
    assert proj.shape == (frames, 3 * dims) and proj.dtype == np.float32
    _PROJ[key] = (proj[:, :dims], proj[:, dims:2 * dims], proj[:, 2 * dims:])
  return _PROJ[key]


def _twin(dev, st, width, m=None, model=None):
  a, b1, b0 = _device_proj(dev, st, model)
  m = st['frames'] if m is None else m
  return hcal.twin_sums(a[:m], b1[:m], b0[:m], width)


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES + [HALVED], ids=IDS + [_id(HALVED)])
def test_sums_are_the_twins_bits_after_every_push(dev, shape, width):
  """sums() == twin_sums(proj of device.cca_online_push(..., want_frames=True), W) with np.array_equal after every
  push (one of them shorter than the tails, one empty) and after the flush: the projection's order and the sums'
  order at once."""
  from telluride_decoding_amd import online
  st = _stretch(shape)
  dims, frames = st['dims'], st['frames']
  assert dev.gpu_available()
  calib = online.OnlineCCACalibration(_bank(st), width)
  step = dev.online_ccacalib_lds_bytes(*st['view1'], *st['view2'], dims, frames)[0]
  assert (step < 64) == (shape == HALVED)
  eeg, att, unatt = _tensors(st)

  def check(at, flushed=False):
    m = at if flushed else max(0, at - calib.delay)
    got = calib.sums()
    assert got.is_cuda and tuple(got.shape) == (1, hcal.sums_count(dims)) and str(got.dtype) == 'torch.float64'
    assert np.array_equal(got[0].cpu().numpy(), _twin(dev, st, width, m)), (at, flushed)

  hcal.run(calib, eeg, att, unatt, [frames // 3, 1, 0, 5, frames - frames // 3 - 6], after_push=check)
  check(frames, True)
  assert calib.windows == frames // width


_WHOLE = {}


def _whole(shape, width):
  """(state bytes, sums) after the whole stretch in one push and an empty flush: once per (shape, W), read-only."""
  from telluride_decoding_amd import online
  key = (shape, width)
  if key not in _WHOLE:
    st = _stretch(shape)
    calib = online.OnlineCCACalibration(_bank(st), width)
    hcal.run(calib, *_tensors(st), [st['frames']])
    _WHOLE[key] = (calib._dev['state'].clone(), calib.sums().clone())
  return _WHOLE[key]


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_any_cut_of_the_stretch_gives_the_same_state_bytes(dev, shape, width):
  """Pushes of 1 (shorter than the tails), W - 1, W, W + 1, random 0 .. 40 with empty pushes, whole, an empty push in
  the middle; flushed by a flushing last push and by an empty flushing push: the state block byte for byte -- sums,
  EEG tail and both feature tails."""
  import torch
  from telluride_decoding_amd import online
  st = _stretch(shape)
  (c1, pre1, post1), (c2, pre2, post2), dims, frames = shape
  want_state, want_sums = _whole(shape, width)
  calib = online.OnlineCCACalibration(_bank(st), width)
  eeg, att, unatt = _tensors(st)
  for name, sizes in hcal.cuts(frames, width).items():
    for flush_last in (False, True):
      hcal.run(calib, eeg, att, unatt, sizes, flush_last=flush_last)
      assert torch.equal(calib._dev['state'], want_state), (name, flush_last)
  assert torch.equal(calib.sums(), want_sums)
  tail = calib._dev['state'][0, 8 * hcal.sums_count(dims):].view(torch.float32)
  post = max(post1, post2)
  t1, t2 = pre1 + post, pre2 + post
  assert torch.equal(tail[:t1 * c1].reshape(t1, c1), eeg[frames - t1:])
  feats = tail[t1 * c1:t1 * c1 + 2 * t2 * c2].reshape(2, t2, c2)
  assert torch.equal(feats[0], att[frames - t2:]) and torch.equal(feats[1], unatt[frames - t2:])


def _result(r, i=0):
  return hcal.result_of(r.corr[i].cpu().numpy(), r.lda[i].cpu().numpy(), float(r.dprime[i].cpu()))


@pytest.mark.parametrize('shape,width', DISTANCES, ids=['%s_w%d' % (_id(s), w) for s, w in DISTANCES])
def test_finish_against_the_two_pass_route_and_the_batch_route(dev, shape, width):
  """finish against Decoder.train's two passes in float64 on the same float32 projections (oracle Correlator fed
  class 0 then class 1, average_data, scaled_lda_fit, calculate_dprime) at the CPU test's bars -- <= 1e-10 on the
  statistics, slope w and the intercept, <= 1e-9 on d' --; for W >= 2 against the route the library had, at the same
  bars: device.window_sums per class into Decoder._add_sums, device.window_class_moments per class,
  fit_class_moments; and the host evaluation (update_decoder) against finish at 1e-12."""
  import torch
  from telluride_decoding_amd import infer_decoder, online, scaled_lda
  st = _stretch(shape)
  dims, frames = st['dims'], st['frames']
  assert frames // width >= min(2 * dims, 30)
  a, b1, b0 = _device_proj(dev, st)
  calib = online.OnlineCCACalibration(_bank(st), width)
  hcal.run(calib, *_tensors(st), [frames // 2, frames - frames // 2])
  r = calib.finish()
  assert r.corr.is_cuda and tuple(r.corr.shape) == (1, 2, 3, dims) and tuple(r.lda.shape) == (1, dims + 2)
  assert torch.equal(r.corr[0, 0], r.corr[0, 1])
  if dims == 1:
    assert float(r.lda[0, 0]) == 1.0
  got = _result(r)
  err, err_d = hcal.distances(got, hcal.two_pass(a, b1, b0, width))
  print('%s W = %d: two-pass corr / lda %.3g, d\' %.3g' % (_id(shape), width, err, err_d))
  record = dict(two_pass=err, two_pass_dprime=err_d)
  batch = batch_d = None
  if width >= 2:
    ad = _up(a)
    streams = [(ad, _up(b0)), (ad, _up(b1))]
    dec = infer_decoder.Decoder()
    for x, y in streams:
      dec._add_sums(frames, dev.window_sums(x, y, [0, frames], frames, frames).cpu().numpy()[0])
    mx, my, pw = dec._stat_vectors(dims)
    moments = [dev.window_class_moments(x, y, width, mx, my, pw).cpu().numpy() for x, y in streams]
    lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    lda.fit_class_moments(moments)
    (m1, v1), (m2, v2) = lda.projected_class_stats()
    want = dict(corr=np.stack([mx, my, pw]), axis=np.real(lda.slope * np.asarray(lda.coef_array)[:, 0]),
                intercept=float(np.real(lda.intercept)), dprime=(m2 - m1) / np.sqrt((v1 + v2) / 2.0))
    batch, batch_d = hcal.distances(got, want)
    print('%s W = %d: batch route corr / lda %.3g, d\' %.3g' % (_id(shape), width, batch, batch_d))
    record.update(batch=batch, batch_dprime=batch_d)
  # update_decoder evaluates the same closed form on the host: the parameters a saved decoder gets are finish's
  dec = hcal.decoder_of(st, 'lda', np.ones(dims + 2))
  dprime = calib.update_decoder(dec)
  p = online.cca_session_parameters(dec)
  host = hcal.result_of(p['corr'], p['lda'], dprime)
  host_err = max(hcal.distances(host, got))
  record.update(host=host_err)
  parity_log.record('online_ccacalib_%s_w%d' % (_id(shape), width), **record)
  assert host_err <= 1e-12
  assert err <= 1e-10
  assert err_d <= 1e-9
  if width >= 2:
    assert batch <= 1e-10
    assert batch_d <= 1e-9


def test_a_padded_bank_is_its_sessions(dev):
  """Three sessions with different rows and different models, every stride padded (rows wider and longer than the
  bank reads, a state row longer than a block), against three single sessions: state bytes and finish exactly."""
  import torch
  view1, view2, dims, frames, width = (5, 2, 9), (3, 1, 4), 2, 300, 7
  (c1, pre1, post1), (c2, pre2, post2) = view1, view2
  sts = [hcal.stretch(view1, view2, dims, frames, seed=s) for s in range(3)]
  nbytes = dev.online_ccacalib_state_bytes(c1, pre1, post1, c2, pre2, post2, dims)
  eeg = torch.zeros((3, frames + 5, c1 + 3), device='cuda')
  feat = torch.zeros((2, 3, frames + 2, c2 + 1), device='cuda')
  for i, s in enumerate(sts):
    eeg[i, :frames, :c1], feat[0, i, :frames, :c2], feat[1, i, :frames, :c2] = _tensors(s)
  eeg, att, unatt = eeg[:, :frames, :c1], feat[0, :, :frames, :c2], feat[1, :, :frames, :c2]
  model = [torch.stack([_up(s[k]) for s in sts]) for k in ('mean_x', 'rot_x', 'mean_y', 'rot_y')]
  state = torch.zeros((3, nbytes + 16), dtype=torch.uint8, device='cuda')[:, :nbytes]
  args = (pre1, post1, pre2, post2, width)
  at = 0
  for n in (130, 1, 0, 169):
    at = dev.online_ccacalib_push(eeg[:, at:at + n], att[:, at:at + n], unatt[:, at:at + n], *model, state, at, *args)
  assert dev.online_ccacalib_push(None, None, None, *model, state, at, *args, flush=True) == frames
  sums = dev.online_ccacalib_sums(state, dims)
  out = dev.online_ccacalib_finish(state, dims, frames, width)
  assert not bool(out.status.any())
  for i, s in enumerate(sts):
    single = torch.zeros((1, nbytes), dtype=torch.uint8, device='cuda')
    rows = [t[None] for t in _tensors(s)]
    dev.online_ccacalib_push(*rows, *[m[i:i + 1] for m in model], single, 0, *args, flush=True)
    assert torch.equal(state[i], single[0]), i
    assert torch.equal(sums[i], dev.online_ccacalib_sums(single, dims)[0])
    one = dev.online_ccacalib_finish(single, dims, frames, width)
    for got, want in zip(out, one):
      assert torch.equal(got[i], want[0]), i
    assert np.array_equal(sums[i].cpu().numpy(), _twin(dev, s, width))
  assert not torch.equal(sums[0], sums[1])


def test_one_launch_per_push_and_one_for_finish(dev):
  """td_profile_read counts ONE launch for a push with rows (also one that emits nothing), none for an empty push,
  one for the flush, one for finish; two identical runs give the same bytes."""
  import torch
  from telluride_decoding_amd import online
  shape, width = SHAPES[3], 7
  st = _stretch(shape)
  frames, delay = st['frames'], 20
  eeg, att, unatt = _tensors(st)
  h = dev.default_handle()
  calib = online.OnlineCCACalibration(_bank(st), width)
  runs = []
  for attempt in range(2):
    calib.reset()
    h.profile_enable(True)
    h.profile_read()
    at = 0
    for n in (5, 0, 1, 37, 87):                              # (the first push emits nothing: 5 <= delay)
      calib.push(eeg[at:at + n], att[at:at + n], unatt[at:at + n])
      assert h.profile_read()[0] == (1 if n else 0), n
      at += n
    assert calib.frames_emitted == frames - delay
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


def test_the_calibrator_follows_set_cca_model(dev):
  """After decoder.set_cca_model the next push projects with the new model: the sums are the twin's, fed the old
  model's projections up to the swap and the new model's behind it."""
  from telluride_decoding_amd import online
  shape, width, cut = SHAPES[1], 7, 130
  st = _stretch(shape)
  other = _stretch(shape, seed=1)
  eeg, att, unatt = _tensors(st)
  bank = _bank(st)
  calib = online.OnlineCCACalibration(bank, width)
  calib.push(eeg[:cut], att[:cut], unatt[:cut])
  bank.set_cca_model(*[_up(other[k]) for k in ('mean_x', 'rot_x', 'mean_y', 'rot_y')])
  calib.push(eeg[cut:], att[cut:], unatt[cut:])
  calib.flush()
  k = cut - calib.delay                                      # frames counted before the swap
  old, new = _device_proj(dev, st), _device_proj(dev, st, other)
  a, b1, b0 = (np.concatenate([o[:k], n[k:]]) for o, n in zip(old, new))
  assert np.array_equal(calib.sums()[0].cpu().numpy(), hcal.twin_sums(a, b1, b0, width))
  assert not np.array_equal(a, old[0])


@pytest.mark.parametrize('reduction', ['first', 'mean', 'lda'])
def test_a_running_bank_after_set_cca_statistics(dev, reduction):
  """A bank trained with other statistics is pushed 130 rows, takes OnlineCCACalibration.finish's corr and lda device
  to device, and is pushed the rest: from the first window that lies wholly behind the swap its scores and its
  winner-take-all decisions are byte for byte those of a fresh bank built with those parameters and pushed the same
  rows.  The rotations are untouched, and a push is still one launch."""
  from telluride_decoding_amd import online
  view1, view2, dims, frames = (5, 2, 9), (3, 1, 4), 2, 600
  width, hop, cut = 20, 10, 130
  st = hcal.stretch(view1, view2, dims, frames)
  tensors = _tensors(st)
  old_lda = np.array([1.0, -0.5, 2.0, -0.5]) if reduction == 'lda' else None
  old_stats = np.stack([np.full(dims, 0.3), np.full(dims, -0.4), np.full(dims, 2.0)])
  dec = _bank(st, reduction=reduction, lda=old_lda, width=width, hop=hop, stats=old_stats)
  calib = online.OnlineCCACalibration(dec, 20)
  hcal.run(calib, *tensors, [frames])
  r = calib.finish()
  trained = hcal.decoder_of(st, reduction, r.lda[0].cpu().numpy() if reduction == 'lda' else None,
                            stats=r.corr[0, 0].cpu().numpy())
  fresh = online.OnlineDecoder(trained, width, hop)
  assert np.array_equal(fresh._dev['corr'].cpu().numpy(), r.corr.cpu().numpy())
  if reduction == 'lda':
    assert np.array_equal(fresh._dev['lda'].cpu().numpy(), r.lda.cpu().numpy())

  def windows(bank, lo, hi):
    out = bank.push(*[t[lo:hi] for t in tensors])
    return out.scores[0], out.decisions[0]

  h = dev.default_handle()
  head = windows(dec, 0, cut)
  rot = dec._dev['rot_x'].clone()
  dec.set_cca_statistics(r.corr, r.lda if reduction == 'lda' else None)
  assert dec._dev['corr'].data_ptr() != r.corr.data_ptr() and np.array_equal(dec._dev['rot_x'].cpu().numpy(),
                                                                             rot.cpu().numpy())
  h.profile_enable(True)
  h.profile_read()
  rest = windows(dec, cut, frames)
  assert h.profile_read()[0] == 1
  h.profile_enable(False)
  last = dec.flush()
  got_s = np.concatenate([head[0], rest[0], last.scores[0]])
  got_d = np.concatenate([head[1], rest[1], last.decisions[0]])
  parts = [windows(fresh, 0, cut), windows(fresh, cut, frames)]
  last = fresh.flush()
  want_s = np.concatenate([parts[0][0], parts[1][0], last.scores[0]])
  want_d = np.concatenate([parts[0][1], parts[1][1], last.decisions[0]])
  assert got_s.shape == want_s.shape == ((frames - width) // hop + 1, 2)
  first = -(-(cut - dec.delay) // hop)                       # the first window that begins at or behind the swap
  assert 0 < first < got_s.shape[0] - 20
  assert got_s[first:].tobytes() == want_s[first:].tobytes()
  assert got_s[:first].tobytes() != want_s[:first].tobytes()
  assert got_d[first:].tobytes() == want_d[first:].tobytes()


def test_refusals_leave_the_state_and_the_next_finish_is_served(dev):
  """Each status by name -- no completed window, too few windows for the scatter, zero power, equal class means --,
  the state untouched, the next finish served; the refusals the device calls make."""
  import torch
  from telluride_decoding_amd import online
  shape, width = SHAPES[2], 10
  st = _stretch(shape)
  (c1, pre1, post1), (c2, pre2, post2), dims, frames = shape
  delay = max(post1, post2)
  eeg, att, unatt = _tensors(st)
  calib = online.OnlineCCACalibration(_bank(st), width)
  calib.push(eeg[:delay + 9], att[:delay + 9], unatt[:delay + 9])              # 9 frames counted: no window of 10
  before = calib._dev['state'].clone()
  with pytest.raises(ValueError, match='session 0: No data for class 0'):
    calib.finish()
  calib.push(eeg[delay + 9:delay + 20], att[delay + 9:delay + 20], unatt[delay + 9:delay + 20])
  assert calib.windows == 2                                                      # 4 windows in all < dims + 2
  before = calib._dev['state'].clone()
  with pytest.raises(ValueError, match='session 0: the pooled scatter .* not positive definite'):
    calib.finish()
  assert torch.equal(calib._dev['state'], before)
  calib.push(eeg[delay + 20:], att[delay + 20:], unatt[delay + 20:])
  calib.flush()
  served = calib.finish()
  assert float(served.dprime[0]) > 0 and np.array_equal(calib.sums()[0].cpu().numpy(), _twin(dev, st, width))
  # session 1: a zero EEG rotation, so every projection a is 0.0 and its power zero; session 2: one block twice
  bank = _bank(st, sessions=3)
  model = {k: np.stack([st[k]] * 3) for k in ('mean_x', 'rot_x', 'mean_y', 'rot_y')}
  model['rot_x'][1] = 0.0
  bank.set_cca_model(model['mean_x'], model['rot_x'], model['mean_y'], model['rot_y'])
  calib = online.OnlineCCACalibration(bank, width)
  calib.push(torch.stack([eeg] * 3), torch.stack([att] * 3), torch.stack([unatt, unatt, att]))
  state = calib._dev['state']
  before = state.clone()
  out = dev.online_ccacalib_finish(state, dims, calib.frames_emitted, width)
  assert out.status.cpu().tolist() == [dev.CALIB_OK, dev.CALIB_NO_POWER, dev.CALIB_SAME_MEANS]
  assert bool(torch.isnan(out.dprime[1:]).all()) and bool(torch.isnan(out.corr[1]).all())
  assert bool(torch.isnan(out.lda[1:]).all()) and not bool(torch.isnan(out.corr[2]).any())
  with pytest.raises(ValueError, match='session 1: the correlation power of a dim'):
    calib.finish()
  assert torch.equal(state, before)
  zeros = torch.zeros((3, 50, c1), device='cuda')
  feat = torch.zeros((3, 50, c2), device='cuda')
  m = [bank._dev[k] for k in ('mean_x', 'rot_x', 'mean_y', 'rot_y')]
  for kwargs, match in ((dict(width=0), 'window of 0'), (dict(width=65537), 'window of 65537'),
                        (dict(frames_before=-1), 'frames before')):
    args = dict(frames_before=50, width=width)
    args.update(kwargs)
    with pytest.raises(ValueError, match='td_ccacalib_online_push.*' + match):
      dev.online_ccacalib_push(zeros, feat, feat, *m, state, args['frames_before'], pre1, post1, pre2, post2,
                               args['width'])
  with pytest.raises(ValueError, match='lags'):
    dev.online_ccacalib_push(zeros, feat, feat, *m, state, 50, pre1 + 1, post1, pre2, post2, width)
  with pytest.raises(ValueError, match='state stride'):
    dev.online_ccacalib_push(zeros[:1], feat[:1], feat[:1], *[t[:1] for t in m], state[:1, :-8], 50, pre1, post1,
                             pre2, post2, width)
  with pytest.raises(ValueError, match='state stride'):
    dev.online_ccacalib_finish(state[:1, :8 * (hcal.sums_count(dims) - 1)], dims, 50, width)
  with pytest.raises(ValueError, match='window of 0'):
    dev.online_ccacalib_finish(state, dims, 50, 0)
  for bad in (0, 17):
    with pytest.raises(ValueError, match='%d dims' % bad):
      dev.online_ccacalib_finish(state, bad, 50, width)
    with pytest.raises(ValueError, match='%d dims' % bad):
      dev.online_ccacalib_sums(state, bad)
  assert torch.equal(state, before)
  calib.push(torch.stack([eeg[:5]] * 3), torch.stack([att[:5]] * 3), torch.stack([unatt[:5], att[:5], unatt[:5]]))
  assert not torch.equal(state, before)
