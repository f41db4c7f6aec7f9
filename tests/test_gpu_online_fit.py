"""The online ridge fit on the GPU (td_fit_online_push / _moments / _solve, online.OnlineRidgeFit): white-noise
recordings of 300 frames (120 for the two large shapes and the full tile) at the shapes where the tiling can go wrong -- the moments and
the tails bit for bit against the NumPy session with and without forgetting, every cut byte for byte through both
tail copies, the moments against LagStats and the weights against float64 and against LagStats.ridge_solve, a bank
against its sessions, one launch per push, repeatability, OnlineDecoder.set_weights device to device, and a singular
system reported, not faulted.

The lambdas.  The weights are compared where a bound on the moments is a bound on the weights: white noise of n frames
and K lagged inputs has the eigenvalues of its covariance inside (1 -+ sqrt(K / n))^2 (Marchenko-Pastur), so the small
shapes (K / n <= 0.42: [0.12, 2.7]) have condition numbers <= 22 at any lambda and the large ones (n = 120 < K:
singular without a ridge, largest eigenvalue <= (1 + sqrt(2048 / 120))^2 = 26.3) <= 27.3 from lambda = 1 on; the
full-tile shape (K = 63, n = 120: [0.08, 3.0]) <= 3.7 from lambda = 1 on.  LagStats
holds its moments to 2^-22 (the two-piece float16 product), so cond x 2.4e-7 <= 1e-5 needs cond <= 41: lambdas 0.1, 1
and 10 for the small shapes, 1 and 10 for the shapes of 120 frames."""
import numpy as np
import pytest

from tests import host_online
from tests import host_online_fit as hof
from tests import parity_log

pytestmark = pytest.mark.gpu

# (c, pre, post, d, frames): no tail at all; K + 1 = 127, one short of two tiles; K + 1 = 65, the bias row alone in a
# second tile, with the widest d; K + 1 = 1345 = 21 x 64 + 1; K + 1 = 2049, the limit; K + 1 = 64, one full tile with
# the ones column its last, and d = 5: one lane of a B thread's second output
SHAPES = [(5, 2, 9, 1, 300), (3, 0, 0, 2, 300), (63, 1, 0, 1, 300), (16, 3, 0, 8, 300), (64, 0, 20, 1, 120),
          (128, 0, 15, 1, 120), (21, 1, 1, 5, 120)]
IDS = ['c%d_pre%d_post%d_d%d_n%d' % s for s in SHAPES]


def _lambdas(frames):
  return (0.1, 1.0, 10.0) if frames == 300 else (1.0, 10.0)


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _up(a):
  import torch
  return torch.from_numpy(np.array(a, order='C')).to('cuda')       # (a copy: the shared recordings are read-only)


_WHOLE = {}


def _whole(shape, forget):
  """(the fit after the whole recording in one push and an empty flush, its moments, its tails, the device
  recording): once per (shape, g), read-only."""
  from telluride_decoding_amd import online
  key = (shape, forget)
  if key not in _WHOLE:
    c, pre, post, d, frames = shape
    eeg, target = hof.recording(c, d, frames)
    xe, xt = _up(eeg), _up(target)
    fit = online.OnlineRidgeFit(c, pre, post, outputs=d, forgetting=forget)
    hof.run(fit, xe, xt, [frames])
    a, b = fit.moments()
    _WHOLE[key] = (fit, a.clone(), b.clone(), [t.clone() for t in fit.tails], xe, xt)
  return _WHOLE[key]


@pytest.mark.parametrize('forget', hof.FORGETS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_moments_and_tails_are_the_numpy_sessions_bits(dev, shape, forget):
  """np.array_equal with online._HostRidgeFitSession -- A * g + np.outer(v, v) per frame in frame order -- after
  three pushes and the flush; A symmetric, A[K][K] the (effective) count."""
  from telluride_decoding_amd import online
  c, pre, post, d, frames = shape
  eeg, target = hof.recording(c, d, frames)
  assert dev.gpu_available()
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d, forgetting=forget)
  host = online._HostRidgeFitSession(c, pre, post, d, forget)
  sizes, at = [frames // 3, 1, frames - frames // 3 - 1], 0
  xe, xt = _up(eeg), _up(target)
  for n in sizes:
    fit.push(xe[at:at + n], xt[at:at + n])
    host.push(eeg[at:at + n], target[at:at + n], at, False)
    at += n
    tails = fit.tails
    assert np.array_equal(tails[0][0].cpu().numpy(), host.tail), at
    assert np.array_equal(tails[1][0].cpu().numpy(), host.target_tail), at
  a, b = fit.moments()
  assert np.array_equal(a[0].cpu().numpy(), host.a) and np.array_equal(b[0].cpu().numpy(), host.b)
  fit.flush()
  host.push(eeg[:0], target[:0], at, True)
  a, b = (t[0].cpu().numpy() for t in fit.moments())
  assert a.dtype == np.float64 and a.shape == (fit.inputs + 1,) * 2 and b.shape == (fit.inputs + 1, d)
  assert np.array_equal(a, host.a) and np.array_equal(b, host.b)
  assert np.array_equal(a, a.T)
  if forget == 1.0:
    assert a[-1, -1] == frames
  whole = _whole(shape, forget)
  assert np.array_equal(whole[1][0].cpu().numpy(), a) and np.array_equal(whole[2][0].cpu().numpy(), b)


@pytest.mark.parametrize('forget', hof.FORGETS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_any_cut_of_the_recording_gives_the_same_bits(dev, shape, forget):
  """Pushes of 1, of pre + post - 1, of 7, random 0 .. 40 with empty pushes, whole, and an empty push in the middle;
  flushed by a flushing last push and by an empty flushing push; the cuts reach the last frame after an odd and after
  an even number of pushes with rows, so both tail copies end up live: moments and tails byte for byte."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, d, frames = shape
  _, want_a, want_b, want_tails, xe, xt = _whole(shape, forget)
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d, forgetting=forget)
  parities = set()
  for name, sizes in hof.cuts(frames, pre, post).items():
    for flush_last in (False, True):
      hof.run(fit, xe, xt, sizes, flush_last=flush_last)
      parities.add(fit._pushes & 1)
      a, b = fit.moments()
      assert torch.equal(a, want_a) and torch.equal(b, want_b), (name, flush_last)
      tails = fit.tails
      assert torch.equal(tails[0], want_tails[0]) and torch.equal(tails[1], want_tails[1]), (name, flush_last)
  assert parities == {0, 1}


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_moments_against_lagstats(dev, shape):
  """The recording accumulated as one file by LagStats(c, pre, post, d=d): .moments() within the project's 1e-5
  relative bar (tests/test_gpu_fit.py, _rel); and within 1e-12 of [oracle.lag.lag_matrix | 1]'s in float64."""
  c, pre, post, d, frames = shape
  _, a, b, _, xe, xt = _whole(shape, 1.0)
  stats = dev.LagStats(c, pre, post, d=d)
  stats.accumulate(xe, y=xt)
  m = stats.moments()
  a, b = a[0].cpu().numpy(), b[0].cpu().numpy()
  err_a, err_b = hof.rel(m['xtx'].cpu().numpy(), a), hof.rel(m['xty'].cpu().numpy(), b)
  want_a, want_b = hof.reference_moments(c, pre, post, d, frames)
  exact_a, exact_b = hof.rel(a, want_a), hof.rel(b, want_b)
  print('%s: LagStats xtx %.3g xty %.3g; float64 xtx %.3g xty %.3g' % (shape, err_a, err_b, exact_a, exact_b))
  parity_log.record('online_fit_moments_c%d_pre%d_post%d_d%d' % shape[:4], lagstats_xtx=err_a, lagstats_xty=err_b,
                    float64_xtx=exact_a, float64_xty=exact_b)
  assert err_a <= 1e-5 and err_b <= 1e-5
  assert exact_a <= 1e-12 and exact_b <= 1e-12


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_solve_against_float64_and_lagstats(dev, shape):
  """np.linalg.solve of the reference's cov_x (float64 moments of the lag matrix, lambda on the bias entry too)
  within 1e-5 by _rel -- the bar for TRF weights --, and LagStats.ridge_solve on the same recording within 2e-5
  (each side within 1e-5 of exact); the lambdas: see the module's docstring."""
  c, pre, post, d, frames = shape
  fit, _, _, _, xe, xt = _whole(shape, 1.0)
  lambdas = _lambdas(frames)
  w, b = fit.solve(lambdas)
  k = fit.inputs
  assert w.is_cuda and tuple(w.shape) == (1, len(lambdas), k, d) and tuple(b.shape) == (1, len(lambdas), d)
  assert str(w.dtype) == 'torch.float32'
  stats = dev.LagStats(c, pre, post, d=d)
  stats.accumulate(xe, y=xt)
  sw, sb = stats.ridge_solve(lambdas)
  w, b, sw, sb = (t.cpu().numpy().astype(np.float64) for t in (w, b, sw, sb))
  xtx, xty = hof.reference_moments(c, pre, post, d, frames)
  for li, lam in enumerate(lambdas):
    want_w, want_b = hof.reference_solve(xtx, xty, frames, lam)
    got, want = np.vstack([w[0, li], b[0, li][None]]), np.vstack([want_w, want_b[None]])
    batch = np.vstack([sw[li], sb[li][None]])
    err, err_batch = hof.rel(got, want), hof.rel(got, batch)
    print('%s lambda %g: float64 %.3g, LagStats.ridge_solve %.3g' % (shape, lam, err, err_batch))
    parity_log.record('online_fit_solve_c%d_pre%d_post%d_d%d_lam%g' % (shape[:4] + (lam,)), float64=err,
                      lagstats=err_batch)
    assert err <= 1e-5
    assert err_batch <= 2e-5


def test_a_bank_is_its_sessions(dev):
  """Three sessions with different data against three single sessions, exactly: moments, tails, weights; the
  strides of a sliced bank."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, d, frames = 63, 1, 0, 1, 300
  for c, pre, post, d in ((63, 1, 0, 1), (5, 2, 9, 1), (16, 3, 0, 8)):
    recs = [hof.recording(c, d, frames, seed=s) for s in range(3)]
    # (wider and longer than the bank reads: neither stride is the packed one)
    eeg = torch.zeros((3, frames + 5, c + 3), device='cuda')
    target = torch.zeros((3, frames + 2, d + 1), device='cuda')
    for i, (e, t) in enumerate(recs):
      eeg[i, :frames, :c], target[i, :frames, :d] = _up(e), _up(t)
    eeg, target = eeg[:, :frames, :c], target[:, :frames, :d]
    bank = online.OnlineRidgeFit(c, pre, post, outputs=d, num_sessions=3, forgetting=0.99)
    hof.run(bank, eeg, target, [130, 1, 0, 169])
    a, b = bank.moments()
    w, bias = bank.solve([1.0, 10.0])
    tails = bank.tails
    for i in range(3):
      single = online.OnlineRidgeFit(c, pre, post, outputs=d, forgetting=0.99)
      hof.run(single, _up(recs[i][0]), _up(recs[i][1]), [frames])
      sa, sb = single.moments()
      sw, sbias = single.solve([1.0, 10.0])
      assert torch.equal(a[i], sa[0]) and torch.equal(b[i], sb[0]), (c, i)
      assert torch.equal(w[i], sw[0]) and torch.equal(bias[i], sbias[0]), (c, i)
      assert torch.equal(tails[0][i], single.tails[0][0]) and torch.equal(tails[1][i], single.tails[1][0])
    assert not torch.equal(a[0], a[1])


def test_one_launch_per_push_and_two_runs_give_the_same_bits(dev):
  """td_profile_read counts ONE launch for a push with rows (also one that emits nothing), none for an empty push,
  at most one for the flush; device tensors in, nothing comes to the host; two identical runs, the same bits."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, d, frames = 64, 0, 20, 1, 120
  eeg, target = hof.recording(c, d, frames)
  xe, xt = _up(eeg), _up(target)
  h = dev.default_handle()
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d)
  runs = []
  for attempt in range(2):
    fit.reset()
    h.profile_enable(True)
    h.profile_read()
    at = 0
    for n in (5, 0, 1, 37, 77):                              # (the first push emits nothing: 5 <= post)
      fit.push(xe[at:at + n], xt[at:at + n, 0])
      assert h.profile_read()[0] == (1 if n else 0), n
      at += n
    assert fit.frames == frames - post
    fit.flush()
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    a, b = fit.moments()
    w, bias = fit.solve([1.0])
    assert a.is_cuda and w.is_cuda
    runs.append([t.clone() for t in (a, b, w, bias) + tuple(fit.tails)])
  for first, second in zip(*runs):
    assert torch.equal(first, second)
  assert torch.equal(runs[0][0], _whole((c, pre, post, d, frames), 1.0)[1])


def _scores(dec, eeg, env, lo, hi):
  return dec.push(eeg[lo:hi], env[lo:hi, 0], env[lo:hi, 1]).scores[0]


def test_set_weights_on_the_device(dev):
  """Weights fitted online go into a running OnlineDecoder device to device: the scores after the swap are those of
  a fresh OnlineDecoder around the new weights that was pushed the same rows, byte for byte -- every window of one
  frame, and of the windows of 20 frames those that begin at or behind the swap --, the scores before it the old
  decoder's; a push is still one launch; a shared model copy becomes S copies."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post = 4, 2, 3
  rec = host_online.recipe(c, pre, post)
  eeg, env = _up(rec['eeg'][:600].astype(np.float32)), _up(rec['env'][:600].astype(np.float32))
  fit = online.OnlineRidgeFit(c, pre, post)
  fit.push(eeg[:300], env[:300, 0])
  w, b = fit.solve([0.1])
  w_new, b_new = w[:, 0, :, 0], b[:, 0, 0]                   # [1, K] and [1] device views
  assert w_new.is_cuda and b_new.is_cuda and w_new.data_ptr() == w.data_ptr()
  make = lambda wv, bv: host_online.linear_decoder(c, pre, post, wv, bv, rec['corr'][0], 'mean-squared')
  new_decoder = make(w_new[0].cpu().numpy(), float(b_new[0].cpu()))
  h = dev.default_handle()
  cut, end = 130, 600
  k = cut - post                                            # frames emitted before the swap
  for width, hop in ((1, 1), (20, 10)):
    dec = online.OnlineDecoder(make(rec['w'], rec['b']), width, hop)
    old = online.OnlineDecoder(make(rec['w'], rec['b']), width, hop)
    new = online.OnlineDecoder(new_decoder, width, hop)
    head = _scores(dec, eeg, env, 0, cut)
    dec.set_weights(w_new, b_new)
    h.profile_enable(True)
    h.profile_read()
    rest = _scores(dec, eeg, env, cut, end)
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    rest = np.concatenate([rest, dec.flush().scores[0]])
    np.testing.assert_array_equal(head, _scores(old, eeg, env, 0, cut))
    want = np.concatenate([_scores(new, eeg, env, 0, cut), _scores(new, eeg, env, cut, end), new.flush().scores[0]])
    got = np.concatenate([head, rest])
    assert got.shape == want.shape
    first = -(-k // hop)                                    # the first window that begins at or behind frame k
    assert 0 < first < got.shape[0] - 10
    assert got[first:].tobytes() == want[first:].tobytes(), (width, hop)
    assert got[:first].tobytes() != want[:first].tobytes()
  # a bank that shared one model copy: S rows make S copies, one row goes to every session
  bank = online.OnlineDecoder([make(rec['w'], rec['b'])] * 2, 1, 1)
  assert int(bank._dev['w'].shape[0]) == 1
  both = torch.stack([_up(np.reshape(rec['w'], -1).astype(np.float32)), w_new[0]])
  bank.set_weights(both, torch.stack([_up(np.float32(np.reshape(rec['b'], -1)[:1]))[0], b_new[0]]))
  assert tuple(bank._dev['w'].shape) == (2, (pre + 1 + post) * c) and tuple(bank._dev['b'].shape) == (2,)
  eeg2, env2 = torch.stack([eeg[:cut]] * 2), torch.stack([env[:cut]] * 2)
  got = bank.push(eeg2, env2[:, :, 0], env2[:, :, 1]).scores
  fresh_old, fresh_new = (online.OnlineDecoder(make(rec['w'], rec['b']), 1, 1), online.OnlineDecoder(new_decoder, 1, 1))
  assert got[0].tobytes() == _scores(fresh_old, eeg, env, 0, cut).tobytes()
  assert got[1].tobytes() == _scores(fresh_new, eeg, env, 0, cut).tobytes()
  bank.reset()
  bank.set_weights(w_new[0].cpu().numpy(), float(b_new[0].cpu()))        # (arrays go in too)
  got = bank.push(eeg2, env2[:, :, 0], env2[:, :, 1]).scores
  assert got[0].tobytes() == got[1].tobytes() == _scores(online.OnlineDecoder(new_decoder, 1, 1), eeg, env, 0,
                                                         cut).tobytes()


def test_a_singular_system_is_reported(dev):
  """All-zero EEG and lambda = 0: cov_x is zero but for the bias entry -- numpy.linalg.LinAlgError, as
  LagStats.ridge_solve reports it -- and the handle solves the next system; the refusals the device call makes."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post, d = 5, 2, 9, 1
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d, num_sessions=2)
  with pytest.raises(ValueError, match='no frame counted yet'):
    fit.solve([0.1])
  zeros = torch.zeros((2, 50, c), device='cuda')
  fit.push(zeros, torch.ones((2, 50), device='cuda'))
  with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
    fit.solve([0.0])
  w, b = fit.solve([0.5])                                   # (0 + 0.5) b = 1 / ... : cov_xy's bias entry is mean(y) = 1
  assert not bool(w.any()) and np.allclose(b.cpu().numpy(), 1.0 / 1.5, rtol=1e-6)
  state = fit._dev['state']
  before = state.clone()
  for kwargs, match in ((dict(forget=0.0), 'forgetting'), (dict(forget=1.5), 'forgetting'),
                        (dict(frames_before=-1), 'frames'), (dict(pre=40, post=40), 'lags')):
    args = dict(frames_before=50, pushes_before=1, pre=pre, post=post, forget=1.0)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
      dev.online_fit_push(zeros, torch.ones((2, 50, 1), device='cuda'), state, args['frames_before'],
                          args['pushes_before'], args['pre'], args['post'], forget=args['forget'])
  with pytest.raises(ValueError, match='state stride'):
    dev.online_fit_push(zeros[:1], torch.ones((1, 50, 1), device='cuda'), state[:1, :-8], 50, 1, pre, post)
  with pytest.raises(ValueError, match='systems'):
    dev.online_fit_solve(state, c, pre, post, d, 41, np.full(40000, 1.0))
  with pytest.raises(RuntimeError, match='no frame emitted'):
    dev.online_fit_solve(state, c, pre, post, d, 0, [1.0])
  assert torch.equal(state, before)
  # dense systems over the limit: 2 sessions x 70 lambdas x 2049^2 float64 = 4.7 GB, refused before anything is built
  big = online.OnlineRidgeFit(128, 0, 15, num_sessions=2)
  assert big.push(torch.ones((2, 16, 128), device='cuda'), torch.ones((2, 16), device='cuda')) == 1
  with pytest.raises(MemoryError, match='dense systems'):
    big.solve(np.full(70, 1.0))
  w, b = big.solve([1.0])                                   # (and the handle goes on: one frame of ones, lambda 1)
  assert tuple(w.shape) == (2, 1, 2048, 1) and bool(torch.isfinite(w).all())
