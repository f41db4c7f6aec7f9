"""The online CCA fit on the GPU (td_ccafit_online_push / _moments / _solve, online.OnlineCCAFit,
OnlineDecoder.set_cca_model): two-view recordings driven by coloured sources (tests/host_online_cca_fit.py) at the
shapes where the two-view staging and the tiling can go wrong -- the state, the tails and the moments bit for bit
against the NumPy session with and without forgetting, every cut byte for byte through both tail copies, a bank
against its sessions, one launch per push, repeatability, the moments against float64 lag matrices, the solve
isolated against the dense stage through LAPACK on the device's own moments, the CCA invariants of the returned
float32 rotations, the closed-form statistics against two passes, the batch route end to end, set_cca_model device to
device, and the device call's refusals."""
import numpy as np
import pytest

from tests import host_online_cca as hcc
from tests import host_online_cca_fit as hc
from tests import parity_log

pytestmark = pytest.mark.gpu

IDS = [hc.shape_id(s) for s in hc.SHAPES]
# the two large shapes run once each with g = 1, plus one g = 0.99 push test
PUSH_CASES = [(s, g) for s in hc.SMALL for g in hc.FORGETS] + [(s, 1.0) for s in hc.LARGE] + [(hc.LARGE[0], 0.99)]
PUSH_IDS = ['%s_g%g' % (hc.shape_id(s), g) for s, g in PUSH_CASES]
SOLVE_CASES = [(s, 1.0) for s in hc.SHAPES] + [(hc.SMALL[0], 0.99)]
SOLVE_IDS = ['%s_g%g' % (hc.shape_id(s), g) for s, g in SOLVE_CASES]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  assert device.gpu_available()
  return device


def _up(a):
  import torch
  return torch.from_numpy(np.array(a, order='C')).to('cuda')       # (a copy: the shared recordings are read-only)


def _np(t):
  return t.cpu().numpy()


_WHOLE = {}
_SOLVED = {}


def _whole(shape, forget):
  """(the fit after the whole recording in one push and an empty flush, its moments, its tails, the device
  recording): once per (shape, g), read-only."""
  key = (shape, forget)
  if key not in _WHOLE:
    eeg, feat = hc.shape_recording(shape)
    xe, xf = _up(eeg), _up(feat)
    fit = hc.make_fit(shape, forgetting=forget)
    hc.run(fit, xe, xf, [shape[6]])
    _WHOLE[key] = (fit, [m.clone() for m in fit.moments()], [t.clone() for t in fit.tails], xe, xf)
  return _WHOLE[key]


def _solved(shape, forget):
  """(result as host arrays, info, the four moment pieces as host float64, lambdas): once per (shape, g)."""
  key = (shape, forget)
  if key not in _SOLVED:
    fit, pieces = _whole(shape, forget)[:2]
    lambdas = hc.lambdas_of(shape)
    r, info = fit.solve(lambdas, hc.dim_of(shape), want_info=True)
    assert all(t.is_cuda for t in r) and str(r.rot_x.dtype) == 'torch.float32' and str(r.corr.dtype) == 'torch.float64'
    _SOLVED[key] = (type(r)(*(_np(t) for t in r)), info, [_np(p[0]) for p in pieces], lambdas)
  return _SOLVED[key]


def _state_square(fit, session=0):
  """The n x n float64 square at the head of a session's state block, as stored."""
  n = fit.inputs + fit.inputs2 + 1
  import torch
  return _np(fit._dev['state'][session, :8 * n * n].view(torch.float64).reshape(n, n))


def _check_against_host(fit, host, what):
  """State square (upper tiles the host's M, lower tiles zero), tails and the four dense pieces: exact."""
  n = fit.inputs + fit.inputs2 + 1
  square = _state_square(fit)
  tile = np.arange(n) // 64
  upper = tile[:, None] <= tile[None, :]
  assert np.array_equal(square[upper], host.m[upper]), what
  assert not square[~upper].any(), what
  tails = fit.tails
  assert np.array_equal(_np(tails[0][0]), host.tail) and np.array_equal(_np(tails[1][0]), host.feat_tail), what
  for got, want in zip(fit.moments(), host.moments()):
    assert np.array_equal(_np(got[0]), want), what


@pytest.mark.parametrize('shape,forget', PUSH_CASES, ids=PUSH_IDS)
def test_state_tails_and_moments_are_the_numpy_sessions_bits(dev, shape, forget):
  """np.array_equal with online._HostCCAFitSession -- M * g + np.outer(u, u) per frame in frame order -- after
  EVERY push and after the flush: the state's square (lower tiles zero), both tails, the four pieces of moments();
  M symmetric, M[n - 1][n - 1] the (effective) count; the whole recording in one push gives the same bits."""
  import torch
  from telluride_decoding_amd import online
  eeg, feat = hc.shape_recording(shape)
  frames = shape[6]
  k1, k2, n, delay = hc.sizes(shape)
  fit = hc.make_fit(shape, forgetting=forget)
  host = online._HostCCAFitSession(*shape[:6], forget)
  pushes = hc.LARGE_PUSHES if shape in hc.LARGE else (frames // 3, 1, frames - frames // 3 - 1)
  assert sum(pushes) == frames
  xe, xf = _up(eeg), _up(feat)
  at = 0
  for size in pushes:
    fit.push(xe[at:at + size], xf[at:at + size])
    host.push(eeg[at:at + size], feat[at:at + size], at, False)
    at += size
    _check_against_host(fit, host, at)
  fit.flush()
  host.push(eeg[:0], feat[:0], at, True)
  _check_against_host(fit, host, 'flush')
  xtx = _np(fit.moments()[0][0])
  assert xtx.dtype == np.float64 and np.array_equal(xtx, xtx.T) and np.array_equal(host.m, host.m.T)
  if forget == 1.0:
    assert xtx[k1, k1] == frames
  whole = _whole(shape, forget)
  for got, want in zip(fit.moments(), whole[1]):
    assert torch.equal(got, want)


@pytest.mark.parametrize('forget', hc.FORGETS)
@pytest.mark.parametrize('shape', hc.SMALL, ids=IDS[:5])
def test_any_cut_of_the_recording_gives_the_same_bits(dev, shape, forget):
  """Pushes of 1 (the first `delay` of them emit nothing), one row short of EACH view's tail, of 7, random 0 .. 40 with
  empty pushes, whole, and an empty push in the middle; flushed by a flushing last push and by an empty flushing
  push; the cuts reach the last frame after an odd and after an even number of pushes with rows, so both tail copies
  end up live: moments and tails byte for byte."""
  import torch
  _, want, want_tails, xe, xf = _whole(shape, forget)
  fit = hc.make_fit(shape, forgetting=forget)
  parities = set()
  for name, sizes in hc.cuts(shape).items():
    for flush_last in (False, True):
      hc.run(fit, xe, xf, sizes, flush_last=flush_last)
      parities.add(fit._pushes & 1)
      for got, ref in zip(fit.moments(), want):
        assert torch.equal(got, ref), (name, flush_last)
      for got, ref in zip(fit.tails, want_tails):
        assert torch.equal(got, ref), (name, flush_last)
  assert parities == {0, 1}


def test_a_bank_is_its_sessions(dev):
  """Three sessions with different data against three single sessions, exactly: moments, tails, the model; the
  strides of a sliced bank (wider and longer than the bank reads: neither stride is the packed one)."""
  import torch
  for shape in (hc.SMALL[0], hc.SMALL[2], hc.SMALL[4]):
    c1, c2, frames = shape[0], shape[3], shape[6]
    dim = hc.dim_of(shape)
    recs = [hc.shape_recording(shape, seed=s) for s in range(3)]
    eeg = torch.zeros((3, frames + 5, c1 + 3), device='cuda')
    feat = torch.zeros((3, frames + 2, c2 + 1), device='cuda')
    for i, (e, f) in enumerate(recs):
      eeg[i, :frames, :c1], feat[i, :frames, :c2] = _up(e), _up(f)
    eeg, feat = eeg[:, :frames, :c1], feat[:, :frames, :c2]
    bank = hc.make_fit(shape, num_sessions=3, forgetting=0.99)
    hc.run(bank, eeg, feat, [130, 1, 0, frames - 131])
    pieces, tails = bank.moments(), bank.tails
    r = bank.solve([1.0], dim)
    for i in range(3):
      single = hc.make_fit(shape, forgetting=0.99)
      hc.run(single, _up(recs[i][0]), _up(recs[i][1]), [frames])
      for got, want in zip(pieces, single.moments()):
        assert torch.equal(got[i], want[0]), (shape, i)
      for got, want in zip(tails, single.tails):
        assert torch.equal(got[i], want[0]), (shape, i)
      for got, want in zip(r, single.solve([1.0], dim)):
        assert torch.equal(got[i], want[0]), (shape, i)
    assert not torch.equal(pieces[0][0], pieces[0][1])
    # ... and a state whose blocks lie further apart than they are long (the device call, its stride in bytes)
    nbytes = dev.online_ccafit_state_bytes(*shape[:6])
    padded = torch.zeros((3, nbytes + 64), dtype=torch.uint8, device='cuda')[:, :nbytes + 8]
    views = shape[1:3] + shape[4:6]
    dev.online_ccafit_push(eeg[:, :200], feat[:, :200], padded, 0, 0, *views, forget=0.99)
    dev.online_ccafit_push(eeg[:, 200:], feat[:, 200:], padded, 200, 1, *views, flush=True, forget=0.99)
    for got, want in zip(dev.online_ccafit_moments(padded, *shape[:6]), pieces):
      assert torch.equal(got, want), shape
    assert not bool(padded[:, nbytes:].any())


def test_one_launch_per_push_and_two_runs_give_the_same_bits(dev):
  """td_profile_read counts ONE launch for a push with rows (also one that emits nothing), none for an empty push,
  one for the flush; device tensors in, nothing comes to the host; two identical runs, the same bits."""
  import torch
  shape = hc.LARGE[0]
  frames, delay = shape[6], hc.sizes(shape)[3]
  eeg, feat = hc.shape_recording(shape)
  xe, xf = _up(eeg), _up(feat)
  h = dev.default_handle()
  fit = hc.make_fit(shape)
  runs = []
  for attempt in range(2):
    fit.reset()
    h.profile_enable(True)
    h.profile_read()
    at = 0
    for size in (5, 0, 1, 37, 77):                           # (the first push emits nothing: 5 <= delay)
      fit.push(xe[at:at + size], xf[at:at + size])
      assert h.profile_read()[0] == (1 if size else 0), size
      at += size
    assert fit.frames == frames - delay
    fit.flush()
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    r = fit.solve([1.0], 3)
    runs.append([t.clone() for t in tuple(fit.moments()) + tuple(r) + tuple(fit.tails)])
  for first, second in zip(*runs):
    assert first.is_cuda and torch.equal(first, second)
  assert torch.equal(runs[0][0], _whole(shape, 1.0)[1][0])


@pytest.mark.parametrize('shape', hc.SHAPES, ids=IDS)
def test_moments_against_float64_lag_matrices(dev, shape):
  """The four pieces against U^T U of U = [lag_matrix(x) | lag_matrix(y) | 1] in float64: 1e-14 of the largest
  element (a sum of up to 600 exact products rounded once each)."""
  k1, k2 = hc.sizes(shape)[:2]
  pieces = [_np(p[0]) for p in _whole(shape, 1.0)[1]]
  errs = [hc.rel(got, want) for got, want in zip(pieces, hc.split_moments(hc.reference_moments(shape), k1, k2))]
  print('%s: xtx %.3g x2tx2 %.3g xtx2 %.3g sum2 %.3g' % ((hc.shape_id(shape),) + tuple(errs)))
  parity_log.record('online_ccafit_moments_' + hc.shape_id(shape), xtx=errs[0], x2tx2=errs[1], xtx2=errs[2],
                    sum2=errs[3])
  assert max(errs) <= 1e-14


@pytest.mark.parametrize('shape,forget', SOLVE_CASES, ids=SOLVE_IDS)
def test_solve_matches_float64_lapack_on_the_devices_own_moments(dev, shape, forget):
  """td_ccafit_online_solve isolated as tests/test_gpu_cca_solve.py::test_cca_solve_matches_float64_lapack isolates
  td_cca_solve: covariances from the device's own moments(), the dense stage through LAPACK (eigh / svd, float64),
  with that test's tolerances -- e rtol 2e-6 / atol 1e-7; the rotations, jointly sign-aligned, within 2e-6 /
  max(gap, 1e-3) of the largest element; the means 1e-6 -- and the gap floors that keep the tolerance from going
  vacuous.  info: the one-launch route for k1 <= 64, k2 <= 16, the eigen route on the 2049 shape (k2 = 256)."""
  r, info, pieces, lambdas = _solved(shape, forget)
  k1, k2 = hc.sizes(shape)[:2]
  dim = hc.dim_of(shape)
  assert r.rot_x.shape == (1, len(lambdas), k1, dim) and r.rot_y.shape == (1, len(lambdas), k2, dim)
  assert r.e.shape == (1, len(lambdas), dim) and r.corr.shape == (1, len(lambdas), 3, dim)
  for li, lam in enumerate(lambdas):
    cxx, cyy, cxy, mx, my = hc.covariances(*pieces, lam)
    wa, wb, we = hc.dense_stage(cxx, cyy, cxy, dim)
    gap = hc.gap_of(we)
    if forget == 1.0:
      assert gap >= hc.GAP_FLOOR[shape], gap
    assert gap >= 1e-3
    a, b = hc.aligned(r.rot_x[0, li].astype(np.float64), r.rot_y[0, li].astype(np.float64), wa, wb)
    tol = 2e-6 / max(gap, 1e-3)
    print('%s g %g lambda %g: e %.3g, rot_x %.3g rot_y %.3g (tol %.3g, gap %.3g), info %s' % (
        hc.shape_id(shape), forget, lam, np.max(np.abs(r.e[0, li] - we) / we), hc.rel(a, wa), hc.rel(b, wb), tol, gap,
        info[0, li]))
    parity_log.record('online_ccafit_solve_%s_g%g_lam%g' % (hc.shape_id(shape), forget, lam),
                      e=float(np.max(np.abs(r.e[0, li] - we) / we)), rot_x=hc.rel(a, wa), rot_y=hc.rel(b, wb), gap=gap)
    np.testing.assert_allclose(r.e[0, li], we, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(a, wa, atol=tol * np.max(np.abs(wa)))
    np.testing.assert_allclose(b, wb, atol=tol * np.max(np.abs(wb)))
    np.testing.assert_allclose(r.mean_x[0], mx, atol=1e-6)
    np.testing.assert_allclose(r.mean_y[0], my, atol=1e-6)
    if k1 <= 64 and k2 <= 16 and k2 <= k1:
      assert info[0, li, 3] & 4, 'the one-launch dense stage was not taken'
    if shape == hc.LARGE[1]:
      assert not info[0, li, 3] & 1 and info[0, li, 0] > 0, 'the eigen route was not taken'


@pytest.mark.parametrize('shape,forget', SOLVE_CASES, ids=SOLVE_IDS)
def test_the_returned_rotations_keep_the_cca_invariants(dev, shape, forget):
  """The float32 rotations against float64 covariances from the device moments: |Rx^T Cxx Rx - I|, |Ry^T Cyy Ry - I|
  and |Rx^T Cxy Ry - diag(e)| <= 2e-6 (the project's e tolerance; the float64 oracle's rotations rounded to float32
  leave <= 9e-8)."""
  r, _, pieces, lambdas = _solved(shape, forget)
  dim = hc.dim_of(shape)
  for li, lam in enumerate(lambdas):
    cxx, cyy, cxy, _, _ = hc.covariances(*pieces, lam)
    rx, ry = r.rot_x[0, li].astype(np.float64), r.rot_y[0, li].astype(np.float64)
    res = (np.max(np.abs(rx.T @ cxx @ rx - np.eye(dim))), np.max(np.abs(ry.T @ cyy @ ry - np.eye(dim))),
           np.max(np.abs(rx.T @ cxy @ ry - np.diag(r.e[0, li].astype(np.float64)))))
    print('%s g %g lambda %g: residuals %.3g %.3g %.3g' % ((hc.shape_id(shape), forget, lam) + res))
    parity_log.record('online_ccafit_invariants_%s_g%g_lam%g' % (hc.shape_id(shape), forget, lam), xx=res[0],
                      yy=res[1], xy=res[2])
    assert max(res) <= 2e-6


@pytest.mark.parametrize('shape,forget', SOLVE_CASES, ids=SOLVE_IDS)
def test_corr_is_the_two_pass_statistics_of_the_returned_model(dev, shape, forget):
  """corr against the two-pass float64 mean and centred power of (X - mean_x) rot_x and (Y - mean_y) rot_y, computed
  on the host from the returned float32 model: 1e-10 relative for power, 1e-12 absolute for the means."""
  r, _, _, lambdas = _solved(shape, forget)
  _, x, y = hc.joint(shape)
  weights = forget ** np.arange(shape[6] - 1, -1, -1.0)
  for li, lam in enumerate(lambdas):
    want = hc.two_pass_statistics(x, y, r.mean_x[0], r.rot_x[0, li], r.mean_y[0], r.rot_y[0, li], weights)
    got = r.corr[0, li]
    err_p, err_m = float(np.max(np.abs(got[2] - want[2]) / want[2])), float(np.max(np.abs(got[:2] - want[:2])))
    print('%s g %g lambda %g: power %.3g relative, means %.3g' % (hc.shape_id(shape), forget, lam, err_p, err_m))
    parity_log.record('online_ccafit_corr_%s_g%g_lam%g' % (hc.shape_id(shape), forget, lam), power=err_p, means=err_m)
    assert err_p <= 1e-10
    assert err_m <= 1e-12


def test_against_the_batch_route_end_to_end(dev):
  """(64, 0, 20 | 8, 0, 15), 600 frames, lambda 1: LagStats.accumulate of the whole recording as one file +
  cca_solve(frames - 1, ...) -- what BrainModelCCA.fit runs.  e rtol 3e-6; rotations 1e-5 of the largest element over
  max(gap, 1e-3) (test_cca_solve_lagged_golden_all_components' bars with the lapack test's gap scaling)."""
  c1, pre1, post1, c2, pre2, post2 = hc.LARGE[0][:6]
  frames, dim, lam = 600, 3, 1.0
  eeg, feat = hc.recording(c1, c2, frames)
  xe, xf = _up(eeg), _up(feat)
  fit = hc.make_fit(hc.LARGE[0])
  fit.push(xe[:250], xf[:250])
  fit.flush(xe[250:], xf[250:])
  r = fit.solve([lam], dim)
  st = dev.LagStats(c1, pre1, post1, c2, pre2, post2)
  st.accumulate(xe, xf, None, [0, frames])
  ra, rb, mx, my, e, _ = st.cca_solve(frames - 1, lam, dim)
  e_on, e_batch = _np(r.e[0, 0]).astype(np.float64), _np(e).astype(np.float64)
  gap = hc.gap_of(e_batch)
  a, b = hc.aligned(_np(r.rot_x[0, 0]).astype(np.float64), _np(r.rot_y[0, 0]).astype(np.float64),
                    _np(ra).astype(np.float64), _np(rb).astype(np.float64))
  err_e = float(np.max(np.abs(e_on - e_batch) / e_batch))
  err_a, err_b = hc.rel(a, _np(ra)), hc.rel(b, _np(rb))
  tol = 1e-5 / max(gap, 1e-3)
  print('batch route: e %.3g, rot_x %.3g rot_y %.3g (tol %.3g, gap %.3g)' % (err_e, err_a, err_b, tol, gap))
  parity_log.record('online_ccafit_vs_batch', e=err_e, rot_x=err_a, rot_y=err_b, gap=gap)
  np.testing.assert_allclose(e_on, e_batch, rtol=3e-6)
  assert err_a <= tol and err_b <= tol
  np.testing.assert_allclose(_np(r.mean_x), _np(mx), atol=1e-6)
  np.testing.assert_allclose(_np(r.mean_y), _np(my), atol=1e-6)


def _scores(dec, eeg, feats, lo, hi):
  return dec.push(eeg[lo:hi], feats[0][lo:hi], feats[1][lo:hi])


def test_set_cca_model_on_the_device(dev):
  """A model fitted online goes into a running CCA OnlineDecoder device to device, with reduction 'mean' and with
  'lda' keeping its LDA: scores and decisions from the first window wholly behind the swap are byte for byte those of
  a fresh OnlineDecoder built from update_model's model and the same corr; the scores before it are the old
  decoder's; one launch per push before and after the swap; S models into a bank that shared one copy."""
  import torch
  from telluride_decoding_amd import brain_model, cca, online
  shape = hc.SMALL[0]
  view1, view2 = shape[:3], shape[3:6]
  k1, k2, n, delay = hc.sizes(shape)
  dims = 3
  eeg_h = hc.shape_recording(shape)[0]
  feat_h = (hc.shape_recording(shape)[1], hc.shape_recording(shape, seed=1)[1])
  eeg, feats = _up(eeg_h), [_up(f) for f in feat_h]
  models = []
  for cut_fit in (200, 400):
    fit = hc.make_fit(shape)
    fit.push(eeg[:cut_fit], feats[0][:cut_fit])
    r = fit.solve([1.0], dims)
    model = fit.update_model(cca.BrainModelCCA(brain_model._shape_dataset(k1, k2, 1), cca_dims=dims), 1.0, dims)
    assert np.array_equal(model.rot_x, _np(r.rot_x[0, 0])) and np.array_equal(model.mean_y[0], _np(r.mean_y[0]))
    models.append((r, model))
  (r_old, m_old), (r_new, m_new) = models
  lda = np.concatenate([np.arange(1.0, dims + 1.0), [-0.8, 0.25]])
  h = dev.default_handle()
  cut, end = 130, 600
  k = cut - delay                                           # frames emitted before the swap
  for reduction, width, hop in (('mean', 1, 1), ('mean', 20, 10), ('lda', 20, 10)):
    use = lda if reduction == 'lda' else None
    make = lambda r, m: hcc.cca_decoder(view1, view2, m.mean_x, m.rot_x, m.mean_y, m.rot_y, _np(r.corr[0, 0]),
                                        reduction, use)
    dec, old = (online.OnlineDecoder(make(r_old, m_old), width, hop) for _ in range(2))
    new = online.OnlineDecoder(make(r_new, m_new), width, hop)
    h.profile_enable(True)
    h.profile_read()
    head = _scores(dec, eeg, feats, 0, cut)
    assert h.profile_read()[0] == 1
    dec.set_cca_model(r_new.mean_x[0], r_new.rot_x[0, 0], r_new.mean_y[0], r_new.rot_y[0, 0], corr=r_new.corr[0, 0])
    rest = _scores(dec, eeg, feats, cut, end)
    assert h.profile_read()[0] == 1
    h.profile_enable(False)
    last = dec.flush()
    want_head = _scores(old, eeg, feats, 0, cut)
    assert head.scores.tobytes() == want_head.scores.tobytes()
    assert head.decisions.tobytes() == want_head.decisions.tobytes()
    wants = [_scores(new, eeg, feats, 0, cut), _scores(new, eeg, feats, cut, end), new.flush()]
    got_s = np.concatenate([head.scores[0], rest.scores[0], last.scores[0]])
    want_s = np.concatenate([w.scores[0] for w in wants])
    got_d = np.concatenate([head.decisions[0], rest.decisions[0], last.decisions[0]])
    want_d = np.concatenate([w.decisions[0] for w in wants])
    first = -(-k // hop)                                    # the first window that begins at or behind frame k
    assert got_s.shape == want_s.shape and 0 < first < got_s.shape[0] - 10
    assert got_s[first:].tobytes() == want_s[first:].tobytes(), (reduction, width, hop)
    assert got_d[first:].tobytes() == want_d[first:].tobytes(), (reduction, width, hop)
    assert got_s[:first].tobytes() != want_s[:first].tobytes()
  # a bank that shared one model copy: S models make S copies, one model goes to every session
  make = lambda r, m: hcc.cca_decoder(view1, view2, m.mean_x, m.rot_x, m.mean_y, m.rot_y, _np(r.corr[0, 0]), 'mean')
  bank = online.OnlineDecoder([make(r_old, m_old)] * 2, 1, 1)
  assert int(bank._dev['rot_x'].shape[0]) == 1
  both = lambda name, pick: torch.stack([pick(getattr(r_old, name)), pick(getattr(r_new, name))])
  bank.set_cca_model(both('mean_x', lambda t: t[0]), both('rot_x', lambda t: t[0, 0]), both('mean_y', lambda t: t[0]),
                     both('rot_y', lambda t: t[0, 0]), corr=both('corr', lambda t: t[0, 0]))
  assert tuple(bank._dev['rot_x'].shape) == (2, k1, dims) and tuple(bank._dev['mean_y'].shape) == (2, k2)
  eeg2 = torch.stack([eeg[:cut]] * 2)
  feats2 = [torch.stack([f[:cut]] * 2) for f in feats]
  got = bank.push(eeg2, feats2[0], feats2[1]).scores
  fresh = [_scores(online.OnlineDecoder(make(r, m), 1, 1), eeg, feats, 0, cut).scores[0] for r, m in models]
  assert got[0].tobytes() == fresh[0].tobytes() and got[1].tobytes() == fresh[1].tobytes()
  bank.reset()
  bank.set_cca_model(m_new.mean_x[0], m_new.rot_x, m_new.mean_y[0], m_new.rot_y, corr=_np(r_new.corr[0, 0]))  # arrays too
  got = bank.push(eeg2, feats2[0], feats2[1]).scores
  assert got[0].tobytes() == got[1].tobytes() == fresh[1].tobytes()


def test_the_device_calls_refusals_leave_the_state_untouched(dev):
  """Every limit refused by name by td_ccafit_online_push / _solve with the state untouched; solve before 2 counted
  frames: ValueError from OnlineCCAFit, TD_ERR_STATE from the device call, and the next valid solve is served."""
  import torch
  shape = hc.SMALL[0]
  c1, pre1, post1, c2, pre2, post2 = shape[:6]
  fit = hc.make_fit(shape, num_sessions=2)
  with pytest.raises(ValueError, match='0 frames counted'):
    fit.solve([0.1], 3)
  eeg, feat = hc.shape_recording(shape)
  xe, xf = torch.stack([_up(eeg[:50])] * 2), torch.stack([_up(feat[:50])] * 2)
  fit.push(xe[:, :10], xf[:, :10])                          # 10 rows, 9 behind: one frame
  state = fit._dev['state']
  before = state.clone()
  with pytest.raises(ValueError, match='1 frames counted'):
    fit.solve([0.1], 3)
  views = (c1, pre1, post1, c2, pre2, post2)
  with pytest.raises(RuntimeError, match='frames counted'):
    dev.online_ccafit_solve(state, *views, 1, [1.0], 3)
  push = lambda **kw: dev.online_ccafit_push(
      kw.get('eeg', xe[:, 10:]), kw.get('feat', xf[:, 10:]), kw.get('state', state), kw.get('frames_before', 10),
      kw.get('pushes_before', 1), kw.get('pre1', pre1), kw.get('post1', post1), kw.get('pre2', pre2),
      kw.get('post2', post2), forget=kw.get('forget', 1.0))
  for kwargs, match in ((dict(forget=0.0), 'forgetting'), (dict(forget=1.5), 'forgetting'),
                        (dict(frames_before=-1), 'frames'), (dict(pushes_before=-1), 'pushes'),
                        (dict(pre1=40, post1=40), 'lags'), (dict(pre2=40, post2=40), 'lags'),
                        (dict(eeg=xe[:1, 10:], feat=xf[:1, 10:], state=state[:1, :-8]), 'state stride')):
    with pytest.raises(ValueError, match=match):
      push(**kwargs)
  wide = torch.zeros((2, 5, 129), device='cuda')
  with pytest.raises(ValueError, match='129 channels'):
    push(eeg=wide, feat=xf[:, :5])
  with pytest.raises(ValueError, match='33 features'):
    push(eeg=xe[:, :5], feat=torch.zeros((2, 5, 33), device='cuda'))
  for kwargs, match in ((dict(dim=0), 'dim must be'), (dict(dim=17), 'dim must be'), (dict(lambdas=[-1.0]), 'lambda'),
                        (dict(lambdas=[]), 'lambdas')):
    with pytest.raises(ValueError, match=match):
      dev.online_ccafit_solve(state, *views, 41, kwargs.get('lambdas', [1.0]), kwargs.get('dim', 3))
  assert torch.equal(state, before)
  fit.push(xe[:, 10:], xf[:, 10:])                          # ... and the fit goes on: 41 frames counted
  r = fit.solve([1.0], 3)
  assert tuple(r.rot_x.shape) == (2, 1, hc.sizes(shape)[0], 3) and bool(torch.isfinite(r.rot_x).all())
  assert bool(torch.isfinite(r.corr).all()) and bool((r.corr[:, 0, 2] > 0).all())
