"""GPU sweep of the blocked float64 Cholesky (csrc/chol.hip), the ridge routes over it (csrc/solve.hip) and the
leave-one-out preconditioned-CG solver (csrc/loso.hip) at their edges, at the cases of tests/chol_edges.py: td_spd_solve against LAPACK and a numpy model of the kernel's own algebra
by the normwise backward error of each right-hand-side column; the ridge routes (ridge_solve on the factorisation,
ridge_solve_async, ridge_solve_multi, wide targets) and td_ridge_solve_loso / _terms against np.linalg.solve in float64
of the systems built from the device's own float64 moments, within the derived bounds of chol_edges (in effect one
float32 rounding of the output); exactly singular members, which must be reported, beside twins that must pass; and a
NaN member, which np.linalg.solve lets through."""
import ctypes

import numpy as np
import pytest

from tests import chol_edges as xe
from tests import parity_log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _spd_solve(dev, a, rhs):
  """td_spd_solve on copies of a [batch, n, n], rhs [batch, n, nrhs]; the matrix must come back bit-identical."""
  import torch
  h = dev.default_handle()
  batch, n, nrhs = rhs.shape
  ad = torch.from_numpy(np.array(a)).cuda()
  rd = torch.from_numpy(np.array(rhs)).cuda()
  try:
    h.check(h.lib.td_spd_solve(h.ptr, ctypes.c_void_p(ad.data_ptr()), ctypes.c_void_p(rd.data_ptr()), n, nrhs, batch))
  finally:
    back = ad.cpu().numpy()
    assert np.array_equal(back, a, equal_nan=True), 'td_spd_solve changed its matrix argument'
  return rd.cpu().numpy()


def _check_spd(name, a, rhs, x, ref, skip=()):
  eta, ratio = xe.spd_distance(a, rhs, x, ref, skip)
  print('%s: eta gpu %.3e  lapack %.3e  model %.3e  eta / bound %.3f  eta / cap %.2e' %
        (name, np.nanmax(eta), np.nanmax(ref.eta_lapack), np.nanmax(ref.eta_model), ratio, np.nanmax(eta) / ref.cap))
  parity_log.record('chol_edges ' + name, eta_gpu=float(np.nanmax(eta)), eta_lapack=float(np.nanmax(ref.eta_lapack)),
                    eta_model=float(np.nanmax(ref.eta_model)), distance_over_bound=ratio)
  keep = [m for m in range(len(a)) if m not in skip]
  assert np.all(np.isfinite(x[keep]))
  assert np.all(eta[keep] <= ref.bound[keep]), (ratio, eta)
  assert np.all(eta[keep] <= ref.cap), (eta, ref.cap)
  return ratio


@pytest.mark.parametrize('case', xe.SPD_CASES, ids=xe.spd_id)
def test_spd_solve_backward_error_against_lapack_and_model(dev, case):
  a, rhs = xe.spd_system(case)
  ref = xe.spd_reference(case)
  x = _spd_solve(dev, a, rhs)
  _check_spd(xe.spd_id(case), a, rhs, x, ref)


@pytest.mark.parametrize('case', xe.SINGULAR_CASES, ids=xe.singular_id)
def test_singular_member_is_reported_and_its_twin_passes(dev, case):
  """Row / column j an exact copy of row / column i in one member: TD_ERR_SINGULAR ("Singular matrix"), wherever the
  block of pivot j is factored and whichever member it is; the twin whose copy is perturbed to a safely positive
  pivot passes, every member inside its bound."""
  a, rhs = xe.singular_system(case, False)
  with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
    _spd_solve(dev, a, rhs)
  a, rhs = xe.singular_system(case, True)
  ref = xe.system_reference(a, rhs)
  x = _spd_solve(dev, a, rhs)
  _check_spd('twin ' + xe.singular_id(case), a, rhs, x, ref)


def test_nan_member_goes_through_like_numpy(dev):
  """np.linalg.solve returns NaN for a matrix that holds one and raises nothing: so does td_spd_solve (a NaN pivot is
  not "not positive"), and the other eight members of the batch are inside their bounds."""
  case = xe.NAN_CASE
  a, rhs = xe.nan_system()
  ref = xe.system_reference(a, rhs, skip=(case.member,))
  x = _spd_solve(dev, a, rhs)
  assert not np.any(np.isfinite(np.linalg.solve(a[case.member], rhs[case.member])))
  assert not np.any(np.isfinite(x[case.member]))
  _check_spd('nan member', a, rhs, x, ref, skip=(case.member,))


# ---- the float32 ridge routes ----------------------------------------------------------------------------------------
def _stats_of(dev, h, case, files):
  st = dev.LagStats(case.c, case.pre, case.post, d=case.d, handle=h)
  x = np.concatenate([f[0] for f in files])
  y = np.concatenate([f[1] for f in files])
  offs = np.concatenate(([0], np.cumsum([len(f[0]) for f in files])))
  st.accumulate(h.to_device(x), None, h.to_device(y), offs, handle=h)
  return st


def _device_moments(st):
  m = st.moments()
  frames, _ = st.counts()
  return m['xtx'].cpu().numpy(), m['xty'].cpu().numpy(), frames


def _check_ridge(name, w, b, ref, **more):
  dw, db, ratio = xe.loso_distance(w, b, ref)
  bw, bb = xe.loso_bounds(ref)
  print('%s: |w - ref| %.3e  |b - ref| %.3e  distance / bound %.3f  cond %.2f  E / rounding %.2e' %
        (name, dw, db, ratio, ref.cond.max(), xe.e_over_rounding(ref)))
  parity_log.record('chol_edges ' + name, w_vs_ref64=dw, b_vs_ref64=db, largest_bound=float(max(bw.max(), bb.max())),
                    distance_over_bound=ratio, cond=float(ref.cond.max()), **more)
  assert xe.e_over_rounding(ref) <= 1.0
  assert np.all(np.abs(w.astype(np.float64) - ref.w) <= bw), (dw, ratio)
  assert np.all(np.abs(b.astype(np.float64) - ref.b) <= bb), (db, ratio)


@pytest.mark.parametrize('case', xe.RIDGE_CASES, ids=xe.ridge_id)
def test_ridge_routes_against_float64(dev, case):
  h = dev.default_handle()
  lams = xe.lambdas(case.n_lambda)
  sts = [_stats_of(dev, h, case, xe.ridge_files(case, s)) for s in range(case.stats)]
  batch = case.n_lambda * (case.stats if case.d <= xe.MAX_RHS else 1)
  refs = [xe.ridge_reference(*_device_moments(st), lams, batch) for st in sts]
  ref = xe.ce.Reference(*(np.stack([getattr(r, f) for r in refs]) for f in xe.ce.Reference._fields))
  h.set_solver('cholesky')
  try:
    if case.route == 'solve':
      w, b = sts[0].ridge_solve(lams, handle=h)
      assert h.last_solve_info()['solver'] == 'cholesky', h.last_solve_info()
      w, b = w[None], b[None]
    elif case.route == 'async':
      w, b, flag = sts[0].ridge_solve_async(lams, handle=h)
      h.synchronize()
      assert flag() == 0
      w, b = w[None], b[None]
    else:
      w, b = dev.LagStats.ridge_solve_multi(sts, lams, handle=h)
  finally:
    h.set_solver('auto')
  w, b = w.cpu().numpy(), b.cpu().numpy()
  assert w.shape == ref.w.shape and b.shape == ref.b.shape
  _check_ridge(xe.ridge_id(case), w, b, ref)


@pytest.mark.parametrize('case', xe.LOSO_CASES, ids=xe.loso_id)
def test_loso_sweep_against_float64(dev, case):
  """td_ridge_solve_loso / td_ridge_solve_loso_terms: every (fold, lambda, output) against np.linalg.solve of the
  fold's own system, built from the moments of the fold's separately summed statistics; status converged in 1..40
  iterations.  The terms cases also ask for k_major, which must be the plain output permuted, bit for bit."""
  h = dev.default_handle()
  lams = xe.lambdas(case.n_lambda)
  files = xe.loso_files(case)
  stats = {g: _stats_of(dev, h, case, [f]) for g, f in enumerate(files)}
  if case.as_terms:
    x, y = files[-1]
    cut = dev.LagStats(case.c, case.pre, case.post, d=case.d, handle=h)
    cut.accumulate(h.to_device(x), None, h.to_device(y), [0, len(x)], rows_used=[len(x) - xe.TRUNCATED], handle=h)
    stats['cut'] = cut
  proto = stats[0]
  total = proto.like().combine([stats[g] for g in range(case.n_files)])
  # the folds' training statistics, summed separately (the reference of both calls; the input of the plain call)
  parts = xe.loso_fold_parts(case)
  if case.as_terms:
    nf = case.n_files
    kept = [[g for g in range(nf - 1) if g != f] + ['cut'] for f in range(nf - 1)] + [list(range(nf - 1)), list(range(nf))]
  else:
    kept = [[g for g, _ in p] for p in parts]
  sums = [proto.like().combine([stats[g] for g in names]) for names in kept]
  ref = xe.loso_reference([_device_moments(s) for s in sums], lams)
  plan = xe.loso_plan(xe.stat_n(case), case.d, len(sums), case.n_lambda)
  if case.as_terms:
    terms = [[(stats[g], sg) for g, sg in fold] for fold in xe.terms_folds(case.n_files)]
    out = dev.LagStats.ridge_solve_loso_terms(total, terms, lams, tol=xe.CG_TOL, handle=h)
  else:
    out = dev.LagStats.ridge_solve_loso(total, sums, lams, tol=xe.CG_TOL, handle=h)
  assert out is not None and dev.LagStats.last_loso_status == 'converged', dev.LagStats.last_loso_status
  w, b, iterations = out
  assert 1 <= iterations <= 40
  if case.as_terms:
    w_km, b_km, _ = dev.LagStats.ridge_solve_loso_terms(total, terms, lams, tol=xe.CG_TOL, handle=h, k_major=True)
    assert tuple(w_km.shape) == (len(terms), xe.stat_n(case) - 1, case.n_lambda * case.d)
    assert np.array_equal(w_km.cpu().numpy(), w.permute(0, 2, 1, 3).reshape(len(terms), -1, case.n_lambda * case.d).cpu().numpy())
    assert np.array_equal(b_km.cpu().numpy(), b.cpu().numpy())
  w, b = w.cpu().numpy(), b.cpu().numpy()
  assert w.shape == ref.w.shape and b.shape == ref.b.shape
  _check_ridge(xe.loso_id(case), w, b, ref, iterations=iterations, chunks=plan.chunks, matvec_chunks=plan.mv_chunks,
               nbig=plan.nbig, last_m=plan.ms[-1])
