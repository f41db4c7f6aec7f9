"""GPU sweep of csrc/eig.hip at the cases of tests/eig_edges.py: td_sym_eigh on both routes, td_jacobi_svd on its
three, td_cca_solve as one launch and as the chain -- each against the float64 (and, for relative accuracy,
longdouble) references of that module within its derived bounds, the route asserted from what the call reports against
the restated route arithmetic.  The CCA references are built from the device's own float64 moments, so that only
eig.hip is on trial.  tests/test_cpu_eig_edges.py holds the models, the tables and the wrong kernels to the same bounds
without a GPU.

Measured on an MI355X, the worst case of every bound as gpu / model / LAPACK -> bound (the parity log has every case):
  sym_eigh   residual 5.2e-16 / 2.3e-16 / 3.5e-16 -> 2.8e-15 (indefinite_3); orthogonality 5.7e-14 / 3.4e-14 / 6.8e-15
             -> 2.7e-13 (rank_deficient_33); spectrum 2.8e-15 / 2.2e-15 / 7.3e-17 -> 1.7e-14 (graded_17); relative
             accuracy against the longdouble Jacobi 1.4e-11 / 7.1e-12 -> 5.7e-11 (graded_17): no quantity above a
             quarter of its bound
  jacobi_svd s 8.1e-13 / 1.5e-13 -> 1.2e-12 (cut_below_k64_m256, the rounds on singular values 1e-6 apart in size);
             vectors 5.3e-10 / 7.8e-9 -> 1.2e-7 (cut_above_k8_m866, the Gram route; the gap term alone); T v = s u
             1.5e-14 / 1.5e-14 -> 2.3e-13; the tied pair's projector 8.2e-15 -> 1.5e-12 (tie_k16_m64, the tied places'
             gap term); null places 6.2e-17 s_1 -> 5.7e-14 s_1
  cca_solve  e 2.4e-8 (0.89 of its bound, reg_27x7), rotations 5.3e-8 of the column's largest entry (0.98 of the bound,
             zero_64x16 through the chain); D_e <= 1.5e-14, D_rot <= 1.2e-9 (the uncorrelated kind), g >= 2.5e-3; both
             invariants <= 8.1e-8; every mean bit for bit.  As in tests/test_gpu_cca_sweep_edges.py, what is measured is the
             float32 rounding of the outputs, which is also all the room the bound leaves.
A rank deficient matrix on the block route reports 41 sweeps, on the GPU as in the model: the null space's entries are
rounding noise that the relative threshold never lets rest, so the outer loop runs out (the answers are inside every
bound; the cost is time)."""
import numpy as np
import pytest

from tests import cca_sweep_edges as cs
from tests import eig_edges as ee
from tests import parity_log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _eigh(dev, a):
  h = dev.default_handle()
  vals, vecs, sweeps = dev.sym_eigh(h.to_device(np.array(a), np.float64))
  return vals.cpu().numpy(), vecs.cpu().numpy(), sweeps


@pytest.mark.parametrize('case', ee.EIG_CASES, ids=ee.eig_id)
def test_sym_eigh(dev, case):
  """Residual, orthogonality and spectrum within 8 max(LAPACK, model, n 2^-53); an already diagonal matrix comes back
  exactly, after no sweep (direct) or one (block); a power-of-two scaling changes no sweep count; the small eigenvalues
  of the graded matrix keep their relative accuracy."""
  a = ee.eig_matrix(case)
  vals, vecs, sweeps = _eigh(dev, a)
  got, bound = ee.eig_measure(a, vals, vecs), ee.eig_bounds(case)
  lap, mod, model = ee.eig_reference(case)
  block = case.n > ee.NB
  print('%s sweeps %d (model %d) | residual gpu %.3g model %.3g lapack %.3g bound %.3g | orthogonality %.3g %.3g %.3g '
        '%.3g | spectrum %.3g %.3g bound %.3g' % (
            ee.eig_id(case), sweeps, model.sweeps, got.residual, mod.residual, lap.residual, bound.residual,
            got.orthogonality, mod.orthogonality, lap.orthogonality, bound.orthogonality, got.spectrum, mod.spectrum,
            bound.spectrum))
  parity_log.record('eig_edges sym_eigh ' + ee.eig_id(case), sweeps=sweeps, residual=got.residual,
                    residual_model=mod.residual, residual_lapack=lap.residual, residual_bound=bound.residual,
                    orth=got.orthogonality, orth_model=mod.orthogonality, orth_lapack=lap.orthogonality,
                    orth_bound=bound.orthogonality, spectrum=got.spectrum, spectrum_model=mod.spectrum,
                    spectrum_bound=bound.spectrum)
  assert got.residual <= bound.residual and got.orthogonality <= bound.orthogonality
  assert got.spectrum <= bound.spectrum
  assert (sweeps >= 1) if block else (sweeps == 0)           # (the route: the direct solver reports no outer sweep)
  if case.kind in ee.DIAGONAL_KINDS:
    assert np.array_equal(vecs, np.eye(case.n)) and np.array_equal(vals, np.diag(a))
    assert sweeps == (1 if block else 0)
  if case.kind in ee.SCALED_KINDS and block:
    assert sweeps == _eigh(dev, ee.eig_matrix(ee.EigCase(case.n, 'pd')))[2]
  if case.kind == 'graded':
    ref = ee.graded_reference(case.n)
    rel, rel_model = ee.relative_error(vals, ref), ee.relative_error(model.vals, ref)
    print('  relative accuracy: gpu %.3g model %.3g bound %.3g' % (rel, rel_model, 8.0 * rel_model))
    parity_log.record('eig_edges graded ' + ee.eig_id(case), relative=rel, relative_model=rel_model)
    assert np.all(vals > 0) and rel <= 8.0 * rel_model


@pytest.mark.parametrize('case', ee.SVD_CASES, ids=ee.svd_id)
def test_jacobi_svd(dev, case):
  """s, the vectors, T v = s u and the tied pair's span within the bounds; the route from the reported sweeps (0: the
  one workgroup or the Gram matrix; >= 1: the rounds); orthogonal vectors come back in the tie rule's order."""
  data = ee.svd_matrix(case)
  h = dev.default_handle()
  u, s, v, sweeps = dev.jacobi_svd(h.to_device(np.array(data.t), np.float64), case.dim)
  u, s, v = u.cpu().numpy(), s.cpu().numpy(), v.cpu().numpy()
  got, bound = ee.svd_measure(data, case.dim, u, s, v), ee.svd_bounds(case)
  mod, _, gaps, route, model_sweeps = ee.svd_reference(case)
  worst = int(np.argmax(got.vec / bound.vec))
  print('%s route %s sweeps %d (model %d) | s gpu %.3g model %.3g bound %.3g | null %.3g %.3g %.3g | vectors %.3g %.3g '
        '%.3g (g %.3g) | triplet %.3g %.3g %.3g | tie %.3g %.3g %.3g' % (
            ee.svd_id(case), route, sweeps, model_sweeps, got.s_rel, mod.s_rel, bound.s_rel, got.s_null, mod.s_null,
            bound.s_null, got.vec[worst], mod.vec[worst], bound.vec[worst], gaps[worst], got.triplet, mod.triplet,
            bound.triplet, got.tie, mod.tie, bound.tie))
  parity_log.record('eig_edges jacobi_svd ' + ee.svd_id(case), route=route, sweeps=sweeps, s_rel=got.s_rel,
                    s_rel_model=mod.s_rel, s_rel_bound=bound.s_rel, s_null=got.s_null, s_null_bound=bound.s_null,
                    vec=got.vec[worst], vec_model=mod.vec[worst], vec_bound=bound.vec[worst], triplet=got.triplet,
                    triplet_model=mod.triplet, triplet_bound=bound.triplet, tie=got.tie, tie_bound=bound.tie)
  assert (sweeps == 0) == (route in ('small', 'gram')), (route, sweeps)
  assert got.s_rel <= bound.s_rel and got.s_null <= bound.s_null
  assert np.all(got.vec <= bound.vec), (got.vec, bound.vec)
  assert got.triplet <= bound.triplet and got.tie <= bound.tie
  assert np.all(s[:-1] >= s[1:])
  if case.kind == 'orthogonal':
    model_v = ee.jacobi_svd_model(data.t, case.dim)[2 if case.tall else 0]
    assert np.array_equal(v if case.tall else u, model_v)
    assert sweeps <= 1


def _solve(dev, case, fused):
  """(the five outputs on the host, what the call reported, the statistics) of one td_cca_solve."""
  h = dev.default_handle()
  x, x2 = ee.cca_data(case)
  pre1, post1, pre2, post2 = ee.cca_lags(case)
  st = dev.LagStats(case.c1, pre1, post1, case.c2, pre2, post2)
  st.accumulate(h.to_device(x), h.to_device(x2), None, [0, len(x)])
  assert (st.k1, st.k2) == ee.cca_k(case)
  frames = st.counts()[0]
  options = ee.cca_options(case, fused)
  try:
    for name, value in options.items():
      h.set_option(name, value)
    st.cca_solve(ee.cca_denom(case, frames), case.reg, case.dim)
    out = st.cca_results_host()
  finally:
    h.set_option('cca_whitening', 0)
    h.set_option('cca_fused', 1)
  return out, ee.Resolved(st.last_cca_fused, st.last_cca_route, st.last_cca_route_y, None), st


def _check_cca(dev, case, fused):
  out, said, st = _solve(dev, case, fused)
  mom = cs.device_moments(st)
  ref = ee.cca_reference(case, mom, fused)
  rep = ee.cca_check(out, ref)
  tag = '%s %s' % (case.name, 'fused' if fused else 'chain')
  print('%s: %s svd %s dropped %d | e err %.3g bound %.3g ratio %.3f | rot err %.3g bound %.3g ratio %.3f | invariants '
        '%.3g | D_e %.2g D_rot %.2g g %.2g' % (tag, tuple(said[:3]), ref.svd_route, ref.dropped_y, rep.err_e, rep.bound_e,
                                                rep.ratio_e, rep.err_rot, rep.bound_rot, rep.ratio_rot, rep.invariants,
                                                rep.d_e, rep.d_rot, rep.g))
  parity_log.record('eig_edges cca_solve ' + tag, d_e=rep.d_e, d_rot=rep.d_rot, g=rep.g, e_vs_ref64=rep.err_e,
                    e_bound=rep.bound_e, e_over_bound=rep.ratio_e, rot_vs_ref64=rep.err_rot, rot_bound=rep.bound_rot,
                    rot_over_bound=rep.ratio_rot, invariants=rep.invariants, means_bitwise=rep.means_ok)
  # the route the device reports is the restated arithmetic's, on the device's own moments
  assert tuple(said[:3]) == tuple(ref.resolved[:3]), (said, ref.resolved)
  # the table's conditions hold on the device's moments too
  cxx, cyy, _ = ref.cov
  assert ee.eig_margin(cxx)[1] and ee.eig_margin(cyy)[1]
  excluded = int(np.sum(~ref.compared))
  assert excluded <= 1 and (excluded == 0 or case.kind in ('copy', 'zero'))
  assert rep.g >= ee.G_MIN, rep.g
  if case.kind in ('copy', 'zero') and case.reg == 0.0:
    assert ee.eig_margin(cyy)[0] <= ee.EPS_EIG and ref.dropped_y == 1          # exactly one eigenvalue is dropped
  if case.kind == 'zero' and case.reg > 0.0:
    assert ref.dropped_y == 0 and out[4][-1] == 0.0                            # the last singular value is exactly 0
  assert rep.means_ok and not rep.failures, rep.failures
  assert rep.ratio_e <= 1.0 and rep.ratio_rot <= 1.0 and rep.invariants <= ee.INVARIANT_TOL
  return ref


@pytest.mark.parametrize('case', ee.FUSED_CASES, ids=ee.cca_id)
def test_cca_solve_one_launch_shapes(dev, case):
  """The one launch (or, where its certificate refuses, the chain it hands over to), then the chain on the same
  statistics with cca_fused = 0: both within the bound of the same reference."""
  ref = _check_cca(dev, case, True)
  assert ref.resolved.fused == (case.kind != 'indefinite')
  assert not _check_cca(dev, case, False).resolved.fused


@pytest.mark.parametrize('case', ee.CHAIN_CASES, ids=ee.cca_id)
def test_cca_solve_chain(dev, case):
  assert not _check_cca(dev, case, True).resolved.fused
