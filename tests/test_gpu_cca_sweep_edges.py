"""GPU sweep of the CCA sweep's device call (td_cca_solve_loso_terms, csrc/cca_sweep.hip over the batched Cholesky of
csrc/chol.hip) at the cases of tests/cca_sweep_edges.py: every output of every (fold, lambda) pair against the float64
reference of that module, built from the device's own float64 moments, within its derived bound -- in effect one
float32 rounding of the output.  The means bit for bit, the statuses as the reference's three rules give them, the
refusals, a NaN, and the whole sweep end to end where the call must refuse half of its pairs.

Measured on an MI355X, the worst over the 689 solved pairs of all cases (the parity log has them per case):
  e          |gpu - ref| 2.98e-8 (batch_8),   0.941 of its bound (chunks_8_1)
  rotations  |gpu - ref| 5.91e-8 of the column's largest entry, 0.993 of its bound (chunk_clamp)
  D_e <= 5.6e-15 (k1_193), D_rot <= 4.7e-13 (k2_64), g >= 2.2e-3; every mean bit for bit.
The float64 terms of the bound are 1e-9 of a column at the most: what is measured is the float32 rounding of the
outputs, which is also all the room the bound leaves."""
import numpy as np
import pytest

from tests import cca_sweep_edges as ce
from tests import parity_log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _accumulate(dev, h, case):
  """(total, [statistics of every recording])"""
  pre1, post1, pre2, post2 = ce.lags(case)
  stats = []
  for x, x2 in ce.make_parts(case):
    st = dev.LagStats(case.c1, pre1, post1, case.c2, pre2, post2, 0, handle=h)
    st.accumulate(h.to_device(x), h.to_device(x2), None, [0, len(x)])
    stats.append(st)
  total = stats[0].like().combine(stats[:case.n_total])
  assert (total.k1, total.k2) == ce.case_k(case)
  return total, stats


def _run(dev, h, case):
  """The device call on the case and its report against the reference from the device's own moments."""
  total, stats = _accumulate(dev, h, case)
  terms = [[(stats[p], sg) for p, sg in fold] for fold in case.folds]
  out = dev.LagStats.cca_solve_loso_terms(total, terms, ce.fold_batches(case), case.batch_size, list(case.lambdas),
                                          case.dim, handle=h)
  out = tuple(np.asarray(t.cpu()) for t in out)
  ref = ce.reference(ce.device_moments(total), [ce.device_moments(st) for st in stats], case.folds, case.lambdas,
                     case.dim)
  rep = ce.check(out, ref)
  print('%s: e err %.3g bound %.3g ratio %.3f | rot err %.3g bound %.3g ratio %.3f | D_e %.2g D_rot %.2g g %.2g' % (
      case.name, rep.err_e, rep.bound_e, rep.ratio_e, rep.err_rot, rep.bound_rot, rep.ratio_rot, rep.d_e, rep.d_rot,
      rep.g))
  parity_log.record('cca_sweep_edges ' + case.name, pairs=rep.pairs_checked, d_e=rep.d_e, d_rot=rep.d_rot, g=rep.g,
                    e_vs_ref64=rep.err_e, e_bound=rep.bound_e, e_over_bound=rep.ratio_e, rot_vs_ref64=rep.err_rot,
                    rot_bound=rep.bound_rot, rot_over_bound=rep.ratio_rot, means_bitwise=rep.means_ok)
  return out, ref, rep, (total, stats)


@pytest.mark.parametrize('case', ce.PLAIN_CASES, ids=ce.case_id)
def test_every_output_of_every_pair(dev, case):
  """Status 0 everywhere; e, rot_x, rot_y inside the bound; mean_x, mean_y bit for bit; the biases."""
  _, ref, rep, _ = _run(dev, dev.default_handle(), case)
  assert rep.pairs_checked == len(case.folds) * len(case.lambdas), rep.failures
  assert rep.g >= ce.G_MIN, rep.g                  # (the gap condition holds on the device's moments too)
  assert rep.status_ok and rep.means_ok and rep.bias_ok and not rep.failures, rep.failures
  assert rep.ratio_e <= 1.0 and rep.ratio_rot <= 1.0


def _ridge_and_cca_still_work(dev, h, st_cca):
  """A ridge solve and a cca_solve on the handle that has just seen refused systems: no stale flag fails them."""
  rng = np.random.default_rng(2)
  x = rng.standard_normal((300, 4)).astype(np.float32)
  y = (x[:, :1] * 0.5 + rng.standard_normal((300, 1))).astype(np.float32)
  st = dev.LagStats(4, 0, 2, d=1, handle=h)
  st.accumulate(h.to_device(x), None, h.to_device(y), [0, 300])
  w, b = (t.cpu().numpy() for t in st.ridge_solve([0.1], handle=h))
  m = st.moments()
  xtx, xty, frames = m['xtx'].cpu().numpy(), m['xty'].cpu().numpy(), st.counts()[0]
  sol = np.linalg.solve(xtx / frames + 0.1 * np.eye(len(xtx)), xty / frames)
  assert np.max(np.abs(w[0] - sol[:-1])) <= 2.5e-7 * np.max(np.abs(sol)) and abs(b[0, 0] - sol[-1, 0]) <= 2.5e-7
  mom = ce.device_moments(st_cca)
  cxx, cyy, cxy, _, _ = ce.covariances(mom, 0.1)
  rx, ry, e, _ = ce.route_r1(cxx, cyy, cxy, 2)
  st_cca.cca_solve(mom.frames - 1, 0.1, 2, handle=h)
  gx, gy, _, _, ge = st_cca.cca_results_host()
  sign = np.sign(np.sum(gx * rx, axis=0))
  np.testing.assert_allclose(ge, e, rtol=1e-5)
  np.testing.assert_allclose(gx * sign, rx, rtol=0, atol=1e-4 * np.max(np.abs(rx)))
  np.testing.assert_allclose(gy * sign, ry, rtol=0, atol=1e-4 * np.max(np.abs(ry)))


@pytest.mark.parametrize('case', ce.STATUS_CASES, ids=ce.case_id)
def test_the_device_marks_the_right_pairs_and_only_those(dev, case):
  """A duplicated column: the pairs the three rules refuse report 1, their neighbours in the same launch report 0 and
  are inside the bound; afterwards the handle solves as before."""
  h = dev.default_handle()
  out, ref, rep, (total, stats) = _run(dev, h, case)
  expect = dict(case.expect)
  assert [[p.rules.status for p in row] for row in ref.pairs] == [list(r) for r in expect['status']]
  assert [[p.rules.rule for p in row] for row in ref.pairs] == [list(expect['rules'])] * len(case.folds)
  assert out[7].tolist() == [list(r) for r in expect['status']]
  assert rep.pairs_checked == sum(r.count(0) for r in expect['status'])
  assert rep.status_ok and rep.means_ok and rep.bias_ok and not rep.failures, rep.failures
  _ridge_and_cca_still_work(dev, h, stats[0])


def test_a_nan_marks_its_fold_and_the_call_returns(dev):
  """A NaN in one EEG channel of a recording that only the last fold adds: both pairs of that fold report 1, the other
  folds are right.  (Every loop of the factorisation, of the tail and of its Jacobi sweeps is bounded by a counter
  whatever the data: the rotation test and every pivot test are false on NaN.)"""
  case = ce.NAN_CASE
  h = dev.default_handle()
  out, ref, rep, (total, stats) = _run(dev, h, case)
  assert out[7].tolist() == [[0, 0], [0, 0], [1, 1]]
  assert rep.pairs_checked == 4
  assert rep.status_ok and rep.means_ok and rep.bias_ok and not rep.failures, rep.failures
  _ridge_and_cca_still_work(dev, h, stats[0])


def test_refusals_queue_nothing(dev):
  """4097 output columns, a negative lambda and a term of another layout are ValueErrors; the same call with the
  argument mended is right afterwards."""
  case = next(c for c in ce.CASES if c.name == 'k1_2')
  h = dev.default_handle()
  total, stats = _accumulate(dev, h, case)
  call = lambda terms, lambdas, dim: dev.LagStats.cca_solve_loso_terms(
      total, terms, [430] * len(terms), 1, lambdas, dim, handle=h)
  with pytest.raises(ValueError, match='output columns'):
    call([[]], list(np.linspace(0.1, 1.0, 4097)), 1)
  with pytest.raises(ValueError, match='output columns'):
    call([[]], list(np.linspace(0.1, 1.0, 2049)), 2)
  with pytest.raises(ValueError, match='lambda must be >= 0'):
    call([[]], [0.1, -1e-3], 1)
  other = dev.LagStats(case.c1, 0, 1, case.c2, 0, 0, 0, handle=h)             # two lags of input_1, not one
  x, x2 = ce.make_parts(case)[0]
  other.accumulate(h.to_device(x), h.to_device(x2), None, [0, len(x)])
  with pytest.raises(ValueError, match='layout differs'):
    dev.LagStats.cca_solve_loso_terms(total, [[(other, -1.0)]], [170], 1, [0.1], 1, handle=h)
  _, _, rep, _ = _run(dev, h, case)
  assert rep.pairs_checked == 4 and not rep.failures, rep.failures


def test_sweep_end_to_end_where_the_call_refuses_half_its_pairs(dev):
  """regression.jackknife_over_regularizations(model='cca') on three recordings with a duplicated EEG channel and
  lambdas (0, 0.1): the device call marks the three lambda = 0 pairs, the sweep refits exactly those, and all six values
  agree with from-scratch float64 refits within the bound rule of tests/test_gpu_cca_sweep.py (2 E_ref + 2e-6, at most
  3e-5; E_ref = the distance of the route that predates the sweep from the same oracle)."""
  from telluride_decoding_amd import brain_data, cca, regression
  from tests.test_gpu_cca_sweep import SMALLEST_MISTAKE
  c, files = ce.E2E, ce.e2e_files()
  dataset = lambda fs: brain_data.Dataset(list(fs), c['batch'], c['pre'], c['post'], c['pre2'], c['post2'])
  res = regression.jackknife_over_regularizations(dataset(files), list(c['lambdas']), model='cca', cca_dims=c['dim'])
  assert regression.LAST_SWEEP['cca_route'] == 'batched+per_fold'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 3, 'per_fold': 3}
  want = ce.e2e_oracle()
  parent = {}
  for f, li in want:
    train = dataset([g for i, g in enumerate(files) if i != f])
    model = cca.BrainModelCCA(train, cca_dims=c['dim'], regularization_lambda=c['lambdas'][li])
    model.fit(train)
    parent[(f, li)] = model.evaluate(dataset([files[f]]))['cca_pearson_correlation_first']
  e_ref = max(abs(parent[p] - want[p]) for p in want)
  bound = min(2.0 * e_ref + 2e-6, SMALLEST_MISTAKE)
  err = max(abs(res['all_runs'][li, f] - want[(f, li)]) for f, li in want)
  parity_log.record('cca_sweep_edges end_to_end', e_ref=e_ref, sweep=err, bound=bound)
  print('end to end: E_ref %.3g sweep %.3g bound %.3g' % (e_ref, err, bound))
  assert err <= bound, (err, e_ref, bound)
