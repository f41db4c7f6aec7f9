"""GPU tests of the CCA leave-one-file-out x lambda sweep (regression.jackknife_over_regularizations(model='cca'),
cca_sweep.py, td_cca_solve_loso_terms) against from-scratch float64 oracle refits.

Tolerance of the end-to-end tests.  The sweep's held-out correlations pass through float32 rotations and the float32
projection kernel; the route that predates the sweep (BrainModelCCA.fit on the training files, .evaluate on the
held-out one) starts from the same per-sample products, summed in another order and whitened differently.  Its distance
from the oracle over the same (fold, lambda) pairs, E_ref, is measured in the test and the sweep must stay within
2 E_ref + 2e-6 (the floor keeps a lucky E_ref from asking for bit-equality) -- and within 3e-5 whatever E_ref is: the
smallest of the deliberate mistakes the cases were designed to expose (denom = n instead of n - 1) moves some entry
of case A by that much.
"""
import functools
import io

import numpy as np
import pytest

from tests import host_cca_sweep as hc
from tests import parity_log

pytestmark = pytest.mark.gpu

SMALLEST_MISTAKE = 3e-5


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _dataset(files, c, off=0):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(list(files), hc.BATCH, c['pre'], c['post'], c['pre2'], c['post2'], off)


def _case_a(lags2=None):
  c = dict(hc.CASE_A)
  if lags2 is not None:
    c['pre2'] = c['post2'] = lags2
  return c


@functools.lru_cache(maxsize=None)
def _parent_route(case, off, pairs, lags2=None):
  """{(fold, lambda index): r} of the route that exists without the sweep: a BrainModelCCA fit per pair."""
  from telluride_decoding_amd import cca
  c, files = (_case_a(lags2), hc.case_a_files()) if case == 'a' else (hc.CASE_B, hc.case_b_files())
  out = {}
  for f, li in pairs:
    train = _dataset([g for i, g in enumerate(files) if i != f], c, off)
    model = cca.BrainModelCCA(train, cca_dims=c['dim'], regularization_lambda=c['lambdas'][li])
    model.fit(train)
    out[(f, li)] = model.evaluate(_dataset([files[f]], c, off))['cca_pearson_correlation_first']
  return out


def _bound(case, off, pairs, want, lags2=None):
  ref = _parent_route(case, off, tuple(pairs), lags2)
  e_ref = max(abs(ref[p] - want[p]) for p in pairs)
  return e_ref, min(2.0 * e_ref + 2e-6, SMALLEST_MISTAKE)


ALL_A = tuple((f, li) for f in range(5) for li in range(3))


@pytest.mark.parametrize('off', [0, 2, -3])
def test_sweep_equals_refits_from_scratch_case_a(dev, off):
  """All 15 (fold, lambda) entries of case A and the (mean, std) summary against oracle refits, every pair on the
  batched route (the float64 restatement factors every system: a fallback here is a failure)."""
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  want = hc.case_a_oracle(off)                                   # [Lambda, F]
  res = regression.jackknife_over_regularizations(_dataset(hc.case_a_files(), c, off), list(c['lambdas']), model='cca',
                                                  cca_dims=c['dim'])
  assert regression.LAST_SWEEP['cca_route'] == 'batched'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 15, 'per_fold': 0}
  got = res['all_runs']
  assert got.shape == (3, 5) and list(res)[:3] == list(c['lambdas'])
  e_ref, bound = _bound('a', off, ALL_A, {(f, li): want[li, f] for f, li in ALL_A})
  err = float(np.max(np.abs(got - want)))
  parity_log.record('cca_sweep_case_a_off%d' % off, e_ref=e_ref, sweep=err, bound=bound)
  print('case A off %d: E_ref %.3g sweep %.3g bound %.3g' % (off, e_ref, err, bound))
  assert err <= bound, (err, e_ref, bound)
  for li, lam in enumerate(c['lambdas']):
    assert abs(res[lam][0] - np.mean(want[li])) <= bound and abs(res[lam][1] - np.std(want[li])) <= bound


def test_sweep_equals_refits_from_scratch_case_b(dev):
  """Case B (K1 = 144: above 128, no multiple of 64; K2 = 31; 35 output columns): six sampled pairs."""
  from telluride_decoding_amd import regression
  c = hc.CASE_B
  want = hc.case_b_oracle()
  res = regression.jackknife_over_regularizations(_dataset(hc.case_b_files(), c), list(c['lambdas']), model='cca',
                                                  cca_dims=c['dim'])
  assert regression.LAST_SWEEP['cca_route'] == 'batched'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 28, 'per_fold': 0}
  e_ref, bound = _bound('b', 0, hc.CASE_B_PAIRS, want)
  err = max(abs(res['all_runs'][li, f] - want[(f, li)]) for f, li in hc.CASE_B_PAIRS)
  parity_log.record('cca_sweep_case_b', e_ref=e_ref, sweep=err, bound=bound)
  print('case B: E_ref %.3g sweep %.3g bound %.3g' % (e_ref, err, bound))
  assert err <= bound, (err, e_ref, bound)


def test_batched_route_equals_per_fold_route(dev):
  """Case A: the forced fallback gives the same 'all_runs' as the batched route."""
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  ds = _dataset(hc.case_a_files(), c)
  want = hc.case_a_oracle(0)
  _, bound = _bound('a', 0, ALL_A, {(f, li): want[li, f] for f, li in ALL_A})
  batched = regression.jackknife_over_regularizations(ds, list(c['lambdas']), model='cca', cca_dims=c['dim'])['all_runs']
  assert regression.LAST_SWEEP['cca_route'] == 'batched'
  forced = regression.jackknife_over_regularizations(ds, list(c['lambdas']), model='cca', cca_dims=c['dim'],
                                                     _route='per_fold')['all_runs']
  assert regression.LAST_SWEEP['cca_route'] == 'per_fold'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 0, 'per_fold': 15}
  err = float(np.max(np.abs(batched - forced)))
  parity_log.record('cca_sweep_batched_vs_per_fold', distance=err, bound=bound)
  assert err <= bound, (err, bound)


def _file_stats(dev, h, x, x2, pre, post, pre2, post2):
  st = dev.LagStats(x.shape[1], pre, post, x2.shape[1], pre2, post2, 0, handle=h)
  st.accumulate(h.to_device(x), h.to_device(x2), None, [0, x.shape[0]])
  return st


def _check_models(dev, h, out, fold_stats, lambdas, dim):
  """The device call's models against cca_solve on each fold's summed statistics: status 0, e within 1e-5 relative,
  rotations up to the joint sign of a component at 1e-4 of the largest entry, means, biases = -mean . rot."""
  rot_x, rot_y, mean_x, mean_y, bias_x, bias_y, e, status = (np.asarray(t.cpu()) for t in out)
  assert not status.any(), status
  for fi, st in enumerate(fold_stats):
    frames = st.counts()[0]
    for li, lam in enumerate(lambdas):
      st.cca_solve(frames - 1, lam, dim, handle=h)
      rx, ry, mx, my, ev = st.cca_results_host()
      cols = slice(li * dim, (li + 1) * dim)
      gx, gy = rot_x[fi][:, cols].astype(np.float64), rot_y[fi][:, cols].astype(np.float64)
      np.testing.assert_allclose(e[fi, li], ev, rtol=1e-5)
      sign = np.sign(np.sum(gx * rx, axis=0))
      assert np.all(sign != 0)
      np.testing.assert_allclose(gx * sign, rx, rtol=0, atol=1e-4 * np.max(np.abs(rx)))
      np.testing.assert_allclose(gy * sign, ry, rtol=0, atol=1e-4 * np.max(np.abs(ry)))
      np.testing.assert_allclose(mean_x[fi], mx[0], rtol=0, atol=2e-6 * max(1.0, np.max(np.abs(mx))))
      np.testing.assert_allclose(mean_y[fi], my[0], rtol=0, atol=2e-6 * max(1.0, np.max(np.abs(my))))
      # (the biases are float32 roundings of the float64 -mean . rot)
      bx = -(mean_x[fi].astype(np.float64) @ gx)
      by = -(mean_y[fi].astype(np.float64) @ gy)
      scale_x = np.sum(np.abs(mean_x[fi][:, None] * gx), axis=0) + 1e-30
      scale_y = np.sum(np.abs(mean_y[fi][:, None] * gy), axis=0) + 1e-30
      assert np.all(np.abs(bias_x[fi][cols] - bx) <= 1e-6 * scale_x)
      assert np.all(np.abs(bias_y[fi][cols] - by) <= 1e-6 * scale_y)


def test_device_call_equals_cca_solve_on_summed_folds(dev):
  """Case A through the device call: folds = total minus the held-out recording (one term; minibatches of one frame,
  so that any frame count is a whole number of them) against cca_solve on the summed statistics."""
  c, files = hc.CASE_A, hc.case_a_files()
  h = dev.default_handle()
  stats = [_file_stats(dev, h, f[0], f[1], c['pre'], c['post'], c['pre2'], c['post2']) for f in files]
  total = stats[0].like().combine(stats)
  frames = [st.counts()[0] for st in stats]
  terms = [[(stats[f], -1.0)] for f in range(len(files))]
  out = dev.LagStats.cca_solve_loso_terms(total, terms, [sum(frames) - n for n in frames], 1, c['lambdas'], c['dim'],
                                          handle=h)
  folds = [stats[0].like().combine([s for i, s in enumerate(stats) if i != f]) for f in range(len(files))]
  _check_models(dev, h, out, folds, c['lambdas'], c['dim'])


# (c1, lags1, c2, lags2): K1 x K2 = 3 x 1, 5 x 2, 64 x 16, 65 x 17, 144 x 31, 70 x 64
EDGE_SHAPES = [(3, 1, 1, 1), (5, 1, 2, 1), (8, 8, 2, 8), (13, 5, 1, 17), (24, 6, 1, 31), (14, 5, 2, 32)]


@pytest.mark.parametrize('c1,l1,c2,l2', EDGE_SHAPES)
def test_kernel_edges_through_the_device_call(dev, c1, l1, c2, l2):
  """One fold with zero terms (the fold IS the total) and one with a term, on a few hundred random frames, at the
  tile edges of K1 and K2, two lambdas, against td_cca_solve on the same statistics."""
  rng = np.random.default_rng(100 * c1 + l2)
  h = dev.default_handle()
  parts = []
  for n in (260, 170):
    x = rng.standard_normal((n, c1)).astype(np.float32) + 1.0
    mix = rng.standard_normal((c1, c2)) / np.sqrt(c1)
    x2 = (x @ mix + 0.7 * rng.standard_normal((n, c2)) - 2.0).astype(np.float32)
    parts.append(_file_stats(dev, h, x, x2, 0, l1 - 1, l2 // 2, l2 - 1 - l2 // 2))
  total = parts[0].like().combine(parts)
  assert (total.k1, total.k2) == (c1 * l1, c2 * l2)
  dim = min(5, total.k1, total.k2)
  lambdas = [1e-2, 1.0]
  out = dev.LagStats.cca_solve_loso_terms(total, [[], [(parts[1], -1.0)]], [430, 260], 1, lambdas, dim, handle=h)
  _check_models(dev, h, out, [total, parts[0]], lambdas, dim)


def test_out_of_range_is_an_error_not_a_fault(dev):
  """k2 > 64, more than four terms, a bad dim and a frame count that is no whole number of minibatches."""
  h = dev.default_handle()
  rng = np.random.default_rng(5)
  x, x2 = rng.standard_normal((200, 4)).astype(np.float32), rng.standard_normal((200, 2)).astype(np.float32)
  wide = _file_stats(dev, h, x, x2, 0, 1, 16, 16)               # K2 = 66
  with pytest.raises(ValueError, match='at most 64'):
    dev.LagStats.cca_solve_loso_terms(wide, [[]], [200], 1, [0.1], 2, handle=h)
  st = _file_stats(dev, h, x, x2, 0, 1, 1, 1)
  with pytest.raises(ValueError, match='terms'):
    dev.LagStats.cca_solve_loso_terms(st, [[(st, -1.0), (st, 1.0)] * 3], [200], 1, [0.1], 2, handle=h)
  with pytest.raises(ValueError, match='dim'):
    dev.LagStats.cca_solve_loso_terms(st, [[]], [200], 1, [0.1], 7, handle=h)
  with pytest.raises(ValueError, match='minibatches'):
    dev.LagStats.cca_solve_loso_terms(st, [[]], [3], 100, [0.1], 2, handle=h)


def test_designed_fallback_for_a_wide_input_2(dev):
  """Case A with input_2 = 2 channels x 33 lags (K2 = 66 > 64): the whole sweep takes the per-fold route."""
  from telluride_decoding_amd import regression
  c = _case_a(16)
  pairs = ((0, 0), (2, 1), (4, 2))
  res = regression.jackknife_over_regularizations(_dataset(hc.case_a_files(), c), list(c['lambdas']), model='cca',
                                                  cca_dims=c['dim'])
  assert regression.LAST_SWEEP['cca_route'] == 'per_fold'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 0, 'per_fold': 15}
  files = hc.case_a_files()
  want = {(f, li): hc.oracle_refit(files, f, c['lambdas'][li], c['dim'], c['pre'], c['post'], 16, 16) for f, li in pairs}
  e_ref, bound = _bound('a', 0, pairs, want, 16)
  err = max(abs(res['all_runs'][li, f] - want[(f, li)]) for f, li in pairs)
  parity_log.record('cca_sweep_wide_input_2', e_ref=e_ref, sweep=err, bound=bound)
  assert err <= bound, (err, e_ref, bound)


def test_jackknife_one_model_takes_the_cca_metric(dev):
  """test_metric='cca_pearson_correlation_first' returns the lambda's row of 'all_runs', honours test_file /
  max_test_count and writes the reference's summary line."""
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  ds = _dataset(hc.case_a_files(), c)
  lam = c['lambdas'][1]
  row = regression.jackknife_over_regularizations(ds, [lam], model='cca', cca_dims=c['dim'])['all_runs'][0]
  buf = io.StringIO()
  cors = regression.jackknife_one_model(ds, lam, test_name='cca', trial_number=3, summary_file=buf,
                                        test_metric='cca_pearson_correlation_first', experiment_parameters='d=3',
                                        cca_dims=c['dim'])
  np.testing.assert_array_equal(cors, row)
  np.testing.assert_allclose(cors, hc.case_a_oracle(0)[1], rtol=0, atol=SMALLEST_MISTAKE)
  assert buf.getvalue() == ('Jackknife test result test=cca, regularization lambda=%s, trial=3, mean correlation=%s, '
                            'std=%s, test count=5\nJackknife parameters:d=3\n' % (lam, np.mean(cors), np.std(cors)))
  first2 = regression.jackknife_one_model(ds, lam, max_test_count=2, test_metric='cca_pearson_correlation_first',
                                          cca_dims=c['dim'])
  np.testing.assert_array_equal(first2, row[:2])
  only = regression.jackknife_one_model(ds, lam, test_file=4, test_metric='cca_pearson_correlation_first',
                                        cca_dims=c['dim'])
  np.testing.assert_array_equal(only, row[4:])
  with pytest.raises(ValueError, match='Could not find metric'):
    regression.jackknife_one_model(ds, lam, test_metric='cca_pearson_correlation_second')
