"""CPU tests of the CCA leave-one-file-out x lambda sweep: the orchestration of cca_sweep.py with the NumPy stand-in
of tests/host_cca_sweep.py as device layer, against from-scratch float64 oracle refits; the public interface."""
import io

import numpy as np
import pytest

from tests import host_cca_sweep as hc
from tests import host_device


def _dataset(files, c, off=0, **kwargs):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(list(files), hc.BATCH, c['pre'], c['post'], c['pre2'], c['post2'], off, **kwargs)


@pytest.mark.parametrize('off', [0, 2, -3])
def test_orchestration_against_refits_from_scratch(off):
  """Case A (every fold's training stream drops a remainder, the means matter, lambda on both sides): all 15
  entries and the (mean, std) summary, on the batched route and on the forced fallback.  atol = 2e-6 as the ridge
  sweep's CPU test (float32 rotations and predictions of the stand-in; the float64 route measures 1.4e-15)."""
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  want = hc.case_a_oracle(off)
  assert want.shape == (3, 5) and np.all(want > 0.3)
  ds = _dataset(hc.case_a_files(), c, off)
  before = dict(hc.CALLS)
  res = regression.jackknife_over_regularizations(ds, list(c['lambdas']), device=hc, model='cca', cca_dims=c['dim'])
  assert hc.CALLS['cca_solve_loso_terms'] == before['cca_solve_loso_terms'] + 1
  assert hc.CALLS['cca_solve'] == before['cca_solve']
  assert regression.LAST_SWEEP['cca_route'] == 'batched'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 15, 'per_fold': 0}
  np.testing.assert_allclose(res['all_runs'], want, rtol=0, atol=2e-6)
  assert list(res) == list(c['lambdas']) + ['all_runs']
  for li, lam in enumerate(c['lambdas']):
    np.testing.assert_allclose(res[lam], (np.mean(want[li]), np.std(want[li])), rtol=0, atol=2e-6)
  forced = regression.jackknife_over_regularizations(ds, list(c['lambdas']), device=hc, model='cca',
                                                     cca_dims=c['dim'], _route='per_fold')
  assert regression.LAST_SWEEP['cca_route'] == 'per_fold'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 0, 'per_fold': 15}
  np.testing.assert_allclose(forced['all_runs'], want, rtol=0, atol=2e-6)


def test_marked_pairs_and_wide_input_2_take_the_fallback(monkeypatch):
  """A (fold, lambda) the device call marks is refitted alone ('batched+per_fold'); an input_2 of more than 64
  lagged columns sends the whole sweep to the fallback without asking the device call."""
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  want = hc.case_a_oracle(0)
  ds = _dataset(hc.case_a_files(), c)
  real = hc.LagStats.cca_solve_loso_terms

  def marking(*args, **kwargs):
    out = list(real(*args, **kwargs))
    out[0][1][:, 2 * c['dim']:] = float('nan')     # (what a marked pair leaves behind is not to be used)
    out[0][3][:, :c['dim']] = float('nan')
    out[7][1, 2] = 1
    out[7][3, 0] = 1
    return tuple(out)

  monkeypatch.setattr(hc.LagStats, 'cca_solve_loso_terms', staticmethod(marking))
  res = regression.jackknife_over_regularizations(ds, list(c['lambdas']), device=hc, model='cca', cca_dims=c['dim'])
  assert regression.LAST_SWEEP['cca_route'] == 'batched+per_fold'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 13, 'per_fold': 2}
  np.testing.assert_allclose(res['all_runs'], want, rtol=0, atol=2e-6)
  monkeypatch.undo()
  wide = dict(c, pre2=16, post2=16)          # K2 = 66
  before = hc.CALLS['cca_solve_loso_terms']
  res = regression.jackknife_over_regularizations(_dataset(hc.case_a_files(), wide), [0.1], device=hc, model='cca',
                                                  cca_dims=c['dim'], folds=[0, 3])
  assert hc.CALLS['cca_solve_loso_terms'] == before
  assert regression.LAST_SWEEP['cca_route'] == 'per_fold' and res['all_runs'].shape == (1, 2)
  files = hc.case_a_files()
  for fi, f in enumerate((0, 3)):
    r = hc.oracle_refit(files, f, 0.1, c['dim'], c['pre'], c['post'], 16, 16)
    assert abs(res['all_runs'][0, fi] - r) <= 2e-6


def test_value_errors():
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  files = hc.case_a_files()
  ds = _dataset(files, c)
  with pytest.raises(ValueError, match='one rank'):
    regression.jackknife_over_regularizations(ds, [0.1], world_size=2, device=hc, model='cca')
  with pytest.raises(ValueError, match='mixup_batch'):
    regression.jackknife_over_regularizations(_dataset(files, c, mixup_batch=True), [0.1], device=hc, model='cca')
  none2 = [(f[0], f[1][:, :0], f[2], f[3]) for f in files]
  with pytest.raises(ValueError, match='Second input to CCA estimator'):
    regression.jackknife_over_regularizations(_dataset(none2, c), [0.1], device=hc, model='cca')
  with pytest.raises(ValueError, match="'linear' or 'cca'"):
    regression.jackknife_over_regularizations(ds, [0.1], device=hc, model='dnn')
  with pytest.raises(ValueError, match='Could not find metric'):
    regression.jackknife_one_model(ds, 0.1, test_metric='cca_pearson_correlation_second', device=hc)


def test_linear_model_is_untouched():
  """model='linear' is the call without the keyword, bit for bit."""
  from telluride_decoding_amd import brain_data, regression
  files = hc.case_a_files()
  ds = brain_data.Dataset(list(files), hc.BATCH, 1, 2)
  plain = regression.jackknife_over_regularizations(ds, [1e-3, 0.1], device=host_device)
  keyed = regression.jackknife_over_regularizations(ds, [1e-3, 0.1], device=host_device, model='linear')
  assert list(plain) == list(keyed)
  np.testing.assert_array_equal(plain['all_runs'], keyed['all_runs'])
  for lam in (1e-3, 0.1):
    assert plain[lam] == keyed[lam]


def test_jackknife_one_model_with_the_cca_metric():
  from telluride_decoding_amd import regression
  c = hc.CASE_A
  ds = _dataset(hc.case_a_files(), c)
  want = hc.case_a_oracle(0)[1]
  buf = io.StringIO()
  cors = regression.jackknife_one_model(ds, c['lambdas'][1], test_name='cca', trial_number=2, summary_file=buf,
                                        test_metric='cca_pearson_correlation_first', experiment_parameters='d=3',
                                        device=hc, cca_dims=c['dim'])
  np.testing.assert_allclose(cors, want, rtol=0, atol=2e-6)
  assert buf.getvalue() == ('Jackknife test result test=cca, regularization lambda=0.1, trial=2, mean correlation=%s, '
                            'std=%s, test count=5\nJackknife parameters:d=3\n' % (np.mean(cors), np.std(cors)))
  first2 = regression.jackknife_one_model(ds, c['lambdas'][1], max_test_count=2, device=hc, cca_dims=c['dim'],
                                          test_metric='cca_pearson_correlation_first')
  np.testing.assert_allclose(first2, want[:2], rtol=0, atol=2e-6)
  only = regression.jackknife_one_model(ds, c['lambdas'][1], test_file=4, device=hc, cca_dims=c['dim'],
                                        test_metric='cca_pearson_correlation_first')
  np.testing.assert_allclose(only, want[4:], rtol=0, atol=2e-6)
