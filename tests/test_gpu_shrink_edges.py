"""The Ledoit-Wolf kernels of csrc/shrink.hip on the MI355X at their edges (the cases of tests/shrink_edges.py, which
tests/test_cpu_shrink_edges.py shows to reach them and to be sensitive enough): td_shrinkage_moment on both routes of
its centred squares with minibatches that span recordings, shorter last minibatches, odd lag counts, more than 64
channels, strided and misaligned views and both signs of the offset; td_shrinkage_terms and td_shrunk_covariance on
their own against long double, at sizes around a workgroup and past the caps of their grids; and the fit
(lamb = -1, use_ridge = False) at K = 260 with spanning minibatches against the oracle.  The observed distances are in
DESIGN section 29."""
import ctypes

import numpy as np
import pytest

from oracle import lag as o_lag
from oracle import regression as o_reg
from tests import host_device as hd
from tests import parity_log
from tests import shrink_edges as se

pytestmark = pytest.mark.gpu

BOUND = 2e-6               # the suite's bound for td_shrinkage_moment (tests/test_gpu_fit.py)
_WORST = {}                # group -> (device's relative error, the float32 reference's on that case, case)


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


@pytest.fixture(scope='module', autouse=True)
def _record_worst():
  yield
  for group, (rel, ref32, where) in sorted(_WORST.items()):
    parity_log.record('shrink_edge_moment_worst', group=group, rel=rel, reference_fp32_rel=ref32, where=where,
                      reference_fp32_worst=max(abs(se.references(c)[2] - se.references(c)[0]) / se.references(c)[0]
                                               for c in (se.CASES_B if group == 'B' else se.CASES_A)))


def _device_moment(dev, case, view=None):
  c, pre, post, off, lens, batch, drop = case
  h = dev.default_handle()
  x = np.concatenate(se.recordings(case))
  if view is None:
    xd = h.to_device(x)
  else:
    extra, col = view
    wide = h.to_device(np.random.default_rng(7).standard_normal((x.shape[0], c + extra)).astype(np.float32))
    wide[:, col:col + c] = h.to_device(x)
    xd = wide[:, col:col + c]
    assert xd.stride(0) == c + extra and xd.data_ptr() == wide.data_ptr() + 4 * col and not xd.is_contiguous()
  offs = np.concatenate(([0], np.cumsum(lens)))
  _, _, used = se.layout(case)
  return dev.shrinkage_moment(xd, offs, pre, post, batch, input_offset=off, rows_used=used, handle=h)


def _check_moment(dev, case, group, view=None):
  want, _, f32 = se.references(case)
  got = _device_moment(dev, case, view)
  rel, ref32 = abs(got - want) / abs(want), abs(f32 - want) / abs(want)
  where = se.case_id(case) + ('' if view is None else '-ld+%d-col%d' % view)
  print('shrink edge moment %s: got %.17g want %.17g rel %.3g (float32 reference %.3g) route %s' % (
      where, got, want, rel, ref32, se.route(case)))
  parity_log.record('shrink_edge_moment', where=where, group=group, rel=rel, reference_fp32_rel=ref32)
  if group not in _WORST or rel > _WORST[group][0]:
    _WORST[group] = (rel, ref32, where)
  assert abs(got - want) <= BOUND * abs(want), (where, rel)


# ---- 1. the moment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', se.CASES_A, ids=se.case_id)
def test_moment_small_k_edges(dev, case):
  """Group A: a wrong edge sample moves these by 3.9e-5 or more (tests/test_cpu_shrink_edges.py)."""
  _check_moment(dev, case, 'A')


@pytest.mark.parametrize('case', se.CASES_B, ids=se.case_id)
def test_moment_spanning_minibatches_above_256_features(dev, case):
  """Group B: a piece of a spanning minibatch's column sums added twice moves these by 2e-3 or more."""
  _check_moment(dev, case, 'B')


@pytest.mark.parametrize('view', se.VIEWS, ids=lambda v: 'ld+%d-col%d' % v)
@pytest.mark.parametrize('case', se.VIEW_CASES, ids=se.case_id)
def test_moment_of_column_slices(dev, case, view):
  """x as a column slice of a wider tensor: aligned with ldx > c (16-byte staging loads), and neither aligned nor a
  row stride of whole float4s (scalar staging)."""
  _check_moment(dev, case, 'B' if case in se.CASES_B else 'A', view)
  # the same values in the same order, however they were staged: the bits of the dense call
  assert _device_moment(dev, case, view) == _device_moment(dev, case)


def test_moment_is_repeatable(dev):
  """Every sum of these kernels has a fixed order: the same call returns the same bits, whatever ran in between
  (the workspace is shared)."""
  for case, other in ((se.B1, se.A3), (se.B5, se.B2), (se.A1, se.B1)):
    got = []
    for _ in range(3):
      got.append(_device_moment(dev, case))
      _device_moment(dev, other)
    assert got[0] == got[1] == got[2], (se.case_id(case), got)


# ---- 2. the shrinkage algebra ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', se.ALGEBRA_N)
def test_shrinkage_terms_match_long_double(dev, n):
  """trace(zc) and sum(zc^2) of the [n + 1, n + 1] corner (the sums' row inside it) and of the [n, n] corner (the
  row outside it, ld > n), within the allowance of a float64 evaluation in any order."""
  h = dev.default_handle()
  s = se.moments_like(n)
  sd = h.to_device(s, np.float64)
  worst = 0.0
  for m in (n + 1, n):
    trace, sq, tol_trace, tol_sq = se.terms_reference(s, m, n)
    got_trace, got_sq = dev.shrinkage_terms(sd, m, n, se.FRAMES, handle=h)
    err_trace = float(abs(se.LD(got_trace) - trace))
    err_sq = float(abs(se.LD(got_sq) - sq))
    print('shrinkage terms n=%d corner %d: trace err %.3g of %.3g, squares err %.3g of %.3g' % (
        n, m, err_trace, tol_trace, err_sq, tol_sq))
    worst = max(worst, err_trace / tol_trace, err_sq / tol_sq)
    assert err_trace <= tol_trace, (n, m, err_trace / tol_trace)
    assert err_sq <= tol_sq, (n, m, err_sq / tol_sq)
  parity_log.record('shrink_edge_terms', n=n, worst_fraction_of_allowance=worst)


def _shrunk(h, sd, n, scale, diag, o64, o32):
  h.check(h.lib.td_shrunk_covariance(h.ptr, ctypes.c_void_p(sd.data_ptr()), sd.stride(0), n, scale, diag,
                                     ctypes.c_void_p(o64.data_ptr() if o64 is not None else 0),
                                     ctypes.c_void_p(o32.data_ptr() if o32 is not None else 0)))


@pytest.mark.parametrize('n', se.ALGEBRA_N)
def test_shrunk_covariance_matches_long_double(dev, n):
  """scale * S[:n, :n] + diag * I from a matrix with ld = n + 1 into outputs with room behind the corner: both
  outputs, each alone, nothing written behind the n * n entries."""
  import torch
  h = dev.default_handle()
  s = se.moments_like(n)
  sd = h.to_device(s, np.float64)
  scale, diag = (1.0 + 1.7e-3) / se.FRAMES, -0.37
  want = se.LD(scale) * s[:n, :n].astype(se.LD) + se.LD(diag) * np.eye(n, dtype=se.LD)
  tol = se.EPS * (np.abs(scale * s[:n, :n]) + abs(diag) * np.eye(n))
  room, mark = (n + 1) * (n + 1), -7.25
  worst, first64 = 0.0, None
  for want64, want32 in ((True, True), (True, False), (False, True)):
    o64 = torch.full((room,), mark, dtype=torch.float64, device=sd.device) if want64 else None
    o32 = torch.full((room,), mark, dtype=torch.float32, device=sd.device) if want32 else None
    _shrunk(h, sd, n, scale, diag, o64, o32)
    if want64:
      got = o64.cpu().numpy()
      assert np.all(got[n * n:] == mark)
      got = got[:n * n].reshape(n, n)
      err = np.abs(got.astype(se.LD) - want).astype(np.float64)
      assert np.all(err <= tol), (n, float(np.max(err / tol)))
      worst = max(worst, float(np.max(err / tol)))
      first64 = got if first64 is None else first64
      np.testing.assert_array_equal(got, first64)            # alone or with the float32 output: the same bits
    if want32:
      got32 = o32.cpu().numpy()
      assert np.all(got32[n * n:] == mark)
      np.testing.assert_array_equal(got32[:n * n].reshape(n, n), first64.astype(np.float32))
  parity_log.record('shrink_edge_covariance', n=n, worst_fraction_of_allowance=worst)
  # the wrapper's own outputs: the same bits
  a, a32 = dev.shrunk_covariance(sd, n, scale, diag, handle=h)
  np.testing.assert_array_equal(a.cpu().numpy(), first64)
  np.testing.assert_array_equal(a32.cpu().numpy(), first64.astype(np.float32))


# ---- 3. the fit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [se.B1, se.B2], ids=se.case_id)
def test_ledoit_wolf_fit_above_256_features(dev, case, monkeypatch):
  """lamb = -1, use_ridge = False through TestBrainData at K = 260 with minibatches that span recordings, against
  the oracle in float64, at the bounds of test_ledoit_wolf_regression_matches_reference_golden."""
  from telluride_decoding_amd import brain_data, brain_model
  c, pre, post, off, lens, batch, _ = case
  rng = np.random.default_rng(5 + c)
  bd = brain_data.TestBrainData('eeg', 'env', 100.0, pre_context=pre, post_context=post, input_offset=off,
                                final_batch_size=batch)
  files = []
  for x in se.recordings(case):
    y = (x[:, :1] * 0.5 + rng.standard_normal((x.shape[0], 1)) * 0.1).astype(np.float32)
    bd.add_file(x, y)
    files.append((x, y, y, np.zeros((x.shape[0], 1), np.float32)))
  ran = []
  for name in ('spd_solve', 'general_solve'):
    fn = getattr(dev, name)
    monkeypatch.setattr(dev, name, lambda *a, _fn=fn, _name=name, **k: (ran.append(_name), _fn(*a, **k))[1])
  w1, b1, _, _, sh1 = brain_model.calculate_linear_regressor_parameters_from_dataset(
      bd.create_dataset('train'), lamb=-1, use_ridge=False)
  batches = list(o_lag.minibatches(files, batch, pre=pre, post=post, input_offset=off))
  assert len(batches) == se.route(case)['total'] // batch >= 5
  f64 = [({'input_1': bx['input_1'].astype(np.float64)}, by.astype(np.float64)) for bx, by in batches]
  w0, b0, _, _, sh0 = o_reg.linear_regressor_from_batches(f64, lamb=-1, use_ridge=False)
  w32, b32, _, _, _ = o_reg.linear_regressor_from_batches(batches, lamb=-1, use_ridge=False)
  ref32 = hd.maxnorm_rel(np.vstack((w32, b32)), np.vstack((w0, b0)))
  err = hd.maxnorm_rel(np.vstack((w1, b1)), np.vstack((w0, b0)))
  print('shrink edge fit %s: shrinkage %.9g (oracle %.9g), weights %.3g (float32 reference %.3g), solvers %s' % (
      se.case_id(case), sh1, sh0, err, ref32, ran))
  parity_log.record('shrink_edge_fit', where=se.case_id(case), shrinkage=sh1, shrinkage_rel=abs(sh1 - sh0) / abs(sh0),
                    maxnorm_rel=err, reference_fp32_rel=ref32, solver='+'.join(ran))
  assert abs(sh1 - sh0) < 1e-4 * abs(sh0)
  assert err < ref32 + 1e-5, (err, ref32)
  # a negative shrinkage: (1 - s) cov + s mu I may be indefinite, the solve is the LU
  assert sh0 < 0.0 and ran == ['general_solve']
