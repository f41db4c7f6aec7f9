"""GPU sweep of the many-output FIR prediction and the CCA projection (csrc/decode.hip: project_mfma_kernel,
predict_fir_mfma_kernel, predict_fir_wave_kernel, predict_fir_kernel, cca_project_kernel<108> and the fallback of
td_cca_transform) at the cases of tests/fir_edges.py, against float64 (oracle.lag.lag_matrix @ w + b,
oracle.cca.cca_transform), in three tiers:

  exact       integer data whose every product and partial sum is a float32: bit equality, every sentinel untouched;
  real        rows 2^-20 .. 2^20 apart, relative to sum |terms|, within max(4e-7, 2 x the pessimistic float32 chain
              model's distance on the same data) (<= 2e-6; 6e-7 for the CCA transform);
  non-finite  a NaN / Inf spoils exactly the outputs whose window holds it (numpy's set), per output column.

x is a column slice of a wider array where the case has a pad; out is always a column slice of an array prefilled
with a sentinel."""
import numpy as np
import pytest

from tests import fir_edges as fe
from tests import parity_log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _sliced(h, a, pad):
  """a [rows, c] on the device as the first c columns of a [rows, c + pad] array of sentinels."""
  if not pad:
    return h.to_device(a)
  wide = np.full((a.shape[0], a.shape[1] + pad), fe.SENTINEL, np.float32)
  wide[:, :a.shape[1]] = a
  return h.to_device(wide)[:, :a.shape[1]]


def _run_fir(dev, case, data):
  """(out [rows, d], frame [rows, d + 3]): the call's output slice and the sentinel-filled array it is a slice of."""
  import torch
  h = dev.default_handle()
  rows = int(np.sum(case.lens))
  frame = torch.full((rows, case.d + 3), float(fe.SENTINEL), dtype=torch.float32, device=h.device)
  out = frame[:, 1:1 + case.d]
  offs = np.concatenate(([0], np.cumsum(case.lens)))
  x = _sliced(h, data.x, case.pad)
  if case.per_file:
    dev.predict_fir_per_file(x, offs, h.to_device(data.w), h.to_device(data.b), case.pre, case.post, out=out, handle=h,
                             input_offset=case.off)
  else:
    dev.predict_fir(x, offs, h.to_device(data.w), h.to_device(data.b.reshape(1, -1)).reshape(-1), case.pre, case.post,
                    out=out, handle=h, input_offset=case.off)
  frame = frame.cpu().numpy()
  return frame[:, 1:1 + case.d], frame


def _run_cca(dev, case, data):
  import torch
  h = dev.default_handle()
  rows = int(np.sum(case.lens))
  frame = torch.full((rows, 2 * case.dims + 3), float(fe.SENTINEL), dtype=torch.float32, device=h.device)
  out = frame[:, 1:1 + 2 * case.dims]
  offs = np.concatenate(([0], np.cumsum(case.lens)))
  vec = lambda v: h.to_device(v.reshape(1, -1)).reshape(-1)      # noqa: E731
  saved = h.accumulate_mode
  try:
    h.set_accumulate_mode(case.mode)
    dev.cca_transform(_sliced(h, data.x, case.pad), _sliced(h, data.x2, case.pad), offs, vec(data.mean1),
                      h.to_device(data.rot1), vec(data.mean2), h.to_device(data.rot2), case.pre1, 0, 0, 0, handle=h,
                      input_offset=case.off, out=out)
  finally:
    h.set_accumulate_mode(saved)
  frame = frame.cpu().numpy()
  return frame[:, 1:1 + 2 * case.dims], frame


def _sentinels_untouched(frame, width):
  return bool(np.all(frame[:, 0] == fe.SENTINEL) and np.all(frame[:, 1 + width:] == fe.SENTINEL))


# ---- FIR ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fe.FIR_CASES, ids=fe.fir_id)
def test_fir_exact_filling_is_bit_exact(dev, case):
  for kind in fe.exact_kinds(case.c * (case.pre + 1 + case.post)):
    data = fe.fir_exact(case, kind)
    got, frame = _run_fir(dev, case, data)
    want = fe.fir_exact_want(case, data)        # the sentinel where a recording defines no output
    differ = np.argwhere(got != want)
    assert differ.size == 0, (kind, len(differ), differ[:8].tolist(), got[tuple(differ[0])], want[tuple(differ[0])])
    assert _sentinels_untouched(frame, case.d), kind


@pytest.mark.parametrize('case', fe.FIR_CASES, ids=fe.fir_id)
def test_fir_real_filling_within_the_model_bound(dev, case):
  data, bound = fe.fir_real(case)
  got, frame = _run_fir(dev, case, data)
  dist = fe.fir_distance(case, data, got)
  print('%s: gpu_vs_ref64 %.3e  bound %.3e' % (fe.fir_id(case), dist, bound))
  parity_log.record('fir_edges ' + fe.fir_id(case), gpu_vs_ref64=dist, bound=bound)
  assert dist <= bound, (dist, bound)
  assert _sentinels_untouched(frame, case.d)


@pytest.mark.parametrize('case', fe.FIR_CASES, ids=fe.fir_id)
def test_fir_nonfinite_spoils_exactly_its_windows(dev, case):
  data = fe.fir_nonfinite(case)
  got, _ = _run_fir(dev, case, data)
  want = fe.fir_nonfinite_want(case, data)
  for q in range(case.d):
    differ = np.flatnonzero(~np.isfinite(got[:, q]) != want[:, q])
    assert differ.size == 0, (q, len(differ), differ[:16].tolist())


# ---- CCA ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fe.CCA_CASES, ids=fe.cca_id)
def test_cca_exact_filling_is_bit_exact(dev, case):
  """Each view's rows separately: with an offset a row exists in one view only, and the other half of it keeps the
  sentinel."""
  for kind in fe.cca_exact_kinds(case):
    data = fe.cca_exact(case, kind)
    got, frame = _run_cca(dev, case, data)
    want = fe.cca_exact_want(case, data)
    differ = np.argwhere(got != want)
    assert differ.size == 0, (kind, len(differ), differ[:8].tolist(), got[tuple(differ[0])], want[tuple(differ[0])])
    assert _sentinels_untouched(frame, 2 * case.dims), kind


@pytest.mark.parametrize('case', fe.CCA_CASES, ids=fe.cca_id)
def test_cca_real_filling_within_6e_7(dev, case):
  data = fe.cca_real(case)
  got, frame = _run_cca(dev, case, data)
  dist = fe.cca_distance(case, data, got)
  print('%s: gpu_vs_ref64 %.3e  bound %.3e' % (fe.cca_id(case), dist, fe.CCA_BOUND))
  parity_log.record('fir_edges ' + fe.cca_id(case), gpu_vs_ref64=dist, bound=fe.CCA_BOUND)
  assert dist <= fe.CCA_BOUND, dist
  assert _sentinels_untouched(frame, 2 * case.dims)


@pytest.mark.parametrize('case', fe.CCA_CASES, ids=fe.cca_id)
def test_cca_nonfinite_spoils_exactly_its_rows_of_its_view(dev, case):
  data = fe.cca_nonfinite(case)
  got, _ = _run_cca(dev, case, data)
  want = fe.cca_nonfinite_want(case, data)
  for q in range(2 * case.dims):
    differ = np.flatnonzero(~np.isfinite(got[:, q]) != want[:, q])
    assert differ.size == 0, (q, len(differ), differ[:16].tolist())
