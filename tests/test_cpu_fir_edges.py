"""What tests/test_gpu_fir_edges.py rests on, checked without a GPU: the restated launch ladder of td_launch_fir and
td_cca_transform against the source's constants, every case of tests/fir_edges.py on the route it names, the tables'
reach, the exact filling's 2^23 condition, the cap of the real tier's bound, and that each tier can see a wrong kernel."""
import numpy as np
import pytest

from tests import fir_edges as fe


def test_restated_constants_equal_the_source():
  assert fe.restated_constants() == fe.source_constants()


@pytest.mark.parametrize('case', fe.FIR_CASES, ids=fe.fir_id)
def test_every_fir_case_reaches_its_route(case):
  route = fe.fir_case_route(case)
  assert (route.name, route.detail) == (case.route, case.detail)
  assert max(case.lens) <= fe.MAX_ROWS
  if case.pad % 4 == 0 and case.c % 4 == 0:     # a pad of four keeps the route
    assert route == fe.fir_route(case.c, case.pre, case.post, case.d, case.c, True, case.per_file)


@pytest.mark.parametrize('case', fe.CCA_CASES, ids=fe.cca_id)
def test_every_cca_case_reaches_its_route(case):
  route = fe.cca_case_route(case)
  assert (route.name, route.detail) == (case.route, case.detail)
  assert max(case.lens) <= fe.MAX_ROWS


def test_ladder_thresholds():
  """The edges of the ladder itself: 32 / 33 outputs of the projection, 64 / 65 lags of the streamed kernel, 96 / 97 lags
  of the matrix-core kernel's 80 KB, 8192 / 8193 floats of row pitch, the second CCA view at 8 / 12 and 32 / 36."""
  assert fe.fir_route(8, 0, 0, 32, 8).name == 'project4' and fe.fir_route(8, 0, 0, 33, 8).name == 'mfma'
  assert fe.fir_route(64, 0, 63, 1, 64).name == 'stream' and fe.fir_route(64, 0, 64, 1, 64).name == 'mfma'
  assert fe.fir_route(64, 0, 95, 2, 64).name == 'mfma' and fe.fir_route(64, 0, 96, 2, 64).name == 'valu'
  assert fe.mfma_plan(64, 96, 1)[4] <= fe.FIR_LDS_MAX < fe.mfma_plan(64, 97, 1)[4]
  assert fe.fir_route(63, 0, 31, 1, 8192).name == 'stream' and fe.fir_route(63, 0, 31, 1, 8193).name == 'wave32x1'
  assert fe.fir_route(64, 0, 31, 3, 64, base_aligned=False).name == 'wave32x2'
  assert fe.cca_route(64, 0, 0, 8, 0, 0, 8, 64, 8).name == 'cca_stream'
  assert fe.cca_route(64, 0, 0, 12, 0, 0, 8, 64, 12).name == 'cca_project108'
  assert fe.cca_route(64, 0, 0, 8, 0, 0, 8, 1 << 20, 8).name == 'cca_project76'
  assert fe.cca_route(64, 0, 0, 36, 0, 0, 8, 64, 36).name == 'fallback'
  assert fe.cca_route(64, 0, 0, 12, 0, 0, 9, 64, 12).name == 'fallback'
  assert fe.cca_route(64, 0, 0, 12, 0, 0, 8, 64, 12, mode='f32').name == 'fallback'


def test_small_calls_get_the_restated_strips():
  rows = sum(fe.R128)
  assert fe.strip_rows('project8', rows) == 128 and fe.strip_rows('mfma', rows) == 128
  assert fe.strip_rows('wave32x2', rows) == 256 and fe.strip_rows('wave32x1', rows) == 256
  assert fe.strip_rows('wave4x8', rows) == 128 and fe.strip_rows('valu', rows) == 256
  assert fe.strip_rows('cca_project108', rows) == 128
  # every recording set crosses the strip of the kernels it is used for, by one row on either side
  for lens, strip in ((fe.R128, 128), (fe.R256, 256), (fe.RCCA, 128)):
    assert {strip - 1, strip, strip + 1} - {n - 1 for n in lens} - set(lens) - {n + 1 for n in lens} == set()
    assert 0 in lens[1:-1] and max(lens) > 2 * strip
  for case in fe.FIR_CASES:
    if case.lens in (fe.R128, fe.R256):
      assert fe.strip_rows(fe.fir_case_route(case), sum(case.lens)) == (128 if case.lens == fe.R128 else 256), case


def test_tables_reach_every_route_and_edge():
  reached = set().union(*(fe.fir_edges(case) for case in fe.FIR_CASES))
  assert fe.REQUIRED_FIR_EDGES - reached == set()
  reached = set().union(*(fe.cca_edges(case) for case in fe.CCA_CASES))
  assert fe.REQUIRED_CCA_EDGES - reached == set()
  assert 90 <= len(fe.FIR_CASES) + len(fe.CCA_CASES) <= 120
  assert len(set(map(fe.fir_id, fe.FIR_CASES))) == len(fe.FIR_CASES)
  assert len(set(map(fe.cca_id, fe.CCA_CASES))) == len(fe.CCA_CASES)


def _three_pieces_live(values):
  _, _, low = fe.bf16_pieces(values)
  return bool(np.any(low != 0))


@pytest.mark.parametrize('case', fe.FIR_CASES, ids=fe.fir_id)
def test_exact_filling_meets_its_condition(case):
  k = case.c * (case.pre + 1 + case.post)
  for kind in fe.exact_kinds(k):
    data = fe.fir_exact(case, kind)
    for v in data:
      assert np.array_equal(v, np.round(v))
    assert fe.fir_exact_sizes(case, kind) <= fe.EXACT_LIMIT
    want, _, defined = fe.fir_reference(case, data)
    assert np.array_equal(want[defined].astype(np.float32).astype(np.float64), want[defined])
  # the narrow operand is one bf16 piece; the wide one has all three wherever a window-spaced sample fits a recording
  assert np.max(np.abs(fe.fir_exact(case, 'wide_x').w)) <= 7 and np.max(np.abs(fe.fir_exact(case, 'wide_w').x)) <= 7
  assert _three_pieces_live(fe.fir_exact(case, 'wide_w').w)
  if max(case.lens) >= 128:
    assert _three_pieces_live(fe.fir_exact(case, 'wide_x').x)
  if k <= 16:
    h, m, low = fe.bf16_pieces(fe.fir_exact(case, 'mid_mid').x)
    assert np.any(m != 0) and not np.any(low != 0)


@pytest.mark.parametrize('case', fe.CCA_CASES, ids=fe.cca_id)
def test_cca_exact_filling_meets_its_condition(case):
  for kind in fe.cca_exact_kinds(case):
    data = fe.cca_exact(case, kind)
    want, size, defined = fe.cca_reference(case, data)
    assert size[defined].max() <= fe.EXACT_LIMIT
    assert np.array_equal(want[defined].astype(np.float32).astype(np.float64), want[defined])
  # a row exists in one view and not in the other wherever the offset is not zero
  _, _, defined = fe.cca_reference(case, fe.cca_exact(case, 'wide_x'))
  assert (case.off == 0) == bool(np.all(defined[:, 0] == defined[:, -1]))


@pytest.mark.parametrize('case', fe.FIR_CASES, ids=fe.fir_id)
def test_real_bound_is_under_its_cap_and_the_tiers_see_wrong_kernels(case):
  data, bound = fe.fir_real(case)
  assert fe.REAL_FLOOR <= bound <= fe.REAL_CAP
  assert fe.fir_distance(case, data, fe.fir_chain_model(case, data)) <= bound / 2 or bound == fe.REAL_FLOOR
  k = case.c * (case.pre + 1 + case.post)
  for model in fe.WRONG_MODELS:
    if not fe.wrong_applies(case, model):
      continue
    seen = fe.fir_distance(case, data, fe.fir_wrong(case, data, model)) > bound
    for kind in fe.exact_kinds(k):
      exact = fe.fir_exact(case, kind)
      seen = seen or not np.array_equal(fe.fir_wrong(case, exact, model), fe.fir_exact_want(case, exact))
    assert seen, model


def test_every_wrong_model_has_cases():
  for model in fe.WRONG_MODELS:
    assert sum(fe.wrong_applies(case, model) for case in fe.FIR_CASES) >= 3, model


@pytest.mark.parametrize('case', [c for c in fe.FIR_CASES if c.lens in (fe.R128, fe.R256)][::6], ids=fe.fir_id)
def test_nonfinite_filling_leaves_finite_outputs_beside_its_windows(case):
  """The non-finite tier can only see a spread if outputs next to a spoiled window are finite: in the longest recording
  the outputs NL - nl frames in front of the strip-edge pair's window, and `ring` frames behind it, must be."""
  data = fe.fir_nonfinite(case)
  bad = fe.fir_nonfinite_want(case, data)
  assert bad.any() and not bad.all()
  strip = fe.strip_rows(fe.fir_case_route(case))
  o0 = int(np.sum(case.lens[:-1]))
  first = o0 + strip - 1 - case.post            # (stream rows: the offset moved the samples with it)
  assert bad[first, 0] and not bad[first - 1, 0]
  assert not bad[o0 + strip + case.pre + 1, 0]
