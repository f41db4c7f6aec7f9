"""The case tables of tests/shrink_edges.py without a GPU: what the bound of tests/test_gpu_shrink_edges.py rests on.
The float64 loop the device is compared with is itself within 1e-14 of long double, and the reference's own float32
arithmetic within a quarter of the device's bound of 2e-6; one wrong edge sample, or one piece of a minibatch's column
sums added twice, moves the result by far more than that bound; and the route arithmetic of td_shrinkage_moment,
restated in shrink_edges.route, shows that the tables reach what they claim to."""
import numpy as np
import pytest

from tests import shrink_edges as se

GPU_BOUND = 2e-6            # of tests/test_gpu_shrink_edges.py and tests/test_gpu_fit.py


def _rel(a, b):
  return float(abs(a - b) / abs(b))


# ---- (a) the references --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', se.CASES, ids=se.case_id)
def test_references_are_accurate_enough_for_the_bound(case):
  f64, ld, f32 = se.references(case)
  assert f64 > 0.0
  assert _rel(se.LD(f64), ld) <= 1e-14
  assert _rel(f32, f64) <= 5e-7                   # a quarter of GPU_BOUND (observed: at most 2.4e-7, c = 104, 32 lags)


def test_float64_loop_is_the_one_of_the_fit_suite():
  from tests.test_gpu_fit import _lw_moment_numpy
  for case in (se.A1, se.B2):
    b = se.minibatches(case)
    assert se._lw_moment_numpy(b) == _lw_moment_numpy(b) == se.references(case)[0]


def test_layout_of_a_known_case():
  """(8, 0, 5, -3): the offset drops three rows of the targets, so the recording of two rows adds nothing, and the
  rows of x behind the last lagged row of a recording exist (no zero padding there before frame 150)."""
  rows, total, used = se.layout(se.GROUP_A[3] + (True,))
  assert rows == [147, 0, 128] and total == 256 and used == [147, 0, 109]
  rows, total, used = se.layout(se.GROUP_A[3] + (False,))
  assert total == 275 and used is None
  assert se.pieces(se.GROUP_A[3] + (False,))[2] == [(128, 19), (147, 45)]
  assert [b.shape[0] for b in se.minibatches(se.GROUP_A[3] + (False,))] == [64, 64, 64, 64, 19]
  # a minibatch over three recordings, the second shorter than the context
  assert se.pieces(se.A1)[2] == [(32, 8), (40, 7), (47, 1)]


# ---- (b) a wrong edge or a doubled piece is far outside the bound --------------------------------------------------
@pytest.mark.parametrize('case', [c for c in se.CASES_A if c[1] + c[2] > 0], ids=se.case_id)
def test_one_wrong_edge_sample_is_visible(case):
  f64 = se.references(case)[0]
  moved = _rel(se.edge_planted(case), f64)
  assert moved >= 1e-5                            # (observed: at least 3.9e-5)
  assert moved >= 5 * GPU_BOUND


def test_cases_without_context_have_no_edge():
  flat = [c for c in se.CASES_A if c[1] + c[2] == 0]
  assert len(flat) == 2 and all(se.edge_planted(c) is None for c in flat)


@pytest.mark.parametrize('case', se.CASES_B, ids=se.case_id)
def test_a_piece_added_twice_is_visible(case):
  f64 = se.references(case)[0]
  planted = se.race_planted(case)
  assert planted is not None
  assert _rel(planted, f64) >= 1e-4               # (observed: at least 2.0e-3)


# ---- (c) what the tables reach -------------------------------------------------------------------------------------
def test_route_restatement_on_known_shapes():
  r = se.route((64, 0, 31, 0, (3000, 2500), 500, True))          # the decoding shape of tests/test_gpu_fit.py
  assert r['tiled'] and r['lds'] == 4 * (159 * 68 + 256) and r['k'] == 2048 and r['chunks'] == 4
  assert r['spanning'] == 0 and r['batches'] == 11               # its minibatches never span: 3000 = 6 * 500
  r = se.route((70, 0, 0, 0, (1000,), 300, False))
  assert not r['tiled'] and r['passes'] == 2 and r['short_last'] and r['chunks'] == 10
  assert se.route(se.CASES_B[5])['lds'] == se.LARGEST_TILE <= 65536 < se.FIRST_TOO_LARGE == se.route(se.CASES_B[6])['lds']


def test_tables_reach_every_edge():
  routes = [(c, se.route(c)) for c in se.CASES]
  tiled = [(c, r) for c, r in routes if r['tiled']]
  wave = [(c, r) for c, r in routes if not r['tiled']]
  assert tiled and wave
  # odd lag counts (uneven halves) and a single lag (an empty half) on the tiled route
  assert {1, 3, 5} <= {r['lags'] for _, r in tiled}
  # more than 64 channels (two passes of the column sums) on both routes
  assert any(c[0] > 64 and r['passes'] == 2 for c, r in tiled) and any(c[0] > 64 and r['passes'] == 2 for c, r in wave)
  # the largest tile that fits and the first that does not, which takes the wave route with c % 4 == 0
  assert any(r['lds'] == se.LARGEST_TILE for _, r in tiled)
  assert any(r['lds'] == se.FIRST_TOO_LARGE and c[0] % 4 == 0 for c, r in wave)
  # a shorter last minibatch on both routes, and whole minibatches only (rows_used) on both
  assert any(r['short_last'] for _, r in tiled) and any(r['short_last'] for _, r in wave)
  assert any(c[6] and not r['short_last'] for c, r in tiled) and any(c[6] and not r['short_last'] for c, r in wave)
  # tiles that cross into another recording and tiles that do not, inside one call
  assert any(r['tiles_crossing'] and r['tiles_plain'] for _, r in tiled)
  # a tile of fewer than 128 rows after a full one (a minibatch of 256 rows, 1200 = 4 * 256 + 176)
  assert any(r['chunks'] == 2 and r['total'] % c[5] not in (0, 128) for c, r in tiled)
  # a minibatch over three recordings, on both routes
  assert any(r['most_pieces'] == 3 for _, r in tiled) and any(r['most_pieces'] == 3 for _, r in wave)
  # both signs of input_offset on the tiled route
  assert any(c[3] > 0 for c, _ in tiled) and any(c[3] < 0 for c, _ in tiled)
  # an empty recording, and recordings shorter than the minibatch, the context and the offset
  cases = [c for c, _ in routes]
  assert any(0 in c[4] for c in cases)
  assert any(0 < min(c[4]) < c[5] for c in cases)
  assert any(0 < min(n for n in c[4] if n) < c[1] + c[2] for c in cases)
  assert any(0 < min(n for n in c[4] if n) < abs(c[3]) for c in cases)
  # Group B: K > 256, every case with a minibatch that spans recordings and a shorter last one
  for c in se.CASES_B:
    r = se.route(c)
    assert r['k'] > 256 and r['spanning'] >= 1 and r['short_last'], c
  assert max(sum(c[4]) * c[0] for c in cases) == 1200 * 104            # the largest input
  # the views: cases of the tiled route (only it stages with 16-byte loads), one per group at least
  assert all(se.route(c)['tiled'] for c in se.VIEW_CASES)


def test_algebra_sizes_stride_both_grids():
  n = np.array(se.ALGEBRA_N)
  assert ((n + 1) ** 2 > 1024 * 256).sum() >= 2 and (n ** 2 <= 1024 * 256).sum() >= 6     # td_shrinkage_terms
  assert (n ** 2 > 4096 * 256).sum() == 1 and 1100 ** 2 > 4096 * 256                     # td_shrunk_covariance
  assert {255, 256, 257} <= set(se.ALGEBRA_N)
  s = se.moments_like(16)
  assert s.shape == (17, 17) and np.array_equal(s, s.T) and s[16, 16] == se.FRAMES
  tr, sq, tol_tr, tol_sq = se.terms_reference(s, 16, 16)
  zc = s[:16, :16] - np.outer(s[16, :16], s[16, :16]) / se.FRAMES ** 2
  assert abs(float(tr) - np.trace(zc)) <= tol_tr and abs(float(sq) - (zc ** 2).sum()) <= tol_sq
  assert 0 < tol_tr < 1e-10 * abs(float(tr)) and 0 < tol_sq < 1e-10 * float(sq)
