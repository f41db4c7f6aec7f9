"""The tables and references of tests/window_edges.py are sound (no GPU): every window-sum case reaches the route it
is there for, the float64 references agree with long double and move by far more than the GPU bound under each of
three planted errors, the restated np_sum is np.sum bit for bit, the restated step recurrence is the oracle's, and
the state-space decoder is finite and well conditioned on every entry of its table."""
import numpy as np
import pytest

from oracle import attention as o_att
from tests import window_edges as we


# ---- routes ---------------------------------------------------------------------------------------------------------
def test_table_has_the_shapes_and_columns_of_its_plan():
  assert len(we.CASES) == len(set(we.CASES)) == 3 * 21 + 3 * 5 + 4 * 3
  for width, hop in we.BLOCK_SHAPES:
    assert sorted({c[0] for c in we.CASES if c[2:] == (width, hop)}) == we.BLOCK_COLS
  for width, hop in we.LONG_SHAPES + we.SHORT_SHAPES + we.PER_WINDOW_SHAPES:
    assert sorted({c[0] for c in we.CASES if c[2:] == (width, hop)}) == we.OTHER_COLS
  for cols, b_cols, width, hop in we.CASES:
    assert cols % b_cols == 0 and 1 <= b_cols <= cols
    if we.window_block_size(width, hop) == 0:
      assert b_cols == cols              # the cycled call is refused without a common block
    elif cols > 1:
      assert {c[1] for c in we.CASES if c[0] == cols and c[2:] == (width, hop)} == {cols, we.proper_divisor(cols)}
      assert we.proper_divisor(cols) < cols
  assert set(we.CONTIGUOUS_CASES) <= set(we.CASES)


@pytest.mark.parametrize('case', we.CASES, ids=we.case_id)
def test_case_reaches_its_route(case):
  cols, _, width, hop = case
  want = we.EXPECTED_ROUTE[(width, hop)]
  got = we.route(case)
  if isinstance(want, str):
    assert got == want
    assert np.gcd(width, hop) < 32 and (width <= 256) == (want == 'short')
  else:
    assert got[:2] == want
    assert got[2] == ('cols' if 8 <= cols <= 64 else 'lanes')
    assert got[3] == ('wide' if want[1] > 64 else 'narrow')
    assert width % got[0] == 0 and hop % got[0] == 0 and got[0] * got[1] == width
  # the trials: several windows, none, none, one, one
  offs = we.trial_offsets(case)
  counts = [len(we.o_cor.window_starts(int(n), width, hop)) for n in np.diff(offs)]
  assert counts == [4, 0, 0, 1, 1] and len(we.window_rows(case)) == 6


def test_table_covers_every_route_and_lane_layout():
  routes = [we.route(c) for c in we.CASES]
  assert {we.route_name(c) for c in we.CASES} == {'cols+narrow', 'lanes+narrow', 'lanes+wide', 'short', 'per_window'}
  assert {we.route_name(c) for c in we.CONTIGUOUS_CASES} == {we.route_name(c) for c in we.CASES}
  blocks = [r for r in routes if not isinstance(r, str)]
  assert {r[2] for r in blocks} == {'cols', 'lanes'}
  assert {r[3] for r in blocks} == {'narrow', 'wide'}
  assert {r[0] for r in blocks} == {32, 33, 100, 257}
  assert {64, 65} <= {r[1] for r in blocks}
  per = {we.rows_per_step(c[0]) for c, r in zip(we.CASES, routes) if not isinstance(r, str) and r[2] == 'cols'}
  assert {1, 3, 8} <= per
  # an odd g that neither the 16 lanes of a block nor `per` divides; idle lanes: 64 - per * cols
  assert 33 % we.BLOCK_LANES and 33 % we.rows_per_step(21) == 0 and 100 % we.rows_per_step(21)
  assert 64 - we.rows_per_step(33) * 33 == 31 and 64 - we.rows_per_step(21) * 21 == 1
  # both sides of every threshold of the dispatch
  assert {7, 8, 9, 63, 64, 65} <= {c[0] for c in we.CASES if not isinstance(we.route(c), str)}
  assert {256, 257} <= {c[2] for c in we.CASES if isinstance(we.route(c), str)}
  # the second search loop: no divisor of 257 in [32, 256]
  assert all(257 % dv for dv in range(32, 257)) and we.window_block_size(514, 257) == 257


def test_window_block_size_restates_the_search():
  """Against a plain search of the same rule."""
  for width, hop in [(1000, 100), (1000, 500), (400, 200), (6000, 6000), (120000, 120000), (65000, 32000),
                     (10, 5), (200, 77), (300, 7), (31 * 4096, 31 * 4096), (8192 * 3, 8192)] + list(we.EXPECTED_ROUTE):
    g = int(np.gcd(width, hop))
    small = [d for d in range(32, 257) if g % d == 0]
    large = [d for d in range(32, 4097) if g % d == 0]
    want = max(small) if small else (max(large) if large else 0)
    if want and width // want > 65536:
      want = 0
    assert we.window_block_size(width, hop) == want, (width, hop)


# ---- references -----------------------------------------------------------------------------------------------------
# the widest window of the table holds the most terms; a reference needs no more than one case per shape and a few
# column counts to show what it is sensitive to
REFERENCE_CASES = [c for c in we.CASES if c[0] in (7, 21, 65) and c[1] != 1]


@pytest.mark.parametrize('case', REFERENCE_CASES, ids=we.case_id)
def test_float64_reference_is_long_double_to_1e14(case):
  f64, ld, mag = we.window_references(case)
  assert f64.shape == ld.shape == mag.shape == (6, case[0], 5)
  assert np.all(np.abs(f64.astype(we.LD) - ld) <= 1e-14 * np.abs(ld))
  # and within the GPU bound's own allowance of it
  assert np.all(np.abs(f64.astype(we.LD) - ld) <= we.window_bound(case))
  assert np.all(mag[:, :, 2:4] == f64[:, :, 2:4]) and np.all(mag >= np.abs(f64))


@pytest.mark.parametrize('case', REFERENCE_CASES, ids=we.case_id)
def test_planted_errors_move_the_sums_past_the_gpu_bound(case):
  """A window that loses its last frame, a column paired with its neighbour in b, a window that reads one row too
  many: each moves at least one sum of at least one window by more than the bound the GPU test allows."""
  a, b = we.window_data(case)
  starts, width = we.window_rows(case), case[2]
  want, bound = we.window_references(case)[0], we.window_bound(case)
  for w in range(len(starts)):
    got = we.five_sums(a, b, starts, width, drop_last_of=w)
    assert np.any(np.abs(got[w] - want[w]) > bound[w]) and np.array_equal(np.delete(got, w, 0), np.delete(want, w, 0))
    # every column of that window notices
    assert np.all(np.any(np.abs(got[w] - want[w]) > bound[w], axis=1))
  if b.shape[1] > 1:
    got = we.five_sums(a, b, starts, width, pair_shift=1)
    assert np.all(np.any(np.abs(got - want) > bound, axis=2))
  got = we.five_sums(a, b, starts[:-1], width, extra_rows=1)       # (the last window ends with the data)
  assert np.all(np.any(np.abs(got - want[:-1]) > bound[:-1], axis=2))


@pytest.mark.parametrize('case', we.CASES, ids=we.case_id)
def test_restated_order_of_summation_is_a_float64_sum(case):
  """The kernels' order followed on the host is one more order of the same exact terms: within the allowance of
  the float64 reference, on every window, column and sum."""
  got, (want, _, _) = we.device_order_sums(case), we.window_references(case)
  assert got.shape == want.shape
  assert np.all(np.abs(got - want) <= we.window_bound(case))


def test_restated_orders_differ_in_bits_across_each_threshold():
  """What a dispatch with an off-by-one threshold would deliver is right to the allowance and wrong in bits: the
  other block kernel at 8 and 64 columns, the other window kernel at 64 and 65 blocks, the other no-common-block
  kernel at 256 and 257 frames.  So the GPU test's bit comparison sees which kernel ran."""
  for case in ((8, 8, 96, 32), (64, 64, 96, 32), (64, 1, 200, 100), (7, 7, 2048, 32), (65, 13, 2080, 32)):
    g, per_win, block, window = we.route(case)
    mine = we.device_order_sums(case)
    # (the block kernels at the column thresholds, the window kernels at the block-count thresholds)
    if per_win < 64:
      other = we.device_order_sums(case, (g, per_win, 'lanes' if block == 'cols' else 'cols', window))
    else:
      other = we.device_order_sums(case, (g, per_win, block, 'wide' if window == 'narrow' else 'narrow'))
    assert np.all(np.abs(other - mine) <= we.window_bound(case))
    assert np.sum(other != mine) >= 10, case
  for case, other in (((65, 65, 256, 7), 'per_window'), ((65, 65, 257, 7), 'short')):
    assert np.sum(we.device_order_sums(case, other) != we.device_order_sums(case)) >= 10, case


# ---- np_sum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', range(1, we.MAX_KW + 1))
def test_np_sum_restated_is_numpy_bit_for_bit(n):
  rng = np.random.default_rng(n)
  for scale in (1.0, 1e8):
    for _ in range(50):
      v = rng.standard_normal(n) * scale ** rng.uniform(-1, 1, n)
      assert we.np_sum(v) == np.sum(v), (n, v)
  # the routine's branches: plain below 8, no tail at a multiple of 8
  assert (n < 8) == (n in range(1, 8)) and (n % 8 == 0) == (n in (8, 16, 24, 32))


def test_the_lag_table_reaches_every_branch_of_np_sum():
  kws = sorted({k_f + k_b + 1 for k_f, k_b in we.LAGS})
  assert kws == [1, 2, 7, 8, 9, 15, 16, 17, 32]
  assert max(kws) == we.MAX_KW and any(k_f > 0 for k_f, _ in we.LAGS)
  assert len(we.SSD_CASES) == 33
  for lags in (we.BATCH_LAGS, we.STREAM_LAGS, [we.WRAPPER_LAGS]):
    assert set(lags) <= set(we.LAGS)


# ---- the step decoder -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_trials', we.STEP_TRIALS)
def test_step_recurrence_is_the_oracles(n_trials):
  s1, s2, wo, states = we.step_inputs(n_trials)
  counts = np.diff(wo)
  assert len(counts) == n_trials and wo[-1] == len(s1) == len(s2)
  if n_trials >= 3:
    assert 0 in counts[1:-1] and 1 in counts and np.any(s1 == s2)
    assert set(states) == set(we.STEP_STATES)
  for t in range(n_trials):
    r = slice(wo[t], wo[t + 1])
    want, want_state = o_att.step_sequence(s1[r], s2[r], state=states[t])
    got, got_state = we.step_recurrence(s1[r], s2[r], states[t])
    np.testing.assert_array_equal(got, want)
    assert got_state == want_state


def test_wta_inputs_hold_their_planted_cases():
  n = 2048 * 256 + 1
  s1, s2 = we.wta_inputs(n)
  both = ~np.isnan(s1) & ~np.isnan(s2)
  assert np.sum(both & (s1 == s2) & (s1 != 0)) > 900
  assert np.sum((s1 == 0) & (s2 == 0) & np.signbit(s1) & ~np.signbit(s2)) > 900
  assert np.sum((s1 == 0) & (s2 == 0) & ~np.signbit(s1) & np.signbit(s2)) > 900
  assert np.sum(np.isnan(s1) & ~np.isnan(s2)) > 900 and np.sum(~np.isnan(s1) & np.isnan(s2)) > 900
  assert np.sum(np.isnan(s1) & np.isnan(s2)) > 900
  with np.errstate(invalid='ignore'):
    want = s1 > s2
  assert not want[~both].any() and 0.4 < want.mean() < 0.6


# ---- column strides -------------------------------------------------------------------------------------------------
def test_wrappers_refuse_a_column_stride_before_any_device_call():
  """window_sums, frame_scores and window_class_moments hand the kernels a row stride only: a transposed or
  column-strided view is refused, before a handle is asked for (so this runs without a GPU)."""
  import torch
  from telluride_decoding_amd import device
  good = torch.zeros((6, 3), dtype=torch.float32)
  transposed = torch.zeros((3, 6), dtype=torch.float32).t()
  strided = torch.zeros((6, 6), dtype=torch.float32)[:, ::2]
  assert transposed.shape == strided.shape == good.shape and transposed.stride(1) == 6 and strided.stride(1) == 2
  stats = (np.zeros(3), np.zeros(3), np.ones(3))
  for bad in (transposed, strided):
    for a, b in ((bad, good), (good, bad)):
      with pytest.raises(ValueError, match='columns of %s must be contiguous' % ('a' if a is bad else 'b')):
        device.window_sums(a, b, [0, 6], 2, 2)
      with pytest.raises(ValueError, match='columns of %s must be contiguous' % ('a' if a is bad else 'b')):
        device.frame_scores(a, b, 'mean', *stats)
      with pytest.raises(ValueError, match='columns of %s must be contiguous' % ('a' if a is bad else 'b')):
        device.window_class_moments(a, b, 2, *stats)
  with pytest.raises(ValueError, match='two dimensions'):
    device.window_sums(good[:, 0], good[:, 0], [0, 6], 2, 2)


# ---- the state-space decoder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', we.SSD_CASES, ids=we.ssd_id)
def test_state_space_oracle_is_finite_and_well_conditioned(case):
  """No overflow, underflow, division by zero or invalid operation anywhere on the table, and inputs a few ulps
  away (one ulp of r2, 2^-52 relative of r1) give the same trajectory to 1e-10: three decades inside the 1e-7 at
  which the device is compared, so a device libm that rounds differently cannot be what a failure there shows."""
  c = we.ssd_stream(case[0], case[1])
  with np.errstate(all='raise'):
    traj = we.ssd_oracle(case)
    moved = we.ssd_oracle(case, np.stack((c[:, 0] * (1 + we.EPS), np.nextafter(c[:, 1], np.inf)), axis=1))
  assert np.all(np.isfinite(traj)) and np.all((traj > 0) & (traj < 1))
  assert np.all(traj[:, 1] >= traj[:, 0]) and np.all(traj[:, 0] >= traj[:, 2])
  np.testing.assert_allclose(moved, traj, rtol=1e-10, atol=0)


def test_batch_streams_are_distinct_and_of_their_lengths():
  for k_f, k_b in we.BATCH_LAGS:
    streams = we.batch_streams(k_f, k_b)
    kw = k_f + k_b + 1
    assert [len(s) for s in streams] == [0, 1, kw - 1, kw, 40]
    heads = [tuple(s[0]) for s in streams if len(s)]
    assert len(set(heads)) == len(heads)
