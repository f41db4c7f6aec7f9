"""The window, score and decision kernels of csrc/windows.hip on the MI355X at their edges (the cases of
tests/window_edges.py, which tests/test_cpu_window_edges.py shows to reach them and to be sensitive enough): every
route of td_window_sums_cycled on every window, column and sum against float64 within the allowance of a float64
sum in any order; window scores, frame scores and window means against the same expressions in float64; the
winner-take-all and step decisions bit for bit, past the caps of their grids and past one workgroup of trials; the
state-space decoder at kw from 1 to 32, with forward lags, other iteration counts, more than 64 trials in a launch
and carried state, against the oracle and the reference's own trajectories (tests/golden/g7b_decoder_lags.npz)."""
import numpy as np
import pytest

from oracle import attention as o_att
from oracle import correlator as o_cor
from oracle import pearson as o_p
from tests import parity_log
from tests import window_edges as we
from tests.conftest import golden

pytestmark = pytest.mark.gpu

EPS = we.EPS
_WORST = {}                # family -> (largest error as a fraction of its allowance, where)


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


@pytest.fixture(scope='module', autouse=True)
def _record_worst():
  yield
  for family, (ratio, where) in sorted(_WORST.items()):
    parity_log.record('window_edge_worst', family=family, worst_fraction_of_allowance=ratio, where=where)


def _note(family, ratio, where):
  if family not in _WORST or ratio > _WORST[family][0]:
    _WORST[family] = (float(ratio), where)


def _d64(h, v):
  return h.to_device(np.asarray(v, np.float64).reshape(-1, 1), np.float64).reshape(-1)


def _slice_of_wider(h, x, seed=11):
  """x as columns [1, 1 + cols) of a device tensor 3 columns wider: a row stride that is not the column count and
  a base 4 bytes off 16-byte alignment."""
  rows, cols = x.shape
  wide = np.random.default_rng(seed).standard_normal((rows, cols + we.EXTRA_COLS)).astype(np.float32)
  wide[:, we.FIRST_COL:we.FIRST_COL + cols] = x
  wd = h.to_device(wide)
  xd = wd[:, we.FIRST_COL:we.FIRST_COL + cols]
  assert xd.stride(0) == cols + we.EXTRA_COLS and xd.stride(1) == 1
  assert xd.data_ptr() == wd.data_ptr() + 4 * we.FIRST_COL and xd.data_ptr() % 16 == 4
  return xd


# ---- 1. window sums -------------------------------------------------------------------------------------------------
def _check_window_sums(dev, case, contiguous):
  h = dev.default_handle()
  a, b = we.window_data(case)
  ad, bd = (h.to_device(a), h.to_device(b)) if contiguous else (_slice_of_wider(h, a), _slice_of_wider(h, b, 12))
  width, hop = case[2], case[3]
  got = dev.window_sums(ad, bd, we.trial_offsets(case), width, hop, handle=h).cpu().numpy()
  want, _, _ = we.window_references(case)
  bound = we.window_bound(case)
  assert got.shape == want.shape and got.shape[0] == len(we.window_rows(case)) == 6
  ratio = float(np.max(np.abs(got - want) / bound))
  where = we.case_id(case) + ('-dense' if contiguous else '')
  print('window sums %s route %s: worst error %.3g of the allowance' % (where, we.route(case), ratio))
  parity_log.record('window_edge_sums', where=where, route=we.route_name(case), worst_fraction_of_allowance=ratio)
  _note('window_sums', ratio, where)
  bad = np.argwhere(~(np.abs(got - want) <= bound))
  assert bad.size == 0, (where, we.route(case), bad[:10].tolist(), ratio)
  # the kernels' sums have a fixed order; followed on the host it gives the device's bits -- and another kernel's
  # order does not (tests/test_cpu_window_edges.py), so this is also the check of WHICH kernel the dispatch chose
  order = we.device_order_sums(case)
  differs = np.argwhere(got != order)
  assert differs.size == 0, (where, we.route(case), 'not the bits of the route', differs[:10].tolist())


@pytest.mark.parametrize('case', we.CASES, ids=we.case_id)
def test_window_sums_every_window_column_and_sum(dev, case):
  """On column slices of wider tensors: every window, every column, all five sums within width 2^-52 sum |term|
  of float64 (a dropped frame, a wrong pairing or a row too many are thousands of allowances:
  tests/test_cpu_window_edges.py), and the bits of the route's own order of summation."""
  _check_window_sums(dev, case, False)


@pytest.mark.parametrize('case', we.CONTIGUOUS_CASES, ids=we.case_id)
def test_window_sums_on_contiguous_tensors(dev, case):
  """One case per route on dense tensors, and the bits of the strided call: the same values in the same order."""
  _check_window_sums(dev, case, True)
  h = dev.default_handle()
  a, b = we.window_data(case)
  offs = we.trial_offsets(case)
  dense = dev.window_sums(h.to_device(a), h.to_device(b), offs, case[2], case[3], handle=h).cpu().numpy()
  sliced = dev.window_sums(_slice_of_wider(h, a), _slice_of_wider(h, b, 12), offs, case[2], case[3],
                           handle=h).cpu().numpy()
  np.testing.assert_array_equal(dense, sliced)


# ---- 2. window scores -----------------------------------------------------------------------------------------------
SCORE_SHAPE = (200, 100)            # width, hop of the score tests (the block route, g = 100)


@pytest.mark.parametrize('cols', [1, 2, 5, 70])
def test_window_scores_mode0_every_reduction(dev, cols):
  """Global-statistics scores from the device's sums, per-column means and powers, against the float64 formula
  from the reference sums."""
  h = dev.default_handle()
  width, hop = SCORE_SHAPE
  case = (cols, cols, width, hop)
  a, b = we.window_data(case)
  rng = np.random.default_rng(50 + cols)
  b = (0.6 * a + b).astype(np.float32)
  offs, starts = we.trial_offsets(case), we.window_rows(case)
  sums = dev.window_sums(h.to_device(a), h.to_device(b), offs, width, hop, handle=h)
  assert sums.shape[0] == len(starts)
  ref = we.five_sums(a, b, starts, width)
  mean_a = 0.5 + 0.1 * rng.standard_normal(cols)
  mean_b = 0.8 + 0.1 * rng.standard_normal(cols)
  power = 1.0 + rng.uniform(0, 1, cols)
  n = float(width)
  per_col = (ref[:, :, 4] - mean_a * ref[:, :, 1] - mean_b * ref[:, :, 0] + n * mean_a * mean_b) / (power * n)
  for red in ('first', 'second', 'mean'):
    if red == 'second' and cols < 2:
      with pytest.raises(ValueError, match='second'):
        dev.window_scores(sums, width, 0, red, mean_a, mean_b, power, handle=h)
      continue
    got = dev.window_scores(sums, width, 0, red, mean_a, mean_b, power, handle=h).cpu().numpy()
    want = o_cor.reduce_correlations(per_col, red)
    err = float(np.max(np.abs(got - want) / (1e-12 + 1e-9 * np.abs(want))))
    parity_log.record('window_edge_scores_mode0', cols=cols, reduction=red, worst_fraction_of_allowance=err)
    _note('window_scores_mode0', err, 'c%d-%s' % (cols, red))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)


CONSTANTS = (0.0, 1.25, -3e4, 1e-30)


@pytest.mark.parametrize('group', [1, 3, 4, 12])
def test_window_pearson_zero_rule_at_awkward_constants(dev, group):
  """12 columns as models of `group` outputs.  Window k of the first 8 has ONE constant column (in a for k < 4,
  in b after), at 0, 1.25, -3e4 (whose raw sum of squares leaves a rounding residue of either sign) and 1e-30:
  exactly that column's group is zero.  The ninth window has none.  Column 7 of a rides on a DC of 10 with a
  relative deviation of 1e-3 throughout: zero only where its group holds a constant column, else the oracle's
  Pearson to 1e-9."""
  h = dev.default_handle()
  cols, width, n_win = 12, 200, 9
  rng = np.random.default_rng(60)
  a = (rng.standard_normal((n_win * width, cols)) + 0.5).astype(np.float32)
  b = (0.6 * a + rng.standard_normal(a.shape)).astype(np.float32)
  a[:, 7] = (10.0 * (1.0 + 1e-3 * rng.standard_normal(n_win * width))).astype(np.float32)
  planted = [2, 5, 9, 11, 0, 4, 8, 10, -1]     # the constant column of window k (never column 7; the last: none)
  for k in range(n_win - 1):
    (a if k < 4 else b)[k * width:(k + 1) * width, planted[k]] = np.float32(CONSTANTS[k % 4])
  sums = dev.window_sums(h.to_device(a), h.to_device(b), [0, n_win * width], width, width, handle=h)
  got = dev.window_scores(sums, width, 1, handle=h, group=group).cpu().numpy()
  assert got.shape == (n_win, cols)
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  worst = 0.0
  for k in range(n_win):
    r = slice(k * width, (k + 1) * width)
    for g0 in range(0, cols, group):
      c = slice(g0, g0 + group)
      if g0 <= planted[k] < g0 + group:
        assert np.all(got[k, c] == 0.0), (k, g0, CONSTANTS[k % 4], got[k, c])
        continue
      assert np.all(got[k, c] != 0.0), (k, g0, got[k, c])
      want = o_p.pearson_correlation(a64[r, c], b64[r, c])
      assert want.shape == (group,)
      worst = max(worst, float(np.max(np.abs(got[k, c] - want) / (1e-9 * np.abs(want)))))
      np.testing.assert_allclose(got[k, c], want, rtol=1e-9, atol=1e-12)
      if g0 <= 7 < g0 + group:
        np.testing.assert_allclose(got[k, 7], want[7 - g0], rtol=1e-9, atol=0)
  parity_log.record('window_edge_pearson', group=group, worst_fraction_of_rtol=worst)
  _note('window_pearson', worst, 'group %d' % group)


# ---- 3. frame scores ------------------------------------------------------------------------------------------------
def _frame_reference(a, b, red, ma, mb, pw, lw, slope, icpt):
  """(the value, the sum of the absolute values of the terms entering it) in float64 NumPy."""
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  v = (a64 - ma) * (b64 - mb) / pw
  mag = (np.abs(a64) + np.abs(ma)) * (np.abs(b64) + np.abs(mb)) / np.abs(pw)
  cols = a.shape[1]
  if red == 'all':
    return v, mag
  if red in ('first', 'second'):
    c = 0 if red == 'first' else 1
    return v[:, c], mag[:, c]
  if red == 'mean':
    return v.sum(axis=1) / cols, mag.sum(axis=1) / cols
  if red == 'mean-squared':
    return (np.sign(v) * v * v).sum(axis=1) / cols, (mag * mag).sum(axis=1) / cols
  return slope * (v * lw).sum(axis=1) + icpt, np.abs(slope) * (mag * np.abs(lw)).sum(axis=1) + np.abs(icpt)


def _frame_stats(cols):
  rng = np.random.default_rng(80 + cols)
  return (0.5 + 0.1 * rng.standard_normal(cols), 0.8 + 0.1 * rng.standard_normal(cols),
          1.0 + rng.uniform(0, 1, cols), rng.standard_normal(cols), -1.7, 0.35)


@pytest.mark.parametrize('cols', [1, 2, 3, 33])
def test_frame_scores_every_reduction_against_float64(dev, cols):
  """All six reductions on column slices of wider tensors, lda with weights, slope and intercept, within
  (cols + 4) 2^-52 of the sum of the absolute values of the terms."""
  h = dev.default_handle()
  rows = 777
  rng = np.random.default_rng(70 + cols)
  a = (rng.standard_normal((rows, cols)) + 0.5).astype(np.float32)
  b = (0.6 * a + rng.standard_normal((rows, cols))).astype(np.float32)
  ad, bd = _slice_of_wider(h, a), _slice_of_wider(h, b, 12)
  ma, mb, pw, lw, slope, icpt = _frame_stats(cols)
  for red in ('first', 'second', 'mean', 'mean-squared', 'lda', 'all'):
    if red == 'second' and cols < 2:
      with pytest.raises(ValueError, match='second'):
        dev.frame_scores(ad, bd, red, ma, mb, pw, handle=h)
      continue
    got = dev.frame_scores(ad, bd, red, ma, mb, pw, lda_w=lw, lda_slope=slope, lda_intercept=icpt,
                           handle=h).cpu().numpy()
    want, mag = _frame_reference(a, b, red, ma, mb, pw, lw, slope, icpt)
    assert got.shape == want.shape
    bound = (cols + 4) * EPS * mag
    ratio = float(np.max(np.abs(got - want) / bound))
    print('frame scores cols %d %s: worst error %.3g of the allowance' % (cols, red, ratio))
    parity_log.record('window_edge_frame_scores', cols=cols, reduction=red, worst_fraction_of_allowance=ratio)
    _note('frame_scores', ratio, 'c%d-%s' % (cols, red))
    assert np.all(np.abs(got - want) <= bound), (cols, red, ratio)


@pytest.mark.parametrize('cols', [1, 3])
def test_frame_scores_past_the_cap_of_the_grid(dev, cols):
  """4096 workgroups of 256 and 257 rows more: the grid-stride loop runs a second time.  The last 300 rows and a
  random thousand of the rest."""
  import torch
  h = dev.default_handle()
  rows = 4096 * 256 + 257
  gen = torch.Generator(device='cpu').manual_seed(90 + cols)
  a = torch.randn((rows, cols), generator=gen, dtype=torch.float32) + 0.5
  b = 0.6 * a + torch.randn((rows, cols), generator=gen, dtype=torch.float32)
  ma, mb, pw, lw, slope, icpt = _frame_stats(cols)
  pick = np.concatenate((np.sort(np.random.default_rng(cols).choice(rows - 300, 1000, replace=False)),
                         np.arange(rows - 300, rows)))
  assert np.sum(pick >= 4096 * 256) == 257
  ah, bh = a.numpy()[pick], b.numpy()[pick]
  ad, bd = h.to_device(a), h.to_device(b)
  for red in ('mean', 'lda', 'all'):
    got = dev.frame_scores(ad, bd, red, ma, mb, pw, lda_w=lw, lda_slope=slope, lda_intercept=icpt, handle=h)
    assert got.shape[0] == rows
    got = got[torch.from_numpy(pick).to(got.device)].cpu().numpy()
    want, mag = _frame_reference(ah, bh, red, ma, mb, pw, lw, slope, icpt)
    bound = (cols + 4) * EPS * mag
    ratio = float(np.max(np.abs(got - want) / bound))
    _note('frame_scores', ratio, 'c%d-%s-rows%d' % (cols, red, rows))
    assert np.all(np.abs(got - want) <= bound), (cols, red, ratio, pick[np.argmax(np.abs(got - want) / bound)])


# ---- 4. window means ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [1, 2, 255, 256, 257, 1000])
def test_window_means_around_the_workgroup_stride(dev, width):
  """Three ragged trials, the middle one a frame short of a window, hop 1 and hop = width."""
  h = dev.default_handle()
  lens = (width + 7, width - 1, 2 * width + 3)
  offs = np.concatenate(([0], np.cumsum(lens)))
  v = np.random.default_rng(width).standard_normal(int(offs[-1])) + 0.5
  vd = _d64(h, v)
  for hop in sorted({1, width}):
    starts = np.concatenate([offs[t] + o_cor.window_starts(lens[t], width, hop) for t in range(3)])
    got = dev.window_means(vd, offs, width, hop, handle=h).cpu().numpy()
    assert got.shape == (len(starts),) and len(o_cor.window_starts(lens[1], width, hop)) == 0
    want = np.array([np.sum(v[s:s + width]) / width for s in starts])
    bound = np.array([width * EPS * np.sum(np.abs(v[s:s + width])) / width for s in starts])
    ratio = float(np.max(np.abs(got - want) / bound))
    parity_log.record('window_edge_means', width=width, hop=hop, worst_fraction_of_allowance=ratio)
    _note('window_means', ratio, 'w%d-h%d' % (width, hop))
    assert np.all(np.abs(got - want) <= bound), (width, hop, ratio)


# ---- 5. decisions ---------------------------------------------------------------------------------------------------
def test_decide_wta_past_the_cap_of_the_grid(dev):
  """2048 workgroups of 256 and one element more, with ties, signed zeros and NaNs: s1 > s2, exactly."""
  h = dev.default_handle()
  n = 2048 * 256 + 1
  s1, s2 = we.wta_inputs(n)
  got = dev.decide_wta(_d64(h, s1), _d64(h, s2), handle=h).cpu().numpy()
  with np.errstate(invalid='ignore'):
    want = (s1 > s2).astype(np.uint8)
  assert got.shape == (n,) and got.dtype == np.uint8
  np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('n_trials', we.STEP_TRIALS)
def test_decide_step_across_workgroups_of_trials(dev, n_trials):
  """One lane per trial, 64 to a workgroup: ragged window counts with 0 and 1, starting states 0.1 / 0.5 / 0.9,
  decisions and returned states equal to the oracle's per trial; and the same launch split in two calls with the
  state carried."""
  h = dev.default_handle()
  s1, s2, wo, states = we.step_inputs(n_trials)
  got, st = dev.decide_step(_d64(h, s1), _d64(h, s2), wo, state=states.copy(), handle=h)
  got = got.cpu().numpy()
  want_states = np.zeros(n_trials)
  for t in range(n_trials):
    r = slice(wo[t], wo[t + 1])
    want, want_states[t] = o_att.step_sequence(s1[r], s2[r], state=float(states[t]))
    np.testing.assert_array_equal(got[r], want.astype(np.uint8), err_msg='trial %d' % t)
  np.testing.assert_array_equal(st, want_states)
  # first halves, then the rest
  half = [(int(wo[t]), int(wo[t] + (wo[t + 1] - wo[t]) // 2), int(wo[t + 1])) for t in range(n_trials)]
  i1 = np.concatenate([np.arange(lo, mid) for lo, mid, _ in half]).astype(np.int64)
  i2 = np.concatenate([np.arange(mid, hi) for _, mid, hi in half]).astype(np.int64)
  wo1 = np.concatenate(([0], np.cumsum([mid - lo for lo, mid, _ in half])))
  wo2 = np.concatenate(([0], np.cumsum([hi - mid for _, mid, hi in half])))
  both = np.zeros(len(s1), np.uint8)
  st1 = states.copy()
  if len(i1):
    o1, st1 = dev.decide_step(_d64(h, s1[i1]), _d64(h, s2[i1]), wo1, state=st1, handle=h)
    both[i1] = o1.cpu().numpy()
  o2, st2 = dev.decide_step(_d64(h, s1[i2]), _d64(h, s2[i2]), wo2, state=st1, handle=h)
  both[i2] = o2.cpu().numpy()
  np.testing.assert_array_equal(both, got)
  np.testing.assert_array_equal(st2, want_states)


# ---- 6. the state-space decoder -------------------------------------------------------------------------------------
def _ssd(dev, case, c, wo=None, state=None):
  h = dev.default_handle()
  k_f, k_b = case[0], case[1]
  prior = we.ssd_prior(case, we.ssd_stream(k_f, k_b))
  return dev.decode_ssd(_d64(h, c[:, 0]), _d64(h, c[:, 1]), [0, c.shape[0]] if wo is None else wo, prior=prior,
                        handle=h, state=state, **we.ssd_kwargs(case)).cpu().numpy()


@pytest.mark.parametrize('case', we.SSD_CASES, ids=we.ssd_id)
def test_decode_ssd_at_every_lag_of_the_table(dev, case):
  """kw from 1 to 32 (every branch of np_sum, arrays full at 32), forward lags, three settings: the oracle's
  trajectory and the reference's own at rtol 1e-7, atol 1e-9."""
  g = golden('g7b_decoder_lags')
  c = we.ssd_stream(case[0], case[1])
  got = _ssd(dev, case, c)
  want = we.ssd_oracle(case)
  kw = case[0] + case[1] + 1
  tol = 1e-9 + 1e-7 * np.abs(want)
  ratio = float(np.max(np.abs(got - want) / tol))
  print('ssd %s (kw %d): worst error %.3g of the allowance' % (we.ssd_id(case), kw, ratio))
  parity_log.record('window_edge_ssd', where=we.ssd_id(case), kw=kw, worst_fraction_of_allowance=ratio,
                    max_abs=float(np.max(np.abs(got - want))))
  _note('ssd_kw%02d' % kw, ratio, we.ssd_id(case))
  assert np.all(got[:kw - 1] == 0.5)
  np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-9)
  np.testing.assert_allclose(got, g[we.ssd_key(case) + '_traj'], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize('n_trials', we.BATCH_TRIALS)
@pytest.mark.parametrize('lags', we.BATCH_LAGS, ids=lambda l: 'f%d-b%d' % l)
def test_decode_ssd_across_workgroups_of_trials(dev, lags, n_trials):
  """Five streams of 0, 1, kw - 1, kw and 40 windows dealt round-robin over 64, 65 and 130 trials: every trial
  has the bits of the single-trial run of its stream, which is the oracle's trajectory."""
  case = lags + ('default',)
  streams = we.batch_streams(*lags)
  single = [_ssd(dev, case, s) if len(s) else np.zeros((0, 3)) for s in streams]
  for s, o in zip(streams, single):
    if len(s):
      np.testing.assert_allclose(o, we.ssd_oracle(case, s), rtol=1e-7, atol=1e-9)
  deal = [t % len(streams) for t in range(n_trials)]
  c = np.concatenate([streams[i] for i in deal])
  wo = np.concatenate(([0], np.cumsum([len(streams[i]) for i in deal])))
  got = _ssd(dev, case, c, wo=wo)
  assert got.shape == (int(wo[-1]), 3)
  for t, i in enumerate(deal):
    np.testing.assert_array_equal(got[wo[t]:wo[t + 1]], single[i], err_msg='trial %d of %d' % (t, n_trials))


@pytest.mark.parametrize('setting', ['default', 'tuned'])
@pytest.mark.parametrize('lags', we.STREAM_LAGS, ids=lambda l: 'f%d-b%d' % l)
def test_decode_ssd_with_carried_state(dev, lags, setting):
  """One window at a time and in uneven chunks through ssd_state: the bits of the single call."""
  h = dev.default_handle()
  case = lags + (setting,)
  c = we.ssd_stream(*lags)
  whole = _ssd(dev, case, c)
  st = dev.ssd_state(1, handle=h)
  one = [_ssd(dev, case, c[i:i + 1], state=st) for i in range(len(c))]
  np.testing.assert_array_equal(np.concatenate(one), whole)
  st = dev.ssd_state(1, handle=h)
  cuts = we.STREAM_CHUNKS
  assert cuts[0] == 0 and cuts[-1] == len(c)
  chunks = [_ssd(dev, case, c[lo:hi], state=st) for lo, hi in zip(cuts[:-1], cuts[1:])]
  np.testing.assert_array_equal(np.concatenate(chunks), whole)


def test_decode_ssd_refuses_lags_it_has_no_room_for(dev):
  h = dev.default_handle()
  s = _d64(h, np.full(4, 0.1))
  for k_f, k_b in ((0, 32), (16, 16), (32, 0)):
    with pytest.raises(ValueError, match='must be <= 32'):
      dev.decode_ssd(s, s, [0, 4], forward_lag=k_f, backward_lag=k_b, handle=h)
  for k_f, k_b in ((-1, 5), (2, -1)):
    with pytest.raises(ValueError):
      dev.decode_ssd(s, s, [0, 4], forward_lag=k_f, backward_lag=k_b, handle=h)
  assert dev.decode_ssd(s, s, [0, 4], forward_lag=0, backward_lag=31, handle=h).shape == (4, 3)


@pytest.mark.parametrize('setting', ['default', 'tuned'])
def test_state_space_decoder_class_at_other_lags(dev, setting):
  """StateSpaceAttentionDecoder with forward_lag 3, backward_lag 11: the streaming call and attention_batch
  against the reference's trajectory."""
  from telluride_decoding_amd import attention_decoder as ad
  g = golden('g7b_decoder_lags')
  k_f, k_b = we.WRAPPER_LAGS
  case = (k_f, k_b, setting)
  key = we.ssd_key(case)
  c, want = g[key + '_corr'], g[key + '_traj']
  outer, inner, newton, offset, tuned = we.SETTINGS[setting]
  made = ad.create_attention_decoder('ssd', ssd_offset=offset)
  assert isinstance(made, ad.StateSpaceAttentionDecoder)
  assert (made.outer_iter, made.inner_iter, made.newton_iter, made.k_f, made.k_b) == (20, 1, 10, 0, 13)
  decoders = []
  for _ in range(2):
    dec = ad.StateSpaceAttentionDecoder(outer, inner, newton, made.fs_corr, forward_lag=k_f, backward_lag=k_b,
                                        offset=offset)
    assert dec.k_w == k_f + k_b + 1
    if tuned:
      dec.tune(c[:we.TUNE_WINDOWS, 0], c[:we.TUNE_WINDOWS, 1])
      np.testing.assert_allclose(dec.mu_d, g[key + '_mu_d_tuned'], rtol=1e-12)
      np.testing.assert_allclose(dec.rho_d, g[key + '_rho_d_tuned'], rtol=1e-12)
    decoders.append(dec)
  stream = np.array([decoders[0].attention(x, y) for x, y in c])
  np.testing.assert_allclose(stream, want, rtol=1e-7, atol=1e-9)
  p, lo, hi = decoders[1].attention_batch(c[:, 0], c[:, 1])
  np.testing.assert_allclose(np.stack((p, lo, hi), axis=1), want, rtol=1e-7, atol=1e-9)
  # two trials in one call: each its own decoder
  p2, lo2, hi2 = decoders[1].attention_batch(np.tile(c[:, 0], 2), np.tile(c[:, 1], 2), [0, len(c), 2 * len(c)])
  np.testing.assert_array_equal(np.stack((p2, lo2, hi2), axis=1), np.tile(np.stack((p, lo, hi), axis=1), (2, 1)))
