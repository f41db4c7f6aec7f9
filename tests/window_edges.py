"""The edge cases of the window, score and decision kernels of csrc/windows.hip (tests/test_gpu_window_edges.py,
tests/test_cpu_window_edges.py): the case tables of td_window_sums_cycled and of the state-space decoder, their
host-side references (no GPU needed) and restatements of the integer arithmetic by which td_window_sums_cycled picks
its kernels, of np_sum and of the step decoder's recurrence.  A plain module, not a conftest.

A window-sum case is (cols, b_cols, width, hop): column j of `a` against column j % b_cols of `b`, full windows of
`width` frames every `hop` in five trials of lengths trial_lengths(width, hop): several windows, an empty trial, a
trial one frame short of a window, exactly one window, one frame short of a second window."""
import functools
import math

import numpy as np

from oracle import attention as o_att
from oracle import correlator as o_cor

LD = np.longdouble
EPS = 2.0 ** -52

# ---- the route of td_window_sums_cycled, restated -------------------------------------------------------------------
BLOCK_LANES = 16       # kBlockLanes
NARROW_MAX = 64        # window_from_blocks_kernel up to this many blocks per window
SHORT_MAX = 256        # window_sums_short_kernel up to this width
COLS_KERNEL = (8, 64)  # block_sums_cols_kernel serves this range of column counts (both ends included)


def window_block_size(width, hop):
  """window_block_size of windows.hip: the largest divisor of gcd(width, hop) in [32, 256], else the largest in
  [32, 4096]; 0 if there is none or a window would span more than 2^16 blocks."""
  g = math.gcd(width, hop)
  best = 0
  for dv in range(min(g, 256), 31, -1):
    if g % dv == 0:
      best = dv
      break
  if best == 0:
    for dv in range(min(g, 4096), 31, -1):
      if g % dv == 0:
        best = dv
        break
  if best == 0 or width // best > (1 << 16):
    return 0
  return best


def route(case):
  """(g, blocks per window, block kernel, window kernel) of a case, or 'short' / 'per_window'."""
  cols, _, width, hop = case
  g = window_block_size(width, hop)
  if g > 0:
    block = 'cols' if COLS_KERNEL[0] <= cols <= COLS_KERNEL[1] else 'lanes'
    return g, width // g, block, 'wide' if width // g > NARROW_MAX else 'narrow'
  return 'short' if width <= SHORT_MAX else 'per_window'


def route_name(case):
  """One of the five ways through td_window_sums_cycled that the table takes."""
  r = route(case)
  return r if isinstance(r, str) else '%s+%s' % r[2:]


def rows_per_step(cols):
  """`per` of block_sums_cols_kernel: whole rows a wave reads per step."""
  return 64 // cols


# ---- the window-sum table -------------------------------------------------------------------------------------------
BLOCK_SHAPES = [(96, 32), (66, 33), (200, 100)]            # g = 32, 33, 100: every column count
LONG_SHAPES = [(514, 257), (2048, 32), (2080, 32)]         # g = 257 (second search loop); 64 and 65 blocks per window
SHORT_SHAPES = [(10, 5), (7, 3), (256, 7)]                 # no common block, width <= 256
PER_WINDOW_SHAPES = [(257, 7)]                             # no common block, width > 256
BLOCK_COLS = [1, 7, 8, 9, 21, 32, 33, 63, 64, 65, 130]
OTHER_COLS = [1, 7, 65]
EXPECTED_ROUTE = {(96, 32): (32, 3), (66, 33): (33, 2), (200, 100): (100, 2), (514, 257): (257, 2),
                  (2048, 32): (32, 64), (2080, 32): (32, 65), (10, 5): 'short', (7, 3): 'short',
                  (256, 7): 'short', (257, 7): 'per_window'}


def proper_divisor(cols):
  """The b_cols of a case's cycled run: 3 for 21 and 63, 13 for 65 and 130, else 1 (none for one column)."""
  if cols == 1:
    return None
  return {21: 3, 63: 3, 65: 13, 130: 13}.get(cols, 1)


def _cases():
  out = []
  for shapes, col_list, cycled in ((BLOCK_SHAPES, BLOCK_COLS, True), (LONG_SHAPES, OTHER_COLS, True),
                                   (SHORT_SHAPES + PER_WINDOW_SHAPES, OTHER_COLS, False)):
    for width, hop in shapes:
      for cols in col_list:
        out.append((cols, cols, width, hop))
        if cycled and proper_divisor(cols) is not None:
          out.append((cols, proper_divisor(cols), width, hop))
  return out


CASES = _cases()
# one case per route again on contiguous tensors (the table itself runs on column slices of wider tensors)
CONTIGUOUS_CASES = [(21, 3, 66, 33), (65, 13, 200, 100), (7, 1, 2080, 32), (7, 7, 7, 3), (65, 65, 257, 7)]
EXTRA_COLS, FIRST_COL = 3, 1          # a case's a and b are [:, 1:1 + cols] of tensors 3 columns wider


def case_id(case):
  return 'c%d-b%d-w%d-h%d' % case


def trial_lengths(width, hop):
  return (width + 3 * hop + 1, 0, width - 1, width, width + hop - 1)


def trial_offsets(case):
  return np.concatenate(([0], np.cumsum(trial_lengths(case[2], case[3])))).astype(np.int64)


def window_rows(case):
  """The first row of every window, trial after trial."""
  offs = trial_offsets(case)
  return np.concatenate([offs[t] + o_cor.window_starts(int(offs[t + 1] - offs[t]), case[2], case[3])
                         for t in range(len(offs) - 1)])


@functools.lru_cache(maxsize=None)
def window_data(case):
  """(a [rows, cols], b [rows, b_cols]) float32: standard normal + 0.5, seeded per case.  (Cached: whoever reads
  them leaves them unchanged.)"""
  cols, b_cols, width, hop = case
  rng = np.random.default_rng([cols, b_cols, width, hop])
  rows = int(trial_offsets(case)[-1])
  a = (rng.standard_normal((rows, cols)) + 0.5).astype(np.float32)
  b = (rng.standard_normal((rows, b_cols)) + 0.5).astype(np.float32)
  return a, b


def five_sums(a, b, starts, width, dt=np.float64, pair_shift=0, extra_rows=0, drop_last_of=None):
  """[windows, cols, 5]: sum a, sum b, sum a^2, sum b^2, sum a b of every window, by slicing, in the type dt;
  column j of a goes with column (j + pair_shift) % b_cols of b.  extra_rows: every window reads that many rows
  more; drop_last_of: that window loses its last frame (the three planted errors of the CPU tests)."""
  cols, b_cols = a.shape[1], b.shape[1]
  pair = (np.arange(cols) + pair_shift) % b_cols
  out = np.zeros((len(starts), cols, 5), dt)
  for w, r0 in enumerate(starts):
    r1 = r0 + width + extra_rows - (1 if drop_last_of == w else 0)
    x, y = a[r0:r1].astype(dt), b[r0:r1][:, pair].astype(dt)
    out[w] = np.stack([x.sum(0), y.sum(0), (x * x).sum(0), (y * y).sum(0), (x * y).sum(0)], axis=1)
  return out


def abs_sums(a, b, starts, width):
  """sum |term| of each of the five sums, float64."""
  return five_sums(np.abs(a), np.abs(b), starts, width)


@functools.lru_cache(maxsize=None)
def window_references(case):
  """(float64 sums, long double sums, sum |term|) of a case, each [windows, cols, 5]."""
  a, b = window_data(case)
  starts, width = window_rows(case), case[2]
  return (five_sums(a, b, starts, width), five_sums(a, b, starts, width, LD), abs_sums(a, b, starts, width))


def window_bound(case):
  """|got - want| <= width 2^-52 sum |term|: the terms (float32 values and products of two of them) are exact in
  float64, a sum of n of them in any order stays within (n - 1) 2^-53 sum |term| of the true sum, and two orders
  within twice that of each other."""
  return case[2] * EPS * window_references(case)[2]


# ---- the kernels' order of summation, restated ----------------------------------------------------------------------
# Every sum of these kernels has a fixed order (windows.hip promises the same bits on every call, and the fused decode
# is tested bit for bit against this chain), so the order can be followed on the host in float64 -- the terms are
# exact, every addition rounds as the device's does -- and the result compared bit for bit.  That pins WHICH kernel
# served a case: the two block kernels and the two window-from-blocks kernels are each right on both sides of their
# thresholds and differ only in this order.
def _seq(t):
  """The terms of axis 0 added one after the other, from 0.0."""
  s = np.zeros(t.shape[1:])
  for row in t:
    s = s + row
  return s


def _shuffle_down_tree(v):
  """Lane 0 of wave_sum: v += shfl_down(v, 32), 16, 8, 4, 2, 1 over the 64 lanes of axis 0."""
  v = v.copy()
  for off in (32, 16, 8, 4, 2, 1):
    v[:off] = v[:off] + v[off:2 * off]
  return v[0]


def _block_sums(t, block):
  """t [blocks, g, cols, 5] -> [blocks, cols, 5] in the order of block_sums_kernel ('lanes': 16 lanes stride
  through the block's rows, then the tree v += v[lane ^ 8], ^ 4, ^ 2, ^ 1) or of block_sums_cols_kernel ('cols': the
  64 // cols row phases each in ascending order, then added to phase 0 in ascending order)."""
  t = np.moveaxis(t, 1, 0)                                  # [g, blocks, cols, 5]
  if block == 'lanes':
    v = np.stack([_seq(t[sub::BLOCK_LANES]) for sub in range(BLOCK_LANES)])
    for m in (8, 4, 2, 1):
      v = v + v[np.arange(BLOCK_LANES) ^ m]
    return v[0]
  per = rows_per_step(t.shape[2])
  v = _seq(t[0::per])
  for q in range(1, per):
    v = v + _seq(t[q::per])
  return v


@functools.lru_cache(maxsize=None)
def device_order_sums(case, forced_route=None):
  """[windows, cols, 5]: the five sums with every addition in the order of the kernels that route(case) names (or
  forced_route: what another dispatch would have given)."""
  cols, b_cols, width, hop = case
  a, b = window_data(case)
  x, y = a.astype(np.float64), b[:, np.arange(cols) % b_cols].astype(np.float64)
  terms = np.stack([x, y, x * x, y * y, x * y], axis=2)     # [rows, cols, 5], exact
  r = route(case) if forced_route is None else forced_route
  offs = trial_offsets(case)
  out = []
  for t in range(len(offs) - 1):
    n = int(offs[t + 1] - offs[t])
    tw = len(o_cor.window_starts(n, width, hop))
    rows = terms[offs[t]:offs[t + 1]]
    if tw == 0:
      continue
    if r == 'short':                                        # one thread per window and column, ascending
      out += [_seq(rows[w * hop:w * hop + width]) for w in range(tw)]
    elif r == 'per_window':                                 # 256 threads stride through the window; four wave trees
      for w in range(tw):
        win = rows[w * hop:w * hop + width]
        lanes = np.stack([_seq(win[tid::256]) for tid in range(256)])
        waves = [_shuffle_down_tree(lanes[64 * k:64 * k + 64]) for k in range(4)]
        out.append((waves[0] + waves[1]) + (waves[2] + waves[3]))
    else:
      g, per_win, block, window = r
      nb = ((tw - 1) * hop + width) // g
      bs = _block_sums(rows[:nb * g].reshape(nb, g, cols, 5), block)
      for w in range(tw):
        mine = bs[w * (hop // g):w * (hop // g) + per_win]
        if window == 'narrow':                              # one thread walks the window's blocks
          out.append(_seq(mine))
        else:                                               # 64 lanes stride through them, then the wave tree
          lanes = np.stack([_seq(mine[j::64]) for j in range(64)])
          out.append(_shuffle_down_tree(lanes))
  return np.stack(out)


# ---- np_sum of windows.hip, restated --------------------------------------------------------------------------------
def np_sum(a):
  """NumPy's pairwise routine below its block size of 128: 8 running sums for n >= 8, combined as a balanced tree,
  then the tail -- in Python floats, the operations of np_sum in windows.hip."""
  a = [float(v) for v in a]
  n = len(a)
  if n < 8:
    s = 0.0
    for v in a:
      s += v
    return s
  r = a[:8]
  i = 8
  while i < n - (n % 8):
    for j in range(8):
      r[j] += a[i + j]
    i += 8
  res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
  while i < n:
    res += a[i]
    i += 1
  return res


# ---- the decision kernels -------------------------------------------------------------------------------------------
STEP_TRIALS = [1, 64, 65, 130]
STEP_STATES = (0.1, 0.5, 0.9)


def step_recurrence(s1, s2, state):
  """decide_step_kernel's scan of one trial: (decisions, final state)."""
  out = []
  for x, y in zip(s1, s2):
    state = min(0.9, state + 0.1) if x > y else max(0.1, state - 0.1)
    out.append(state > 0.5)
  return np.array(out, dtype=bool), state


@functools.lru_cache(maxsize=None)
def step_inputs(n_trials):
  """(s1, s2, window_offsets, starting states) of a launch of n_trials trials: ragged window counts with 0 and 1
  among them (a trial without windows in the middle of the launch as soon as there are three), scores rounded to
  one decimal (ties), starting states 0.1 / 0.5 / 0.9 in turn."""
  rng = np.random.default_rng(400 + n_trials)
  counts = rng.integers(2, 30, n_trials)
  counts[1::7] = 0
  counts[2::7] = 1
  if n_trials == 1:
    counts[0] = 23
  wo = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
  s1 = np.round(rng.standard_normal(int(wo[-1])), 1)
  s2 = np.round(rng.standard_normal(int(wo[-1])), 1)
  states = np.array([STEP_STATES[t % 3] for t in range(n_trials)], np.float64)
  return s1, s2, wo, states


def wta_inputs(n):
  """Two score streams of n entries with planted ties, signed zeros and NaNs on either side and on both."""
  rng = np.random.default_rng(77)
  s1, s2 = rng.standard_normal(n), rng.standard_normal(n)
  idx = rng.permutation(n)[:6000].reshape(6, 1000)
  idx[:, -1] = [n - 1, n - 2, n - 3, n - 4, n - 5, n - 6]      # the element after the capped grid among them
  s2[idx[0]] = s1[idx[0]]
  s1[idx[1]], s2[idx[1]] = 0.0, -0.0
  s1[idx[2]], s2[idx[2]] = -0.0, 0.0
  s1[idx[3]] = np.nan
  s2[idx[4]] = np.nan
  s1[idx[5]], s2[idx[5]] = np.nan, np.nan
  return s1, s2


# ---- the state-space decoder ----------------------------------------------------------------------------------------
MAX_KW = 32            # kMaxKw
LAGS = [(0, 0), (0, 1), (0, 6), (0, 7), (1, 7), (3, 11), (0, 14), (0, 15), (2, 14), (0, 31), (5, 26)]
SSD_WINDOWS, TUNE_WINDOWS = 60, 30
# name -> (outer_iter, inner_iter, newton_iter, offset, tuned on the first TUNE_WINDOWS windows)
SETTINGS = {'default': (20, 1, 10, 0.0, False), 'tuned': (20, 1, 10, 0.0, True), 'short': (3, 2, 4, 1.0, False)}
SSD_CASES = [(k_f, k_b, s) for k_f, k_b in LAGS for s in ('default', 'tuned', 'short')]
BATCH_LAGS = [(0, 7), (3, 11), (0, 31)]
BATCH_TRIALS = [64, 65, 130]
STREAM_LAGS = [(1, 7), (5, 26)]
STREAM_CHUNKS = (0, 3, 4, 11, 12, 37, 38, 59, 60)       # uneven chunks of the 60 windows
WRAPPER_LAGS = (3, 11)


def ssd_id(case):
  return 'f%d-b%d-%s' % case


def ssd_key(case):
  return 'f%d_b%d_%s' % case


@functools.lru_cache(maxsize=None)
def ssd_stream(k_f, k_b, n=SSD_WINDOWS):
  """[n, 2] correlations of the two speakers: 0.15 + 0.05 N(0, 1) and 0.05 + 0.05 N(0, 1), seeded per lag pair."""
  rng = np.random.default_rng(7000 + 64 * k_f + k_b)
  return np.stack((0.15 + 0.05 * rng.standard_normal(n), 0.05 + 0.05 * rng.standard_normal(n)), axis=1)


def ssd_prior(case, c=None):
  """(rho_d, mu_d) of a tuned case, None otherwise."""
  k_f, k_b, setting = case
  c = ssd_stream(k_f, k_b) if c is None else c
  offset, tuned = SETTINGS[setting][3:]
  return o_att.tune_log_normal_priors(c[:TUNE_WINDOWS, 0], c[:TUNE_WINDOWS, 1], offset) if tuned else None


def ssd_kwargs(case):
  k_f, k_b, setting = case
  outer, inner, newton, offset, _ = SETTINGS[setting]
  return dict(outer_iter=outer, inner_iter=inner, newton_iter=newton, forward_lag=k_f, backward_lag=k_b,
              offset=offset)


def ssd_oracle(case, c=None):
  """The [windows, 3] trajectory of oracle.attention.StateSpace on a case's stream (or on c)."""
  k_f, k_b, setting = case
  c = ssd_stream(k_f, k_b) if c is None else c
  dec = o_att.StateSpace(**ssd_kwargs(case))
  if SETTINGS[setting][4]:
    dec.tune(c[:TUNE_WINDOWS, 0], c[:TUNE_WINDOWS, 1])
  return np.array([dec.attention(x, y) for x, y in c], np.float64).reshape(-1, 3)


def batch_lengths(k_f, k_b):
  """The five stream lengths of the batched runs: no window, one, one short of the first estimate, the first
  estimate, and 40."""
  kw = k_f + k_b + 1
  return (0, 1, kw - 1, kw, 40)


@functools.lru_cache(maxsize=None)
def batch_streams(k_f, k_b):
  """Five distinct streams of batch_lengths(k_f, k_b) windows."""
  out = []
  for i, n in enumerate(batch_lengths(k_f, k_b)):
    rng = np.random.default_rng(9000 + 1000 * i + 64 * k_f + k_b)
    out.append(np.stack((0.15 + 0.05 * rng.standard_normal(n), 0.05 + 0.05 * rng.standard_normal(n)), axis=1))
  return tuple(out)
