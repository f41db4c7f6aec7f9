"""The edge cases of the Ledoit-Wolf kernels of csrc/shrink.hip (tests/test_gpu_shrink_edges.py,
tests/test_cpu_shrink_edges.py): the case tables of td_shrinkage_moment, their host-side references (no GPU needed)
and a restatement of the integer arithmetic by which td_shrinkage_moment picks a route.  A plain module, not a conftest.

A case is (c, pre, post, input_offset, lens, batch, drop): recordings of `lens` rows and c channels, the lag window
[-pre, post], minibatches of `batch` rows of the concatenated lag stream.  drop = True trims rows_used to whole
minibatches (what batch(drop_remainder=True) leaves: tests/test_gpu_fit.py's recipe), drop = False leaves a shorter
last minibatch.  The data is that of test_shrinkage_moment_matches_reference_accumulation: standard normal + 0.7 as
float32, seed 99 + c."""
import functools

import numpy as np

from oracle import lag as o_lag

LD = np.longdouble

# ---- the tables ---------------------------------------------------------------------------------------------------
# Group A: small K, where ONE wrong edge sample moves the result by more than the bound.  Files shorter than a
# minibatch, than the context and than the offset; an empty file; a minibatch over three files; 1, 3 and 5 lags on the
# tiled route (its two lag halves uneven, one of them empty); tiles that cross a file and tiles that do not.
GROUP_A = [
    (4, 1, 1, 0, (40, 7, 23), 16),
    (4, 2, 0, 0, (1, 1, 50), 8),
    (8, 2, 3, 2, (150, 0, 131, 5), 64),
    (8, 0, 5, -3, (150, 2, 131), 64),
    (3, 1, 1, 0, (40, 7, 23), 16),
    (5, 2, 3, 2, (150, 0, 131, 5), 64),
    (12, 3, 0, 0, (90, 33), 32),
    (12, 0, 0, 0, (90, 33), 32),
    (8, 1, 1, 0, (100, 60, 200), 256),
    (4, 2, 2, 0, (100, 60, 200), 256),
]
# Group B: K > 256 with minibatches that span recordings (the column sums of such a minibatch are added up piece by
# piece), a shorter last minibatch everywhere.
GROUP_B = [
    (20, 0, 12, 0, (300, 170, 231), 128),     # tiled, K = 260
    (13, 3, 16, 0, (300, 170, 231), 100),     # wave route, K = 260
    (68, 0, 3, 0, (300, 170, 231), 128),      # two channel passes, tiled
    (72, 1, 2, -2, (300, 170, 231), 128),     # the same with a pre-context and an offset
    (64, 0, 31, 0, (700, 500), 256),          # the decoding shape at its smallest spanning size
    (100, 0, 31, 0, (700, 500), 256),         # a tile of 64 624 bytes: the largest that fits
    (104, 0, 31, 0, (700, 500), 256),         # 69 712 bytes: the first that does not (wave route, c % 4 == 0)
]
CASES_A = [s + (drop,) for s in GROUP_A for drop in (True, False)]
CASES_B = [s + (False,) for s in GROUP_B]
CASES = CASES_A + CASES_B

A1, A3 = GROUP_A[0] + (False,), GROUP_A[2] + (False,)
B1, B2, B5 = (GROUP_B[i] + (False,) for i in (0, 1, 4))
# column slices of a wider tensor: (extra columns, first column).  ldx = c + 4 from column 0 keeps the 16-byte
# staging loads with ldx > c; ldx = c + 3 from column 1 is neither a multiple of 4 nor aligned: scalar staging
VIEWS = [(4, 0), (3, 1)]
VIEW_CASES = [A3, B1, B5]
LARGEST_TILE, FIRST_TOO_LARGE = 64624, 69712


def case_id(case):
  c, pre, post, off, lens, batch, drop = case
  return 'c%d-l%d+%d-o%d-%s-B%d-%s' % (c, pre, post, off, 'x'.join(map(str, lens)), batch, 'drop' if drop else 'tail')


# ---- data ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recordings(case):
  """The recordings of a case.  (Cached: whoever reads them leaves them unchanged.)"""
  c, lens = case[0], case[4]
  rng = np.random.default_rng(99 + c)
  return tuple((rng.standard_normal((n, c)) + 0.7).astype(np.float32) for n in lens)


def _file_streams(case, files=None):
  c, pre, post, off = case[:4]
  out = []
  for x in (recordings(case) if files is None else files):
    a = np.zeros((x.shape[0], 1), np.float32)
    xl, _, _, _ = o_lag.window_streams(x, a, a, a, pre=pre, post=post, input_offset=off)
    out.append(xl)
  return out


def layout(case):
  """(rows every file adds to the lag stream, rows of the stream in use, rows_used for the device call or None)."""
  batch, drop = case[5], case[6]
  rows = [s.shape[0] for s in _file_streams(case)]
  if not drop:
    return rows, sum(rows), None
  total = (sum(rows) // batch) * batch
  used, left = [], total
  for n in rows:
    used.append(min(left, n))
    left -= used[-1]
  return rows, total, used


def minibatches(case, files=None):
  """The minibatches of the lag stream, float32, as the reference's dataset hands them out."""
  batch = case[5]
  _, total, _ = layout(case)
  stream = np.concatenate(_file_streams(case, files))
  return [stream[i:min(i + batch, total)] for i in range(0, total, batch)]


# ---- the three references -----------------------------------------------------------------------------------------
def _moment(batches, dt, extra=None):
  """np.sum(sum_x2tx2) of brain_model.py:429-443 in the type dt, as sum_r (sum_k xc[r, k]^2)^2.  extra: {minibatch:
  a row that is added to sum_x with that minibatch} -- a column sum that was added once too often."""
  sum_x, n, tot = 0.0, 0, dt(0.0)
  for b, x in enumerate(batches):
    x = np.asarray(x, dt)
    n += x.shape[0]
    sum_x = sum_x + x.sum(axis=0, keepdims=True)
    if extra is not None and b in extra:
      sum_x = sum_x + np.asarray(extra[b], dt)
    x2 = (x - sum_x / n) ** 2
    tot += (x2.sum(axis=1) ** 2).sum()
  return tot


def _lw_moment_numpy(batches, extra=None):
  """The literal minibatch loop in float64 (tests/test_gpu_fit.py's reference of the same name)."""
  return float(_moment(batches, np.float64, extra))


def lw_moment_longdouble(batches):
  return _moment(batches, LD)


def lw_moment_float32(batches):
  """The same loop in the reference's own arithmetic: float32 minibatches, a float32 running sum and mean, and the
  matrix (xc ** 2)^T (xc ** 2) itself, formed and summed in float32 (brain_model.py:438-443); the minibatches' sums
  are added up as the float64 loop adds them.  (The ones column of the reference is left out: its centred value is
  1 - n / n = 0 exactly.)"""
  sum_x, n, tot = 0.0, 0, 0.0
  for x in batches:
    x = np.asarray(x, np.float32)
    n += x.shape[0]
    sum_x = sum_x + np.sum(x, axis=0, keepdims=True)
    x2 = (x - sum_x / n) ** 2
    x2tx2 = x2.T @ x2
    assert x2tx2.dtype == np.float32
    tot += float(np.sum(x2tx2))
  return tot


@functools.lru_cache(maxsize=None)
def references(case):
  """(float64, long double, float32) results of a case."""
  b = minibatches(case)
  return _lw_moment_numpy(b), lw_moment_longdouble(b), lw_moment_float32(b)


# ---- the two planted errors ---------------------------------------------------------------------------------------
def edge_planted(case):
  """The float64 result with ONE zero-padded feature of the lag stream set to the nearest sample of its recording
  (what a clamped or off-by-one edge read would deliver), or None if the case has no context.  Of the padded features
  of the first recording's rows in use, the one whose nearest sample is largest: a sample of ordinary size and not one
  that happens to lie near zero."""
  c, pre, post, off = case[:4]
  if pre + post == 0:
    return None
  rows, _, used = layout(case)
  n = rows[0] if used is None else used[0]
  x = recordings(case)[0][max(off, 0):]
  lags = pre + 1 + post
  t = np.arange(n)[:, None] + np.arange(lags)[None, :] - pre             # the frame behind (row, lag)
  padded = np.repeat((t < 0) | (t >= x.shape[0]), c, axis=1)
  assert padded.any() and x.shape[0] > 0
  nearest = x[np.clip(t, 0, x.shape[0] - 1)].reshape(n, lags * c)
  stream0 = _file_streams(case)[0][:n]
  assert not stream0[padded].any()
  r, k = np.unravel_index(np.argmax(np.where(padded, np.abs(nearest), -1.0)), padded.shape)
  batches = [b.copy() for b in minibatches(case)]
  batch = case[5]
  batches[r // batch][r % batch, k] = nearest[r, k]
  return _lw_moment_numpy(batches)


def pieces(case):
  """Per minibatch the (first row, rows) of every piece that comes from one recording."""
  batch = case[5]
  rows, total, used = layout(case)
  ends = np.cumsum(rows if used is None else used)
  out = []
  for g in range(0, total, batch):
    g_end, p = min(g + batch, total), []
    while g < g_end:
      f = int(np.searchsorted(ends, g, side='right'))
      n = min(g_end, int(ends[f])) - g
      p.append((g, n))
      g += n
    out.append(p)
  return out


def race_planted(case):
  """The float64 result if the second piece of the first minibatch that spans recordings were added to the
  minibatch's column sums twice (two workgroups doing the same read-modify-write), or None if none spans."""
  batch = case[5]
  batches = minibatches(case)
  for b, p in enumerate(pieces(case)):
    if len(p) > 1:
      g, n = p[1]
      again = np.asarray(batches[b][g - b * batch:g - b * batch + n], np.float64).sum(axis=0, keepdims=True)
      return _lw_moment_numpy(batches, {b: again})
  return None


# ---- the route of td_shrinkage_moment, restated -------------------------------------------------------------------
SQ_TILE = 128          # kSqTile
WAVE_ROWS = 32         # kRowsPerWg


def route(case):
  """What the host code and the kernels derive from a shape: the route of the centred squares, its LDS bytes, the
  channel passes of the column sums, the minibatches that span recordings and the 128-row tiles that cross one."""
  c, pre, post, off, lens, batch, drop = case
  lags = pre + 1 + post
  stride = ((c // 4) | 1) * 4
  lds = 4 * ((SQ_TILE + lags - 1) * stride + 2 * SQ_TILE)
  tiled = c % 4 == 0 and lds <= 65536
  rows, total, used = layout(case)
  ends = np.cumsum(rows if used is None else used)
  p = pieces(case)
  crossing = plain = 0
  for b in range(len(p)):
    for g0 in range(b * batch, min(b * batch + batch, total), SQ_TILE):
      g_end = min(b * batch + batch, total, g0 + SQ_TILE)
      f = int(np.searchsorted(ends, g0, side='right'))
      if g_end <= ends[f]:
        plain += 1
      else:
        crossing += 1
  return dict(k=c * lags, lags=lags, tiled=tiled, lds=lds, passes=(c + 63) // 64, total=total, batches=len(p),
              spanning=sum(len(q) > 1 for q in p), most_pieces=max(len(q) for q in p),
              short_last=total % batch != 0, tiles_crossing=crossing, tiles_plain=plain,
              chunks=(batch + (SQ_TILE if tiled else WAVE_ROWS) - 1) // (SQ_TILE if tiled else WAVE_ROWS))


# ---- the shrinkage algebra: td_shrinkage_terms and td_shrunk_covariance -------------------------------------------
ALGEBRA_N = [1, 2, 16, 255, 256, 257, 513, 1100]     # 513^2 > 1024 * 256 and 1100^2 > 4096 * 256: the grids stride
EPS = 2.0 ** -52
FRAMES = 700.0


@functools.lru_cache(maxsize=None)
def moments_like(n):
  """A random symmetric float64 [n + 1, n + 1] whose last row and column look like the column sums of FRAMES frames
  (the ones row of the moments, the frame count in its corner)."""
  rng = np.random.default_rng(700 + n)
  a = rng.standard_normal((n + 1, n + 1))
  s = (a + a.T) * 0.5 * FRAMES + np.eye(n + 1) * FRAMES
  row = (0.3 + 0.2 * rng.standard_normal(n + 1)) * FRAMES
  row[n] = FRAMES
  s[n, :] = row
  s[:, n] = row
  return s


def terms_reference(s, m, row):
  """trace(zc) and sum(zc^2) of zc = s[:m, :m] - mean^T mean, mean = s[row, :m] / FRAMES, in long double, with the
  allowances of a float64 evaluation in any order (tests/test_gpu_decoding._reference's rule: a sum of n terms stays
  within n 2^-52 sum |terms|): every zc carries (|S_ij| + 3 |m_i m_j|) 2^-52 of its own -- one rounding of each
  mean, of the product and of the difference -- so the trace gets (m + 4) 2^-52 sum_i (|S_ii| + m_i^2) and the sum
  of squares 2^-52 (m^2 sum zc^2 + 8 sum |zc| (|S_ij| + |m_i m_j|))."""
  c = s[:m, :m].astype(LD)
  mean = s[row, :m].astype(LD) / LD(FRAMES)
  outer = mean[:, None] * mean[None, :]
  zc = c - outer
  mag = np.abs(c) + np.abs(outer)
  trace, sq = np.trace(zc), (zc ** 2).sum()
  tol_trace = (m + 4) * EPS * float(np.trace(mag))
  tol_sq = EPS * (m * m * float(sq) + 8.0 * float((np.abs(zc) * mag).sum()))
  return trace, sq, tol_trace, tol_sq
