"""Shared by the online CCA fit tests (CPU and GPU): two-view recordings driven by coloured sources, the shapes and
the cuts of a recording into pushes, the float64 references -- the joint lag matrix [lag_matrix(x) | lag_matrix(y) | 1]
and its moments, the dense stage through LAPACK, the two-pass statistics of a model's projections -- and a driver that
walks one cut through an online.OnlineCCAFit.  Everything is computed once per key and shared: treat what these
functions return as read-only.

The sources are coloured on purpose: with white sources the lagged canonical correlations come in near-equal
multiplets and the canonical vectors are not defined, so no comparison of rotations would mean anything."""
import numpy as np

from oracle import lag as olag

SEED = 4409
FORGETS = (1.0, 0.99)
DIM = 3
AR = (0.9, 0.5, 0.0, -0.6)                 # the sources' AR(1) coefficients (unit variance each)
STRENGTHS = (2.0, 1.2, 0.7, 0.4)

# (c1, pre1, post1, c2, pre2, post2, frames).  n = k1 + k2 + 1:
#   79: the EEG sets the delay; view 2 straddles the tile edge at 64
#    6: no tails at all
#   90: the features set the delay, the EEG tail is longer than its own context needs, the view boundary at column 63
#  128: k1 = one whole tile, n = two whole tiles, a one-column view
#  129: the ones row alone in a third tile
# 1473: the bench's CCA shape, 300 work tiles;  2049: the limit
SMALL = [(5, 2, 9, 3, 1, 4, 600), (3, 0, 0, 2, 0, 0, 300), (7, 3, 5, 2, 0, 12, 600), (16, 3, 0, 1, 0, 62, 600),
         (16, 3, 0, 1, 0, 63, 600)]
LARGE = [(64, 0, 20, 8, 0, 15, 120), (128, 0, 13, 32, 0, 7, 120)]
SHAPES = SMALL + LARGE
LARGE_PUSHES = (37, 1, 50, 32)
# the smallest gap between neighbouring canonical correlations (and from the last to 0) the recordings must keep, so
# that a tolerance scaled by 1 / gap means something: small shapes at lambda 0.1 and 1, the two large ones at 1
GAP_FLOOR = {s: 1.5e-2 for s in SMALL}
# (measured in NumPy float64 with this recipe at dim 3: >= 1.5e-2 on the small shapes, 5.27e-3 and 2.24e-3 at lambda 1
# on the two large ones)
GAP_FLOOR[LARGE[0]], GAP_FLOOR[LARGE[1]] = 5.2e-3, 2.2e-3


def shape_id(shape):
  return 'c%d_%d_%d__c%d_%d_%d_n%d' % tuple(shape)


def dim_of(shape):
  """DIM, or the narrower view's width where that is less (3 + 2 columns have two components)."""
  k1, k2 = sizes(shape)[:2]
  return min(DIM, k1, k2)


def lambdas_of(shape):
  return (0.1, 1.0) if shape in SMALL else (1.0,)


def sizes(shape):
  """(k1, k2, n, delay) of a shape."""
  c1, pre1, post1, c2, pre2, post2 = shape[:6]
  k1, k2 = (pre1 + 1 + post1) * c1, (pre2 + 1 + post2) * c2
  return k1, k2, k1 + k2 + 1, max(post1, post2)


_RECORDINGS = {}
_JOINT = {}
_MOMENTS = {}


def recording(c1, c2, frames, seed=0):
  """(eeg [frames, c1], feat [frames, c2]) float32: four AR(1) sources of unit variance at strengths STRENGTHS, mixed
  into both views by standard-normal matrices, plus white noise of 1.0 on the EEG and of 0.5 on the features.  The
  draws, in order: the sources' innovations [frames, 4], the EEG's mixing matrix and noise, the features'."""
  key = (c1, c2, frames, seed)
  if key not in _RECORDINGS:
    rng = np.random.default_rng(SEED + 31 * c1 + c2 + 7919 * seed)
    white = rng.standard_normal((frames, len(AR)))
    src = np.zeros_like(white)
    for j, a in enumerate(AR):
      src[0, j] = np.sqrt(1.0 - a * a) * white[0, j]             # (the recursion starts from rest)
      for t in range(1, frames):
        src[t, j] = a * src[t - 1, j] + np.sqrt(1.0 - a * a) * white[t, j]
    src *= np.asarray(STRENGTHS)[None, :]
    eeg = (src @ rng.standard_normal((len(AR), c1)) + rng.standard_normal((frames, c1))).astype(np.float32)
    feat = (src @ rng.standard_normal((len(AR), c2)) + 0.5 * rng.standard_normal((frames, c2))).astype(np.float32)
    eeg.setflags(write=False)
    feat.setflags(write=False)
    _RECORDINGS[key] = (eeg, feat)
  return _RECORDINGS[key]


def shape_recording(shape, seed=0):
  return recording(shape[0], shape[3], shape[6], seed)


def joint(shape, seed=0):
  """[lag_matrix(eeg) | lag_matrix(feat) | 1] of the whole recording in float64: (U [frames, n], X, Y)."""
  key = (tuple(shape), seed)
  if key not in _JOINT:
    c1, pre1, post1, c2, pre2, post2, frames = shape
    eeg, feat = recording(c1, c2, frames, seed)
    x = olag.lag_matrix(eeg.astype(np.float64), pre1, post1)
    y = olag.lag_matrix(feat.astype(np.float64), pre2, post2)
    _JOINT[key] = (np.hstack([x, y, np.ones((frames, 1))]), x, y)
  return _JOINT[key]


def reference_moments(shape, seed=0):
  """U^T U of the whole recording in float64."""
  key = (tuple(shape), seed)
  if key not in _MOMENTS:
    u = joint(shape, seed)[0]
    _MOMENTS[key] = u.T @ u
  return _MOMENTS[key]


def split_moments(m, k1, k2):
  """The four dense pieces in the layout of LagStats.moments: xtx (ones row / column last), x2tx2, xtx2, sum2."""
  n = k1 + k2 + 1
  x = np.r_[np.arange(k1), n - 1]
  return m[np.ix_(x, x)], m[k1:n - 1, k1:n - 1], m[:k1, k1:n - 1], m[k1:n - 1, n - 1]


def covariances(xtx, x2tx2, xtx2, sum2, lam, by_count=False):
  """(cov_xx, cov_yy, cov_xy, mean_x, mean_y) from the dense pieces, float64: the reference's normalisation
  (S / (count - 1) - mean^T mean, + lambda I on the auto-covariances) or, by_count, the plain covariance S / count -
  mean^T mean of the counted frames."""
  xtx, x2tx2, xtx2, sum2 = (np.asarray(a, np.float64) for a in (xtx, x2tx2, xtx2, sum2))
  k1, k2 = xtx.shape[0] - 1, x2tx2.shape[0]
  count = xtx[k1, k1]
  mx, my = xtx[k1, :k1] / count, sum2 / count
  denom = count if by_count else count - 1.0
  return (xtx[:k1, :k1] / denom - np.outer(mx, mx) + lam * np.eye(k1),
          x2tx2 / denom - np.outer(my, my) + lam * np.eye(k2), xtx2 / denom - np.outer(mx, my), mx, my)


def dense_stage(cxx, cyy, cxy, dim, eps=1e-12):
  """cca.py:345-367 with the symmetric LAPACK solver, float64 (tests/test_gpu_cca_solve.py: _numpy_dense_stage)."""
  def whiten(c):
    lam, v = np.linalg.eigh(c)
    keep = lam > eps
    return (v[:, keep] / np.sqrt(lam[keep])) @ v[:, keep].T
  k11, k22 = whiten(cxx), whiten(cyy)
  u, e, vt = np.linalg.svd(k11 @ cxy @ k22, full_matrices=False)
  return k11 @ u[:, :dim], k22 @ vt.T[:, :dim], e[:dim]


def gap_of(e):
  """The smallest gap between neighbouring canonical correlations, and from the last to 0."""
  return float(np.min(np.abs(np.diff(np.concatenate((np.asarray(e, np.float64), [0.0]))))))


def aligned(a, b, ra, rb):
  """Joint per-component sign of (rot_x[:, i], rot_y[:, i]) fixed against the reference."""
  sign = np.sign(np.sum(a * ra, axis=0) + np.sum(b * rb, axis=0))
  sign[sign == 0] = 1
  return a * sign, b * sign


def two_pass_statistics(x, y, mean_x, rot_x, mean_y, rot_y, weights=None):
  """{mean_a, mean_b, power} [3, dim] of the projections (x - mean_x) rot_x and (y - mean_y) rot_y in float64, two
  passes (the mean, then the centred squares): infer_decoder.Decoder._add_sums' values.  weights: per frame (the
  forgetting fit's g^age), else all ones."""
  f64 = lambda a: np.asarray(a, np.float64)
  a = (x - f64(mean_x).reshape(1, -1)) @ f64(rot_x)
  b = (y - f64(mean_y).reshape(1, -1)) @ f64(rot_y)
  w = np.ones((x.shape[0],)) if weights is None else f64(weights)
  total = np.sum(w)
  ma, mb = (w @ a) / total, (w @ b) / total
  va = (w @ ((a - ma) ** 2)) / total
  vb = (w @ ((b - mb) ** 2)) / total
  return np.stack([ma, mb, np.sqrt(va * vb)])


def rel(got, want):
  """The project's relative error: the largest difference over the largest magnitude (tests/test_gpu_fit.py)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def cuts(shape, seed=0):
  """{name: list of push sizes summing to frames}: ones, one row short of EACH view's tail (pre_v + delay - 1),
  sevens, random 0 .. 40, whole, and the whole recording with an empty push in the middle of two halves."""
  c1, pre1, post1, c2, pre2, post2, frames = shape
  delay = max(post1, post2)
  rng = np.random.default_rng(SEED + seed)

  def fill(size):
    size = max(1, size)
    return [size] * (frames // size) + ([frames % size] if frames % size else [])

  random = []
  while sum(random) < frames:
    random.append(int(min(rng.integers(0, 41), frames - sum(random))))
  half = frames // 2
  return {'ones': fill(1), 'tail1-1': fill(pre1 + delay - 1), 'tail2-1': fill(pre2 + delay - 1), 'sevens': fill(7),
          'random': random, 'whole': [frames], 'empty-middle': [half, 0, frames - half]}


def run(fit, eeg, feat, sizes_, flush_last=False, convert=None):
  """Walks one cut of (eeg [frames, c1] / [S, frames, c1], feat) through `fit` from a reset: every push in turn, then
  the flush on its own (an empty flushing push) -- or, flush_last, the last piece carried by the flush itself (a
  flushing last push).  convert: what turns a host piece into what push takes (a device tensor).  Returns the
  frames counted."""
  fit.reset()
  convert = convert or (lambda a: a)
  banked = len(eeg.shape) == 3                     # (host arrays or device tensors: both slice)
  at = 0
  for i, n in enumerate(sizes_):
    piece_e = convert(eeg[:, at:at + n] if banked else eeg[at:at + n])
    piece_f = convert(feat[:, at:at + n] if banked else feat[at:at + n])
    at += n
    if flush_last and i == len(sizes_) - 1:
      frames = fit.flush(piece_e, piece_f)
      assert frames == at == fit.frames
      return frames
    got = fit.push(piece_e, piece_f)
    assert got == max(0, at - fit.delay) == fit.frames
  frames = fit.flush()
  assert frames == at == fit.frames
  return frames


def make_fit(shape, **kwargs):
  from telluride_decoding_amd import online
  c1, pre1, post1, c2, pre2, post2 = shape[:6]
  return online.OnlineCCAFit(c1, pre1, post1, c2, pre2, post2, **kwargs)
