"""Shared by the online fit tests (CPU and GPU): white-noise recordings, the cuts of a recording into pushes, the
float64 references -- the moments of [oracle.lag.lag_matrix | 1] and np.linalg.solve of the reference's cov_x -- and a
driver that walks one cut through an online.OnlineRidgeFit.  Everything is computed once per key and shared: treat
what these functions return as read-only."""
import numpy as np

from oracle import lag as olag

SEED = 3407
FORGETS = (1.0, 0.99)
LAMBDAS = (1e-3, 0.1, 10.0)

_RECORDINGS = {}
_MOMENTS = {}


def recording(c, d, frames, seed=0):
  """(eeg [frames, c], target [frames, d]) float32 white noise, the target a little correlated with the EEG."""
  key = (c, d, frames, seed)
  if key not in _RECORDINGS:
    rng = np.random.default_rng(SEED + 7919 * seed + 31 * c + d)
    eeg = rng.standard_normal((frames, c)).astype(np.float32)
    mix = rng.standard_normal((c, d)) / np.sqrt(c)
    target = (0.5 * eeg.astype(np.float64) @ mix + rng.standard_normal((frames, d))).astype(np.float32)
    eeg.setflags(write=False)
    target.setflags(write=False)
    _RECORDINGS[key] = (eeg, target)
  return _RECORDINGS[key]


def lagged_ones(eeg, pre, post):
  """[oracle.lag.lag_matrix(eeg, pre, post) | 1] in float64: the reference's minibatch with its ones column."""
  x = olag.lag_matrix(np.asarray(eeg, np.float64), pre, post)
  return np.hstack([x, np.ones((x.shape[0], 1), np.float64)])


def reference_moments(c, pre, post, d, frames, seed=0):
  """(X^T X, X^T y) of the whole recording in float64, X = lagged_ones."""
  key = (c, pre, post, d, frames, seed)
  if key not in _MOMENTS:
    eeg, target = recording(c, d, frames, seed)
    x = lagged_ones(eeg, pre, post)
    _MOMENTS[key] = (x.T @ x, x.T @ target.astype(np.float64))
  return _MOMENTS[key]


def reference_solve(xtx, xty, count, lam):
  """np.linalg.solve of the reference's cov_x = xtx / n + lambda I (lambda on the bias entry too,
  brain_model.py:447-455, 477) and cov_xy = xty / n, float64: (W [K, d], b [d])."""
  n1 = xtx.shape[0]
  sol = np.linalg.solve(xtx / count + lam * np.identity(n1), xty / count)
  return sol[:-1], sol[-1]


def rel(got, want):
  """The project's relative error: the largest difference over the largest magnitude (tests/test_gpu_fit.py)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def cuts(frames, pre, post, seed=0):
  """{name: list of push sizes summing to frames}: ones, pre + post - 1, sevens, random 0 .. 40, whole, and the
  whole recording with an empty push in the middle of two halves."""
  rng = np.random.default_rng(SEED + seed)

  def fill(size):
    size = max(1, size)
    return [size] * (frames // size) + ([frames % size] if frames % size else [])

  random = []
  while sum(random) < frames:
    random.append(int(min(rng.integers(0, 41), frames - sum(random))))
  half = frames // 2
  return {'ones': fill(1), 'tail-1': fill(pre + post - 1), 'sevens': fill(7), 'random': random, 'whole': [frames],
          'empty-middle': [half, 0, frames - half]}


def run(fit, eeg, target, sizes, flush_last=False, convert=None):
  """Walks one cut of (eeg [frames, c] / [S, frames, c], target) through `fit` from a reset: every push in turn, then
  the flush on its own (an empty flushing push) -- or, flush_last, the last piece carried by the flush itself (a
  flushing last push).  convert: what turns a host piece into what push takes (a device tensor).  Returns the
  frames counted."""
  fit.reset()
  convert = convert or (lambda a: a)
  banked = len(eeg.shape) == 3                     # (host arrays or device tensors: both slice)
  at = 0
  for i, n in enumerate(sizes):
    piece_e = convert(eeg[:, at:at + n] if banked else eeg[at:at + n])
    piece_t = convert(target[:, at:at + n] if banked else target[at:at + n])
    at += n
    if flush_last and i == len(sizes) - 1:
      frames = fit.flush(piece_e, piece_t)
      assert frames == at == fit.frames
      return frames
    got = fit.push(piece_e, piece_t)
    assert got == max(0, at - fit.delay) == fit.frames
  frames = fit.flush()
  assert frames == at == fit.frames
  return frames
