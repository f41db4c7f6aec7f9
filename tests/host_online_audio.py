"""Shared by tests/test_cpu_online_audio.py and tests/test_gpu_online_audio.py: the rate / window cases of the online
audio front end, its recordings (seeded int16 draws: every float32 square is an integer, so every window sum is exact
in float64), the cuts a cut-invariance test walks, td_audio_online_plan restated by counting, and the oracle
(tests/host_audio.HostAudioFeatures(exact=True).compute_intensity on the whole recording).  Test infrastructure."""
import math

import numpy as np

from tests import host_audio as ha

ROWS = 3000
LOG10_2 = float(np.log10(2))

# (fs_in, fs_out, window): the plan's cases
PLAN_CASES = [(16000, 64, w) for w in (0.1, 0.5, 1, 1.5, 3, 7.3)] + [
    (44100, 100, 1), (44100, 100, 2), (6400, 100, 1), (6300, 100, 1), (6500, 100, 1), (1000, 100, 0.5),
    (100, 64, 0.1), (64, 100, 1.5), (100, 100, 3), (3, 2, 1)]
PLAN_IDS = ['%d_to_%d_w%g' % case for case in PLAN_CASES]


def tail_rows(fs_in, fs_out, window):
  """K as the issue states it: ceil((window / 2 + max(window / 2, 0.5)) fs_in / fs_out) + 2."""
  half = 0.5 * window
  return int(math.ceil((half + max(half, 0.5)) * fs_in / fs_out)) + 2


def frames_of(rows, fs_in, fs_out):
  return int(round(rows / fs_in * fs_out))


def brute_emitted(rows, fs_in, fs_out, window, flush=False):
  """The frames emitted once `rows` rows are pushed, by counting over the whole recording's windows (windows_loop
  with no clamp at the end): frame i needs u_i <= rows and i < F(rows); a flush emits every i < F(rows)."""
  total = frames_of(rows, fs_in, fs_out)
  if flush or total == 0:
    return total
  upper = ha.windows_loop(1 << 62, 0, total, fs_in, fs_out, window)[:, 1]
  return int(np.sum(upper <= rows))


def raw_window(i, fs_in, fs_out, window):
  """(a_i, u_i), unclamped, in the reference's order."""
  hw = 0.5 * window / fs_out
  t = float(i) / fs_out
  return int(round(fs_in * (t - hw))), int(round(fs_in * (t + hw)))


_RECORDINGS = {}


def recording(c, dtype='int16', seed=0, sessions=None):
  """ROWS rows of c channels of seeded int16 draws over the whole range, as `dtype`; computed once and shared:
  read-only."""
  key = (c, np.dtype(dtype).name, seed, sessions)
  if key not in _RECORDINGS:
    rng = np.random.default_rng(1000 * c + seed)
    shape = (ROWS, c) if sessions is None else (sessions, ROWS, c)
    x = rng.integers(-32768, 32768, size=shape).astype(np.int16).astype(dtype)
    x.setflags(write=False)
    _RECORDINGS[key] = x
  return _RECORDINGS[key]


def noise(c, seed=0):
  """ROWS rows of float32 that are no integers: noise under a slow envelope."""
  key = ('noise', c, seed)
  if key not in _RECORDINGS:
    rng = np.random.default_rng(77 + 10 * c + seed)
    t = np.arange(ROWS, dtype=np.float64)[:, None] / ROWS
    x = ((0.2 + np.abs(np.sin(2 * np.pi * (3 * t + 0.1 * np.arange(c))))) * rng.standard_normal((ROWS, c)))
    x = x.astype(np.float32)
    x.setflags(write=False)
    _RECORDINGS[key] = x
  return _RECORDINGS[key]


def cuts(total, k, seed=0):
  """{name: (push sizes summing to total, flush as a call of its own)}: one push; one-row pushes; 1, 63, 64, 65,
  K - 1, K, K + 1 and the rest; a seeded random cut with empty pushes; the flush with the last push and apart."""
  rng = np.random.default_rng(seed)
  head = [1, 63, 64, 65, k - 1, k, k + 1]
  while sum(head) >= total:
    head.pop(int(np.argmax(head)))
  random = []
  while sum(random) < total:
    random.append(int(min(rng.integers(0, 401) * (rng.random() > 0.25), total - sum(random))))
  random.insert(1, 0)
  return {'whole': ([total], False), 'whole_flush_apart': ([total], True), 'ones': ([1] * total, True),
          'edges': (head + [total - sum(head)], False), 'edges_flush_apart': (head + [total - sum(head)], True),
          'random': (random, True), 'random_flush_with': (random, False)}


def oracle(x, fs_in, fs_out, window, exponent):
  """HostAudioFeatures(exact=True).compute_intensity(whole) on a fresh object: (frames [F, c] float64, the windows
  [F, 2] int64)."""
  h = ha.HostAudioFeatures(fs_in, fs_out, window, exponent, exact=True)
  x = np.asarray(x)
  assert x.shape[0] >= x.shape[1]              # (the batch transpose rule stays out of it)
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    out = h.compute_intensity(x)
  return out, h.windows


def features(fs_in, fs_out, window, exponent=1):
  from telluride_decoding_amd import preprocess
  return preprocess.AudioFeatures('audio', fs_in, fs_out, window, exponent)


def run_audio(obj, x, sizes, flush_apart=True):
  """x [n, c] (or [S, n, c]) through an online.OnlineAudioFeatures in pushes of `sizes`, flushed with the last push's
  successor (flush_apart) -- the object has no flushing push --: (out32, out64) along the frames, host arrays."""
  x3 = x if x.ndim == 3 else x[None]
  outs, at = [], 0
  for n in sizes:
    outs.append(obj.push(x3[:, at:at + n] if x.ndim == 3 else x[at:at + n], want64=True))
    at += n
  assert at == x3.shape[1]
  outs.append(obj.flush(want64=True))
  host = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else a
  return (np.concatenate([host(o[0]) for o in outs], axis=1), np.concatenate([host(o[1]) for o in outs], axis=1))
