"""Shared by tests/test_cpu_online_pre.py and tests/test_gpu_online_pre.py: the recording of the front end's
comparisons (the recipe of tests/test_gpu_preprocess_sweep.signal), its configurations, the cuts of a recording a
cut-invariance test walks, a brute-force count of what a push emits, and the oracle (tests/host_preprocess's
HostPreprocessor on the whole recording).  Test infrastructure."""
import numpy as np

from tests import host_preprocess as hp

ROWS = 3000


def signal(n, c, seed, offset=2.0, fs=1000.0):
  """DC offset + slow drift + white noise, float64 (tests/test_gpu_preprocess_sweep.signal's recipe)."""
  rng = np.random.default_rng(seed)
  t = np.arange(n, dtype=np.float64)[:, None] / fs
  return offset + 0.5 * np.sin(2 * np.pi * 0.05 * t + np.arange(c)) + rng.standard_normal((n, c))


_SIGNALS = {}


def recording(c, fs, dtype=np.float32):
  """The 3000 raw rows of a case, computed once and shared: read-only."""
  key = (c, float(fs), np.dtype(dtype).name)
  if key not in _SIGNALS:
    _SIGNALS[key] = signal(ROWS, c, seed=c, fs=fs).astype(dtype)
    _SIGNALS[key].setflags(write=False)
  return _SIGNALS[key]


# sections: 0, 1 (high-pass only), 2 (low-pass only), 7 (the split in the middle) and 16
FILTERS = {
    0: dict(),
    1: dict(highpass_cutoff=0.5, highpass_order=1),
    2: dict(lowpass_cutoff=30, lowpass_order=3),
    7: dict(highpass_cutoff=0.5, highpass_order=4),          # + the automatic low-pass (order 10) when downsampling
    16: dict(highpass_cutoff=0.5, highpass_order=15, lowpass_cutoff=30, lowpass_order=15),
}
HARD = dict(fs_in=1000, fs_out=1000, highpass_cutoff=0.01, highpass_order=16, lowpass_cutoff=1, lowpass_order=16)


def config(sections, fs_in, fs_out, c, **more):
  """Preprocessor keyword arguments of a case: the filter of `sections` sections, a global re-reference on the
  channels but the last, every other channel (from channel 1 when there are two), mean 0.25, std 1.5."""
  kw = dict(fs_in=fs_in, fs_out=fs_out, data_mean=0.25, data_std=1.5, **FILTERS[sections])
  if sections == 7 and fs_out >= fs_in:
    kw.update(lowpass_cutoff=0.375 * fs_out, lowpass_order=10)
  if c >= 3:
    kw.update(ref_channels=[list(range(c))], channels_to_ref=[list(range(c - 1))],
              channel_numbers=list(range(1, c, 2)))
  kw.update(more)
  return kw


def make(kw):
  from telluride_decoding_amd import preprocess
  kw = dict(kw)
  return preprocess.Preprocessor('front', kw.pop('fs_in'), kw.pop('fs_out'), **kw)


def sections_of(kw):
  sos = make(kw).sos
  return 0 if sos is None else int(sos.shape[0])


def cuts(total, seed=0):
  """{name: (push sizes summing to total, flush as a call of its own)}."""
  rng = np.random.default_rng(seed)
  head = [1, 7, 9, 10, 11, 63, 64, 65, 500]
  random = []
  while sum(random) < total:
    random.append(int(min(rng.integers(0, 401) * (rng.random() > 0.25), total - sum(random))))
  random.insert(1, 0)
  return {'whole': ([total], False), 'whole_flush_apart': ([total], True), 'ones': ([1] * total, True),
          'edges': (head + [total - sum(head)], False), 'random': (random, True), 'random_flush_with': (random, False)}


QUICK_CUTS = ('whole', 'edges', 'random')


def brute_frames(rows, fs_in, fs_out, flush):
  """The frames emitted once `rows` rows are pushed, by counting: frame j needs its row r_j among the rows pushed
  and j < F(rows); a flush emits every j < F(rows)."""
  if fs_in == fs_out:
    return rows
  total = int(np.round(float(rows) / fs_in * fs_out))
  if flush or total == 0:
    return total
  r = np.round(np.arange(total) * (1.0 / fs_out) * fs_in)
  return int(np.sum(r <= rows - 1))


def oracle(kw, x):
  """HostPreprocessor(kw).process(whole, reset=True): (output float64, its filter state [S, 2, C] or None)."""
  h = hp.HostPreprocessor(kw)
  out = h.process(np.asarray(x), reset=True)
  return out, h.state()


def run_front(front, x, sizes, want64=True):
  """x [n, C] (or [S, n, C]) through an online.OnlinePreprocessor in pushes of `sizes`, the last one followed by
  a flush: (out32, out64) concatenated along the frames, as host arrays."""
  x3 = x if x.ndim == 3 else x[None]
  outs, at = [], 0
  for n in sizes:
    outs.append(front.push(x3[:, at:at + n] if x.ndim == 3 else x[at:at + n], want64=want64))
    at += n
  assert at == x3.shape[1]
  outs.append(front.flush(want64=want64))
  host = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else a
  if want64:
    return (np.concatenate([host(o[0]) for o in outs], axis=1), np.concatenate([host(o[1]) for o in outs], axis=1))
  return np.concatenate([host(o) for o in outs], axis=1)
