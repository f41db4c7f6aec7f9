"""Inputs and host restatements for the ingest tests (tests/test_cpu_ingest.py, tests/test_gpu_ingest.py) and for
tests/golden/make_ingest.py, which runs the reference on the same inputs and stores what it returns in G19.
Every input is regenerated here from a seed; G19 keeps only checksums of them.  Test infrastructure."""
import math

import numpy as np


def checksum(x):
  x = np.asarray(x, np.float64)
  return np.array([x.sum(), (x * x).sum(), np.abs(x).max() if x.size else 0.0])


def _rng(name):
  return np.random.default_rng(sum(map(ord, name)) + 19)


# ---------------------------------------------------------------- host functions: inputs
def close_times_cases():
  """{name: (times, min_time)}; 'reftest' is the reference test's literal."""
  onsets = np.array([1.1, 2.4, 3.5, 6.7, 25.8, 30.4, 87.2, 90.2])
  rng = _rng('close')
  base = np.cumsum(0.5 + rng.random(40))
  noisy = np.concatenate((base, base + 0.05, base[::3] + 0.09))
  return {'reftest': (np.sort(np.concatenate((onsets, onsets + 0.1))), 0.2),
          'default': (rng.permutation(noisy), 0.06),
          'single': (np.array([4.25]), 0.06)}


def regression_cases():
  """{name: (audio times, eeg times)}; 'reftest' is the reference test's literal."""
  audio = np.arange(0, 5, 1)
  eeg = audio + 1.3
  eeg[0] = math.pi
  rng = _rng('regress')
  a2 = np.cumsum(1.0 + rng.random(25))
  e2 = a2 + 0.73 + 0.002 * rng.standard_normal(25)
  e2[[3, 11]] += 0.5
  return {'reftest': (audio, eeg), 'jitter': (a2, e2[:23])}


def histogram_cases():
  """{name: (audio triggers, eeg triggers, max_time, fs)}: fs = 0, fs > 0 (the reference test's, seeded), and
  with max_time."""
  rng = _rng('hist')
  a = rng.random(10)
  e = a + 1.42
  samples = np.sort(rng.integers(0, 5000, 12))
  return {'reftest': (a, e, 0, 100),
          'samples': (samples, np.concatenate((samples[2:] + 37, [11, 4999])), 0, 0),
          'maxtime': (np.concatenate((a, [7.5])), np.concatenate((e, [0.2, 0.21, 0.22])), 2.0, 100)}


def pulse_train():
  """(stereo sound [n, 2] float64 with trigger pulses in channel 1, its sample rate)."""
  fs, n = 8000, 20000
  rng = _rng('pulse')
  sound = np.zeros((n, 2))
  sound[:, 0] = rng.standard_normal(n)
  for start in (0, 1200, 1203, 6000, 15555, 19999):
    sound[start:start + 2, 1] = 0.5
  sound[9000:9004, 1] = -0.25         # (a negative pulse is no trigger)
  return sound, fs


def natus_signal():
  """(raw Natus trigger channel [n] whose corrected byte codes carry events in the low bit, its sample rate)."""
  sr, n = 512, 4000
  codes = np.full(n, 4.0)
  for start, width in ((100, 30), (700, 51), (701 + 51, 20), (2500, 1), (3990, 10)):
    codes[start:start + width] += 1.0
  codes[1500:1600] += 2.0             # (another bit: no event)
  raw = 5151600.0 - (codes + 32768.0) / 0.0063606452364314
  return raw, sr


def fix_offset_cases():
  """[(signal, sample rate, offset seconds)]"""
  return [(np.arange(10), 4, 1), (np.arange(40).reshape(20, 2), 4, 0.3), (np.arange(7.0), 3, 0),
          (np.arange(30).reshape(10, 3), 2.5, 1.9)]


def assemble_channels():
  """(ordered [(name, data)] of uneven lengths and widths, sample rate, the request -- in another order)."""
  rng = _rng('assemble')
  chans = [('TRIG', rng.integers(0, 9, 57)), ('Fp2', rng.standard_normal(60)),
           ('pair', rng.standard_normal((55, 2))), ('unused', rng.standard_normal(70)),
           ('O1', rng.standard_normal(58).astype(np.float32))]
  return chans, 64, ['O1', 'pair', 'TRIG', 'Fp2']


def adjust_inputs():
  rng = _rng('adjust')
  return {'eeg': rng.standard_normal((103, 4)).astype(np.float32), 'intensity': rng.standard_normal(100),
          'spectrogram': rng.standard_normal((101, 6))}


def memory_experiment_inputs():
  """The reference's test_brain_memory_experiment, seeded: (audio [2 fs, 1], fs, {C1, C2}, frame rate)."""
  fs, frame_sr = 16000, 100
  audio = _rng('memexp').standard_normal((2 * fs, 1))
  return audio, fs, [('C1', np.arange(2 * frame_sr)), ('C2', np.arange(2 * frame_sr) + 200)], frame_sr


# ---------------------------------------------------------------- moments
def moments_data(name, rows_list, width, dtype, base=1e4):
  """[rows_i, width] arrays drawn as offset + N(0, 1) per column, the offsets base * 100^(column % 3): EEG with
  a DC offset, on which a one-pass sum of squares cancels."""
  rng = _rng('moments' + name)
  offsets = base * 100.0 ** (np.arange(width) % 3)
  return [(offsets + rng.standard_normal((rows, width))).astype(dtype) for rows in rows_list]


def moments_truth(arrays, columnwise):
  """(mean, std) by two passes in np.longdouble with math.fsum for the sums: the ground truth."""
  cols = [np.concatenate([np.asarray(a, np.float64)[:, c] for a in arrays]) for c in range(arrays[0].shape[1])]
  if not columnwise:
    cols = [np.concatenate(cols)]
  means, stds = [], []
  for x in cols:
    mean = np.longdouble(math.fsum(x)) / np.longdouble(x.size)
    d = x.astype(np.longdouble) - mean
    sq = (d * d)
    # fsum of the float64 heads and tails of the long double squares
    head = sq.astype(np.float64)
    tail = (sq - head.astype(np.longdouble)).astype(np.float64)
    total = np.longdouble(math.fsum(head)) + np.longdouble(math.fsum(tail))
    means.append(float(mean))
    stds.append(float(np.sqrt(total / np.longdouble(x.size))))
  if columnwise:
    return np.array(means).reshape(1, -1), np.array(stds).reshape(1, -1)
  return means[0], stds[0]


# (name, rows of each array, width, dtype): the reference's find_mean_std on these is stored in G19
G19_MOMENT_CASES = (('m32', (63, 1025), 3, 'float32'), ('m64', (1, 63, 4097), 64, 'float64'),
                    ('m32w', (1025, 63, 1, 4097, 63), 148, 'float32'), ('m1', (4097,), 1, 'float32'))


# ---------------------------------------------------------------- encoder inputs
F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001,
                         0xffbfffff, 0x00000001, 0x807fffff, 0x00400000, 0x7f7fffff, 0x3f800000],
                        np.uint32).view(np.float32)
# overflow, exactly half way between two float32 (ties to even, both directions), just above and below a tie,
# results that are float32 denormals (with ties), below half the smallest denormal, the largest finite float32
F64_EDGES = np.array([1e39, -1e39, 3.5e38, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50,
                      1.0 + 2.0 ** -24 - 2.0 ** -53, 2.0 ** -140 * (1 + 2.0 ** -10), 2.0 ** -149 * 1.5,
                      2.0 ** -149 * 2.5, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -40), 2.0 ** -151, -2.0 ** -127,
                      float(np.finfo(np.float32).max), float(np.finfo(np.float32).max) * (1 + 2.0 ** -25),
                      float(np.finfo(np.float32).max) * (1 + 2.0 ** -24), np.inf, -np.inf, np.nan, 0.0, -0.0,
                      5e-324, 1e-310], np.float64)


def fill_bits(shape, dtype, seed, specials=True):
  """Random finite values of `dtype` with the special patterns above cycled through the first entries."""
  rng = np.random.default_rng(seed)
  n = int(np.prod(shape))
  x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dtype)
  if specials:
    pool = F32_SPECIALS if np.dtype(dtype) == np.float32 else F64_EDGES
    k = min(n, len(pool))
    x[:k] = pool[:k]
  return x.reshape(shape)


def same_bits(a, b):
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ulp_distance32(a, b):
  """Elementwise distance of two float32 arrays in units in the last place (on the ordered integer line)."""
  def key(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)
  return np.abs(key(a) - key(b))
