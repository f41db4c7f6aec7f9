"""Host float64 restatement of AudioFeatures (the reference's preprocess.py:589-755), for the CPU tests
against G18 and the GPU tests: the intensity with its buffer, window indices and quirks (squares in
float32, means in float64), and the spectrogram as scipy's STFT recipe written out with numpy.fft.
Test infrastructure."""
import math

import numpy as np

# (name, fs_in, fs_out, window, exponent, channels, frames, streamed call lengths, user buffer rows)
INTENSITY_CASES = (
    ('i16', 16000, 100, 1, 1, 1, 16000, (3001, 1, 6998, 1, 5999), 0),
    ('i44', 44100, 100, 2.5, float(np.log10(2)), 2, 44100, (10000, 34100), 0),
    ('i48', 48000, 64, 3, 0.5, 2, 30000, (12345, 7, 17648), 160),
    ('i44m', 44100, 64, 1, 1, 1, 22050, (7000, 15050), 0),
    ('pass', 100, 100, 1, 1, 2, 300, (120, 2, 178), 0),
    ('passup', 100, 200, 1, 2, 1, 250, (100, 150), 3),
    ('nan', 100, 1000, 1.5, 1, 1, 50, (20, 30), 0),
)
# (name, samples, segment_size, n_overlap, n_trans, smoothing_filter); None: the reference's defaults
SPECTROGRAM_CASES = (
    ('default', 800, None, None, None, None),
    ('reftest', 16000, 128, 2, 2, (1,)),
    ('s256', 1500, 256, 4, 2, None),
    ('s100', 1500, 100, 3, 3, (.5, .5)),
    ('short120', 120, None, None, None, None),
    ('zeros', 1000, None, None, None, None),
)
# G18 keeps every COLUMN_STEP-th frame of a spectrogram wider than this many frames (the golden stays small)
GOLDEN_MAX_FRAMES, COLUMN_STEP = 64, 5
SPECTROGRAM_RAISES = (('short50', 50),)


def _sweep_taps(n):
  return tuple(0.1 + 0.9 * ((7 * j) % 11) / 10.0 for j in range(n))


# The spectrogram kernels' tile edges, for the GPU sweep and the scipy cross-check of `spectrogram`:
# (name, samples, segment_size, n_overlap, n_trans, smoothing_filter); None: the reference's default filter.
# The DFT runs 64 frames per workgroup, 16 bins per wave, 4 waves per workgroup and 64-sample LDS stages; the
# FIR 16 x 64 tiles with a (taps - 1) halo.  Comments: (seg, hop, nfft, bins, frames).
SPECTROGRAM_SWEEP = (
    ('seg1', 65, 1, 4, 2, None),                    # (1, 1, 2, 2, 65)
    ('seg2', 64, 2, 4, 2, None),                    # (2, 1, 4, 3, 65)
    ('seg63', 1010, 63, 4, 2, None),                # (63, 16, 126, 64, 65): all four waves of one group
    ('seg64', 1009, 64, 4, 2, None),                # (64, 16, 128, 65, 65)
    ('seg65', 1073, 65, 4, 2, None),                # (65, 17, 130, 66, 65)
    ('seg127', 2018, 127, 4, 2, None),              # (127, 32, 254, 128, 65)
    ('seg129', 2081, 129, 4, 2, None),              # (129, 33, 258, 130, 65)
    ('seg1023', 16130, 1023, 4, 2, None),           # (1023, 256, 2046, 1024, 65)
    ('frames2', 2, 2, 1, 2, None),                  # (2, 2, 4, 3, 2): no wave gives one frame (1 sample raises)
    ('frames63', 977, 64, 4, 2, None),              # (64, 16, 128, 65, 63)
    ('frames64', 993, 64, 4, 2, None),              # (64, 16, 128, 65, 64)
    ('frames129', 2033, 64, 4, 2, None),            # (64, 16, 128, 65, 129)
    ('seg1_frames129', 129, 1, 1, 3, None),         # (1, 1, 3, 2, 129)
    ('bins5', 500, 8, 2, 1, None),                  # (8, 4, 8, 5, 126)
    ('bins16', 600, 15, 3, 2, None),                # (15, 5, 30, 16, 121)
    ('bins17', 600, 16, 4, 2, None),                # (16, 4, 32, 17, 151)
    ('bins32', 700, 31, 2, 2, None),                # (31, 16, 62, 32, 45)
    ('bins33', 700, 32, 2, 2, None),                # (32, 16, 64, 33, 45)
    ('bins256', 3000, 255, 4, 2, None),             # (255, 64, 510, 256, 48)
    ('hop1_s64', 300, 64, 64, 2, None),             # (64, 1, 128, 65, 301)
    ('hop1_s37', 200, 37, 37, 3, None),             # (37, 1, 111, 56, 200)
    ('hopseg_s1', 100, 1, 1, 2, None),              # (1, 1, 2, 2, 100)
    ('hopseg_s64', 3000, 64, 1, 2, None),           # (64, 64, 128, 65, 48)
    ('hopseg_s100', 3000, 100, 1, 3, None),         # (100, 100, 300, 151, 31)
    ('ntrans1_s128', 2000, 128, 8, 1, None),        # (128, 16, 128, 65, 126): nfft == seg
    ('ntrans1_s129', 2081, 129, 4, 1, None),        # (129, 33, 129, 65, 65): odd nfft == seg
    ('ntrans3_s64', 1009, 64, 4, 3, None),          # (64, 16, 192, 97, 65)
    ('ntrans3_s65', 1073, 65, 4, 3, None),          # (65, 17, 195, 98, 65): odd nfft
    ('ntrans4_s33', 800, 33, 2, 4, None),           # (33, 17, 132, 67, 48)
    ('ntrans3_s1023', 9000, 1023, 2, 3, (1,)),      # (1023, 512, 3069, 1535, 19): odd nfft, 24 k groups
    ('s1024_nfft4096_hop1', 1500, 1024, 1024, 4, None),   # (1024, 1, 4096, 2049, 1501)
    ('short70', 70, 128, 2, 2, None),               # (70, 6, 256, 129, 13): seg shrunk to the wave
    ('short127', 127, 128, 2, 2, None),             # (127, 63, 256, 129, 3)
    ('short1000', 1000, 1024, 2, 4, None),          # (1000, 488, 4096, 2049, 4)
    ('negtaps', 1009, 64, 4, 2, (1, -2, .5)),       # (64, 16, 128, 65, 65): negative power, NaN everywhere
    ('negtaps_one', 1009, 64, 4, 2, (-1,)),
    ('negtaps_mild', 1009, 64, 4, 2, (1, -0.02)),   # some cells below -off: NaN everywhere too
) + tuple(('taps%d' % n, 2033, 64, 4, 2, _sweep_taps(n)) for n in range(1, 17))   # (64, 16, 128, 65, 129)


def sweep_case(name):
  """(wave, kwargs of compute_spectrogram) of SPECTROGRAM_SWEEP's case `name`."""
  _, samples, seg, n_overlap, n_trans, taps = next(c for c in SPECTROGRAM_SWEEP if c[0] == name)
  kw = dict(segment_size=seg, n_overlap=n_overlap, n_trans=n_trans)
  if taps is not None:
    kw['smoothing_filter'] = taps
  return spectrogram_input(name, samples), kw


def gaussian(m, std):
  """scipy.signal.windows.gaussian(m, std)."""
  n = np.arange(m) - (m - 1.0) / 2.0
  return np.exp(-n ** 2 / (2 * std * std))


def tone_440():
  """The reference test's input (preprocess_test.py:289-308): a Gaussian-windowed 440 Hz tone, 1 s at 16 kHz."""
  window = gaussian(16000, 16000 / 4.0).reshape(-1, 1)
  t = np.linspace(0, 1, 16000).reshape(-1, 1)
  return np.sin(2 * np.pi * t * 440) * window, window


def tone_6000():
  """The reference's spectrogram test input (preprocess_test.py:310-333)."""
  window = gaussian(16000, 16000 / 4.0)
  t = np.linspace(0, 1, 16000)
  return np.sin(2 * np.pi * t * 6000) * window


def windows_loop(frames_in, tau, rows, fs_in, fs_out, window):
  """The reference's window bounds, Python floats in its order (preprocess.py:657-661)."""
  hw = 0.5 * window / fs_out
  out = np.empty((rows, 2), np.int64)
  for i in range(rows):
    t = float(i) / fs_out
    out[i, 0] = int(max(0, round(fs_in * (t - hw)) + tau))
    out[i, 1] = int(min(frames_in, round(fs_in * (t + hw)) + tau))
  return out


def windows_vec(frames_in, tau, rows, fs_in, fs_out, window):
  """The same with numpy's rint (half-even, as Python's round of a float)."""
  hw = 0.5 * window / fs_out
  t = np.arange(rows, dtype=np.float64) / fs_out
  t1 = np.maximum(0, np.rint(fs_in * (t - hw)).astype(np.int64) + tau)
  t2 = np.minimum(frames_in, np.rint(fs_in * (t + hw)).astype(np.int64) + tau)
  return np.stack([t1, t2], axis=1)


def window_means(data, windows):
  """Row i: the float64 mean of data[t1_i:t2_i] (NaN when empty)."""
  out = np.full((windows.shape[0], data.shape[1]), np.nan)
  for i, (t1, t2) in enumerate(windows):
    if t2 > t1:
      out[i] = np.sum(data[t1:t2].astype(np.float64), axis=0) / (t2 - t1)
  return out


def window_means_exact(data, windows):
  """Row i: the mean of data[t1_i:t2_i] with the window's sum exact, rounded once (NaN when empty).
  Integer-valued data (float32 squares of integers are) take int64 prefix sums; other data math.fsum per
  window and channel, on shapes small enough to afford it.  A window holding an inf or a NaN takes numpy's
  sum, which is then exact too (inf, -inf or NaN)."""
  data = np.asarray(data, np.float64)
  windows = np.asarray(windows, np.int64)
  n, c = data.shape
  out = np.full((windows.shape[0], c), np.nan)
  full = windows[:, 1] > windows[:, 0]
  t1, t2 = windows[full, 0], windows[full, 1]
  finite = np.isfinite(data)
  if finite.all() and np.array_equal(data, np.round(data)) and (
      n == 0 or float(np.max(np.abs(data), initial=0.0)) * (n + 1) < 2.0 ** 62):
    cs = np.zeros((n + 1, c), np.int64)
    np.cumsum(data.astype(np.int64), axis=0, out=cs[1:])
    out[full] = (cs[t2] - cs[t1]).astype(np.float64) / (t2 - t1)[:, None]
    return out
  bad = np.zeros((n + 1, c), np.int64)
  np.cumsum(~finite, axis=0, out=bad[1:])
  for i, a, b in zip(np.flatnonzero(full), t1, t2):
    for j in range(c):
      col = data[a:b, j]
      s = math.fsum(col) if bad[b, j] == bad[a, j] else float(np.sum(col))
      out[i, j] = s / (b - a)
  return out


class HostAudioFeatures(object):
  """compute_intensity / audio_resample with the reference's buffer, in float64."""

  def __init__(self, fs_in, fs_out, window=1, exponent=1, buff=None, exact=False):
    """exact: window sums exact (window_means_exact) rather than summed row after row (window_means)."""
    self.fs_in, self.fs_out, self.window, self.exponent = fs_in, fs_out, window, exponent
    self.buff = None if buff is None else np.asarray(buff)
    self.means = window_means_exact if exact else window_means
    self.windows = None           # the last windowed call's (t1, t2) rows

  def _resample(self, data, square):
    data = np.asarray(data)
    if square:
      data = data.astype(np.float32)
    if data.ndim <= 1:
      data = data.reshape(-1, 1)
    if data.shape[1] > data.shape[0]:
      data = data.T
    if square:
      data = data * data                       # float32 squares
    if self.buff is not None:
      data = np.concatenate((self.buff, data), axis=0)
      tau = self.buff.shape[0]
    else:
      tau = 0
    hw = 0.5 * self.window / self.fs_out
    self.buff = data[-int(self.fs_in * hw):, :]
    frames_in = data.shape[0]
    rows = int(round((frames_in - tau) / self.fs_in * self.fs_out))
    if not (self.fs_out < self.fs_in or self.window > 1):
      return (data ** 0.5) ** self.exponent if square else data
    bounds = windows_vec if self.means is window_means_exact else windows_loop   # (equal: a CPU test)
    self.windows = bounds(frames_in, tau, rows, self.fs_in, self.fs_out, self.window)
    out = self.means(data, self.windows)
    return np.sqrt(out) ** self.exponent if square else out

  def audio_resample(self, data):
    return self._resample(data, False)

  def compute_intensity(self, data):
    return self._resample(data, True)


def spectrogram_shape(n, segment_size=128, n_overlap=8, n_trans=4):
  """(seg, hop, nfft, frames) after scipy's checks; raises ValueError as scipy does."""
  seg = min(int(segment_size), n)
  nfft = int(segment_size * n_trans)
  noverlap = int(segment_size - segment_size / n_overlap)
  if noverlap >= seg:
    raise ValueError('noverlap must be less than nperseg.')
  hop = seg - noverlap
  padded = n + 2 * (seg // 2)
  padded += (-(padded - seg) % hop) % seg
  return seg, hop, nfft, (padded - seg) // hop + 1


def lfilter_fir(b, x, axis):
  """scipy.signal.lfilter(b, [1], x, axis) (zero initial state)."""
  x = np.moveaxis(np.asarray(x, np.float64), axis, 0)
  y = np.zeros_like(x)
  for j, bj in enumerate(b):
    y[j:] += bj * x[:x.shape[0] - j]
  return np.moveaxis(y, 0, axis)


def spectrogram(wave, segment_size=128, n_overlap=8, n_trans=4, smoothing_filter=(.2, 1, .2)):
  """compute_spectrogram restated: (spectrogram [K, T] float64, frequencies)."""
  w = np.squeeze(wave).astype(np.float32).astype(np.float64)
  seg, hop, nfft, frames = spectrogram_shape(w.shape[0], segment_size, n_overlap, n_trans)
  pe = w.copy()
  pe[1:] = w[1:] - 0.95 * w[:-1]
  pad = seg // 2
  total = (frames - 1) * hop + seg
  xp = np.zeros(max(total, w.shape[0] + 2 * pad))
  xp[pad:pad + w.shape[0]] = pe
  win = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(seg) / seg)
  idx = np.arange(frames)[:, None] * hop + np.arange(seg)[None, :]
  spec = np.fft.rfft(xp[idx] * win / win.sum(), n=nfft, axis=1).T
  p = np.real(spec * np.conj(spec))
  p = lfilter_fir(smoothing_filter, p, 0)
  p = lfilter_fir(smoothing_filter, p, 1)
  with np.errstate(invalid='ignore', divide='ignore'):
    off = 0.0001 * np.max(p)
    s = (off + p) ** 0.25 - off ** 0.25
    s = 255 / np.max(s) * s
  return s, np.fft.rfftfreq(nfft, 1.0)


def intensity_input(name, fs_in, channels, frames):
  """A case's integer-valued input (exact in int16, float32 and float64): uniform integer noise under a slow
  triangular envelope.  Integer draws and IEEE arithmetic only, so every platform makes the same samples."""
  rng = np.random.default_rng(sum(map(ord, name)))
  t = np.arange(frames)[:, None] / fs_in
  phase = (1.3 * t + 0.16 * np.arange(channels)) % 1.0
  env = 1.0 + 0.8 * (4.0 * np.abs(phase - 0.5) - 1.0)
  return np.round(env * rng.integers(-6000, 6001, size=(frames, channels)))


def case_input(g18, name):
  """Intensity case `name`'s input, regenerated and checked against the checksums G18 stores."""
  c = next(c for c in INTENSITY_CASES if c[0] == name)
  x = intensity_input(name, c[1], c[5], c[6])
  np.testing.assert_array_equal(checksum(x), g18[name + '_xsum'])
  return x


def checksum(x):
  x = np.asarray(x, np.float64)
  return np.array([x.sum(), (x * x).sum(), np.abs(x).max() if x.size else 0.0])


def golden_columns(frames):
  """The frames G18 keeps of a spectrogram with `frames` frames."""
  return np.arange(frames) if frames <= GOLDEN_MAX_FRAMES else np.arange(0, frames, COLUMN_STEP)


def case_wave(g18, name):
  """Spectrogram case `name`'s wave, regenerated and checked against G18's checksums (to float64 rounding:
  np.sin may differ in the last place between platforms)."""
  samples = next(c for c in SPECTROGRAM_CASES if c[0] == name)[1]
  wave = spectrogram_input(name, samples)
  np.testing.assert_allclose(checksum(wave), g18['spec_%s_xsum' % name], rtol=1e-12, atol=1e-9)
  return wave


def spectrogram_input(name, samples):
  if name == 'reftest':
    return tone_6000()
  if name == 'zeros':
    return np.zeros(samples)
  rng = np.random.default_rng(sum(map(ord, name)))
  t = np.arange(samples) / 16000.0
  return np.sin(2 * np.pi * 440 * t) * (1 + np.sin(2 * np.pi * 3 * t)) + 0.3 * rng.standard_normal(samples)
