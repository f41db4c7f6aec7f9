"""Host float64 restatement of AudioFeatures (the reference's preprocess.py:589-755), for the CPU tests
against G18 and the GPU tests: the intensity with its buffer, window indices and quirks (squares in
float32, means in float64), and the spectrogram as scipy's STFT recipe written out with numpy.fft.
Test infrastructure."""
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


class HostAudioFeatures(object):
  """compute_intensity / audio_resample with the reference's buffer, in float64."""

  def __init__(self, fs_in, fs_out, window=1, exponent=1, buff=None):
    self.fs_in, self.fs_out, self.window, self.exponent = fs_in, fs_out, window, exponent
    self.buff = None if buff is None else np.asarray(buff)

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
    out = window_means(data, windows_loop(frames_in, tau, rows, self.fs_in, self.fs_out, self.window))
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
