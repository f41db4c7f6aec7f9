"""GPU parity of the AudioFeatures drop-in (csrc/audio.hip through telluride_decoding_amd.preprocess) against
the reference's own outputs (G18) and the host float64 restatement (tests/host_audio.py).
Bounds: intensity within 1e-12 x max of the restatement and 2e-6 x max of the reference (whose means are
float32); spectrogram within 1e-9 on the 0-255 scale; shapes, dtypes, NaN positions, window indices and the
carried buffer exact.  The observed distances go to tests/parity_log."""
import json

import numpy as np
import pytest

from tests import host_audio as ha
from tests import parity_log

pytestmark = pytest.mark.gpu

CASES = [c[0] for c in ha.INTENSITY_CASES]
SPECS = [c[0] for c in ha.SPECTROGRAM_CASES]
INPUTS = ('f32', 'f64', 'i16', 'dev_f32', 'dev_f64', 'dev_i16')


@pytest.fixture(scope='module')
def g18(load_golden):
  return load_golden('g18_audio')


@pytest.fixture(scope='module')
def pp():
  from telluride_decoding_amd import preprocess
  return preprocess


@pytest.fixture(scope='module')
def torch():
  import torch as t
  return t


def case(name):
  return next(c for c in ha.INTENSITY_CASES if c[0] == name)


def as_input(torch, x, kind):
  dtype = {'f32': np.float32, 'f64': np.float64, 'i16': np.int16}[kind.replace('dev_', '')]
  a = np.ascontiguousarray(x, dtype=dtype)
  return torch.from_numpy(a).cuda() if kind.startswith('dev_') else a


def host(torch, y):
  if isinstance(y, torch.Tensor):
    assert y.is_cuda
    return y.cpu().numpy()
  assert isinstance(y, np.ndarray)
  return y


def dist(got, want):
  """max |got - want| / max |want| over the non-NaN entries; shape, dtype and NaN positions exact."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert got.dtype == want.dtype, (got.dtype, want.dtype)
  assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions differ'
  ok = ~np.isnan(want)
  if not ok.any():
    return 0.0
  return float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]))) / float(np.max(np.abs(want[ok])))


def check_buffer(p, want):
  assert p._buff_dtype == want.dtype
  got = p._buff.cpu().numpy()
  assert got.shape == want.shape
  np.testing.assert_array_equal(got, want.astype(np.float64))


@pytest.mark.parametrize('kind', INPUTS)
@pytest.mark.parametrize('name', CASES)
def test_intensity_cases(g18, pp, torch, name, kind):
  _, fs_in, fs_out, window, exponent, c, _, calls, brows = case(name)
  x = ha.case_input(g18, name)
  buff = g18[name + '_buff'] if brows else None
  worst_ref = worst_host = 0.0
  # whole
  p = pp.AudioFeatures('g', fs_in, fs_out, window=window, exponent=exponent,
                       buff=None if buff is None else buff.copy())
  hst = ha.HostAudioFeatures(fs_in, fs_out, window, exponent, buff)
  got = host(torch, p.compute_intensity(as_input(torch, x, kind)))
  worst_ref = max(worst_ref, dist(got, g18[name + '_whole']))
  worst_host = max(worst_host, dist(got, hst.compute_intensity(x)))
  check_buffer(p, g18[name + '_whole_buff'])
  # streamed, mono calls as 1-D waves
  p = pp.AudioFeatures('g', fs_in, fs_out, window=window, exponent=exponent,
                       buff=None if buff is None else buff.copy())
  hst = ha.HostAudioFeatures(fs_in, fs_out, window, exponent, buff)
  s = 0
  for i, m in enumerate(calls):
    piece = x[s:s + m] if c > 1 else x[s:s + m, 0]
    got = host(torch, p.compute_intensity(as_input(torch, piece, kind)))
    worst_ref = max(worst_ref, dist(got, g18['%s_call%d' % (name, i)]))
    worst_host = max(worst_host, dist(got, hst.compute_intensity(piece)))
    check_buffer(p, g18['%s_buff%d' % (name, i)])
    s += m
  # audio_resample of the samples themselves (the reference's run had float64 input)
  if kind in ('f64', 'dev_f64'):
    p = pp.AudioFeatures('g', fs_in, fs_out, window=window, exponent=exponent)
    got = host(torch, p.audio_resample(as_input(torch, x, kind)))
    worst_ref = max(worst_ref, dist(got, g18[name + '_resample']))
    worst_host = max(worst_host, dist(got, ha.HostAudioFeatures(fs_in, fs_out, window).audio_resample(
        x.astype(np.float64))))
  parity_log.record('audio_intensity_%s_%s' % (name, kind), ref=worst_ref, host=worst_host)
  assert worst_ref <= 2e-6 and worst_host <= 1e-12


def test_intensity_tone_and_reference_assertion(g18, pp):
  """The reference's preprocess_test.test_audio_intensity, and its output (G18)."""
  x, window = ha.tone_440()
  p = pp.AudioFeatures('test', 16000, 100, window=1, exponent=np.log10(2), buff=None)
  loudness = p.compute_intensity(x)
  d = dist(loudness, g18['tone_out'])
  dh = dist(loudness, ha.HostAudioFeatures(16000, 100, 1, np.log10(2)).compute_intensity(x))
  parity_log.record('audio_intensity_tone', ref=d, host=dh)
  assert d <= 2e-6 and dh <= 1e-12
  assert len(loudness) == 100
  loudness = loudness / np.max(loudness)
  expected = window[np.arange(0, len(window), 16000 / 100, dtype=np.int32)] ** np.log10(2)
  assert np.max(np.abs(expected - loudness)) < 0.015


@pytest.mark.parametrize('fs_in,fs_out,window,tau', [(16000, 100, 1, 0), (44100, 100, 2.5, 551),
                                                     (48000, 64, 3, 1125), (100, 1000, 1.5, 7),
                                                     (8000, 63, 1.7, 3), (11025.0, 99.5, 2, 0),
                                                     (44100, 100, 1, 220)])
def test_device_window_indices(torch, fs_in, fs_out, window, tau):
  """The kernel's float64 window bounds equal the reference's Python-float loop, row for row."""
  from telluride_decoding_amd import device
  n = 3 * int(fs_in) + 17
  rows = int(round(n / fs_in * fs_out))
  x = torch.ones((n, 1), dtype=torch.float32, device='cuda')
  buf = torch.ones((tau, 1), dtype=torch.float64, device='cuda') if tau else None
  _, win = device.audio_intensity(x, buf, rows, fs_in, fs_out, 0.5 * window / fs_out, True, False, 1,
                                  windows=True)
  np.testing.assert_array_equal(win.cpu().numpy(), ha.windows_loop(n + tau, tau, rows, fs_in, fs_out, window))


def test_intensity_quirks(pp, torch):
  rng = np.random.default_rng(7)
  x = rng.standard_normal((1000, 2)).astype(np.float32)
  p = pp.AudioFeatures('q', 16000, 100)
  p.compute_intensity(x)
  with pytest.raises(ValueError):          # 1 x 2 is transposed to 2 x 1: no longer the buffer's width
    p.compute_intensity(x[:1])
  with pytest.raises(ValueError):
    p.compute_intensity(x[:, :1])
  q = pp.AudioFeatures('q', 16000, 100, buff=np.ones((10, 3), np.float32))
  with pytest.raises(ValueError):
    q.compute_intensity(x)
  m = pp.AudioFeatures('q', 16000, 100)
  assert m.compute_intensity(x[:1, 0]).shape == (0, 1)
  # a wide input is transposed: 2 x 1000 is 1000 frames of 2 channels
  r1 = pp.AudioFeatures('q', 16000, 100).compute_intensity(x.T.copy())
  r2 = pp.AudioFeatures('q', 16000, 100).compute_intensity(x)
  np.testing.assert_array_equal(r1, r2)
  # three contiguous channels take the lane-per-channel kernel
  y = rng.standard_normal((3000, 3)).astype(np.float32)
  got = pp.AudioFeatures('q', 16000, 100, window=2).compute_intensity(torch.from_numpy(y).cuda())
  want = ha.HostAudioFeatures(16000, 100, 2).compute_intensity(y)
  assert dist(got.cpu().numpy(), want) <= 1e-12
  # so does a non-contiguous layout, a channel slice of a wider tensor, through device.audio_intensity with its
  # row stride (AudioFeatures copies such a slice first); the columns around it are NaN
  from telluride_decoding_amd import device
  wide = np.full((3000, 5), np.nan, np.float32)
  wide[:, 1:4] = y
  view = torch.from_numpy(wide).cuda()[:, 1:4]
  assert not view.is_contiguous() and view.stride() == (5, 1)
  got = device.audio_intensity(view, None, want.shape[0], 16000, 100, 0.5 * 2 / 100, True, True, 1)
  assert dist(got.cpu().numpy(), want) <= 1e-12
  got = pp.AudioFeatures('q', 16000, 100, window=2).compute_intensity(view)
  assert dist(got.cpu().numpy(), want) <= 1e-12
  # the pass-through in numpy's dtypes: a float64 exponent promotes the float32 square root, a Python float not
  z = rng.standard_normal((500, 1)).astype(np.float32)
  for exponent, dtype, bound in ((np.log10(2), np.float64, 1e-12), (0.3, np.float32, 4e-7)):
    got = pp.AudioFeatures('q', 100, 100, exponent=exponent).compute_intensity(z)
    want = ha.HostAudioFeatures(100, 100, 1, exponent).compute_intensity(z)
    assert want.dtype == dtype and dist(got, want) <= bound
  # a device buffer of the caller's
  b = torch.from_numpy(np.full((40, 2), 4.0, np.float64)).cuda()
  got = pp.AudioFeatures('q', 16000, 100, buff=b).compute_intensity(x)
  want = ha.HostAudioFeatures(16000, 100, 1, 1, np.full((40, 2), 4.0)).compute_intensity(x)
  assert dist(got, want) <= 1e-12


def test_intensity_20_minutes_every_row(pp, torch):
  """20 min of 44.1 kHz stereo (52.9M frames) to 100 Hz, every output row against the restatement."""
  n = 20 * 60 * 44100
  rng = np.random.default_rng(20)
  x = rng.standard_normal((n, 2), dtype=np.float32)
  x *= (1.0 + 0.5 * np.sin(np.arange(n, dtype=np.float32) * np.float32(2e-5)))[:, None]
  p = pp.AudioFeatures('long', 44100, 100, window=1, exponent=np.log10(2))
  got = p.compute_intensity(torch.from_numpy(x).cuda()).cpu().numpy()
  sq = x * x
  want = np.sqrt(ha.window_means(sq, ha.windows_loop(n, 0, 120000, 44100, 100, 1))) ** np.log10(2)
  d = dist(got, want)
  parity_log.record('audio_intensity_20min', host=d)
  assert got.shape == (120000, 2) and d <= 1e-12


@pytest.mark.parametrize('on_device', (False, True))
@pytest.mark.parametrize('name', SPECS)
def test_spectrogram_cases(g18, pp, torch, name, on_device):
  kw = json.loads(str(g18['spec_%s_kwargs' % name]))
  wave = ha.case_wave(g18, name)
  p = pp.AudioFeatures('g', 16000, 16000)
  s, f = p.compute_spectrogram(torch.from_numpy(wave).cuda() if on_device else wave, **kw)
  s = host(torch, s)
  assert s.dtype == np.float64
  assert s.shape == tuple(g18['spec_%s_shape' % name])
  d = dist(s[:, g18['spec_%s_cols' % name]], g18['spec_%s_out' % name]) * 255
  with np.errstate(invalid='ignore', divide='ignore'):
    dh = dist(s, ha.spectrogram(wave, **kw)[0]) * 255
  np.testing.assert_array_equal(f, g18['spec_%s_f' % name])
  parity_log.record('audio_spectrogram_%s%s' % (name, '_dev' if on_device else ''), ref=d, host=dh)
  assert d <= 1e-9 and dh <= 1e-9


def test_spectrogram_reference_assertion(pp):
  """The reference's preprocess_test.test_audio_spectrogram."""
  p = pp.AudioFeatures('test', 16000, 16000, window=1, exponent=np.log10(2), buff=None)
  spectrogram, _ = p.compute_spectrogram(ha.tone_6000(), segment_size=128, n_overlap=2, n_trans=2,
                                         smoothing_filter=[1])
  assert spectrogram.shape == (129, 251)
  assert np.argmax(spectrogram[:, 125]) == round(6000 / (16000 / (2 * 128)))


def test_spectrogram_limits_and_short_waves(pp):
  p = pp.AudioFeatures('s', 16000, 100)
  rng = np.random.default_rng(5)
  w = rng.standard_normal(9000)
  for kw in (dict(segment_size=1024, n_overlap=4, n_trans=4, smoothing_filter=np.ones(16) / 16),
             dict(segment_size=37, n_overlap=2, n_trans=3)):
    s, _ = p.compute_spectrogram(w, **kw)
    with np.errstate(invalid='ignore', divide='ignore'):
      want = ha.spectrogram(w, **kw)[0]
    assert dist(s, want) * 255 <= 1e-9
  with pytest.raises(ValueError, match='noverlap'):
    p.compute_spectrogram(w[:50])
  s, _ = p.compute_spectrogram(w[:120])
  assert s.shape == (257, 16)
