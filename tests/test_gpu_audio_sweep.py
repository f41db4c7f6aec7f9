"""GPU sweep of the AudioFeatures kernels (csrc/audio.hip through telluride_decoding_amd.preprocess and
telluride_decoding_amd.device) against the float64 host restatement (tests/host_audio.py) at their tile edges.

Intensity: 1, 2, 3, 4, 5 and 8 channels (the 16-B kernel for 1, 2 and 4 contiguous aligned channels, the
lane-per-channel kernel otherwise); float32, float64 and int16 from numpy and from device tensors; both
compute_intensity and audio_resample; spans of 1 to 9 rows at every start residue mod 4, 2.5 s windows,
windowed upsampling with empty windows, a user buffer longer than a span, uneven streaming with 0-, 1- and 2-frame
calls; aligned, offset and row-strided device layouts; inf, NaN and float32 overflow.  The restatement sums each
window exactly (host_audio.window_means_exact).
Spectrogram: host_audio.SPECTROGRAM_SWEEP (segment, frame and bin counts at the DFT's and the FIR's tile edges,
hop 1 and hop = segment, odd nfft, 1 to 16 taps, negative taps, short waves), int16 / float64 / strided / offset /
NaN / all-zero waves, the cached cos / sin tables, and every cell of a 60 s spectrogram.
Bounds: intensity within 1e-12 x max of the restatement (the float32 pass-through within 4e-7); spectrogram within
1e-9 on the 0-255 scale; shapes, dtypes, NaN and inf positions, window indices and the carried buffer exact.
Every case writes its distance to tests/parity_log."""
import math

import numpy as np
import pytest

from tests import host_audio as ha
from tests import parity_log

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

TOL = 1e-12            # intensity vs the exact restatement, x max
TOL_F32 = 4e-7         # the float32 pass-through (test_intensity_quirks' bound)
SPEC_TOL = 1e-9        # spectrogram, on the 0-255 scale
CHANNELS = (1, 2, 3, 4, 5, 8)
KINDS = ('f32', 'f64', 'i16', 'dev_f32', 'dev_f64', 'dev_i16')
OPS = ('intensity', 'resample')
SHORT_FS_OUT = (990, 480, 330, 245, 198, 165, 141, 124, 110)   # fs_in 1000, window 1: spans of ~1 ... 9 rows


@pytest.fixture(scope='module')
def pp():
  from telluride_decoding_amd import preprocess
  return preprocess


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


@pytest.fixture(scope='module')
def torch():
  import torch as t
  return t


def dist(got, want):
  """max |got - want| / max |want| over the finite entries; shape, dtype, NaN and inf positions exact."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert got.dtype == want.dtype, (got.dtype, want.dtype)
  assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions differ'
  assert np.array_equal(np.isposinf(got), np.isposinf(want)), '+inf positions differ'
  assert np.array_equal(np.isneginf(got), np.isneginf(want)), '-inf positions differ'
  ok = np.isfinite(want)
  if not ok.any():
    return 0.0
  scale = float(np.max(np.abs(want[ok].astype(np.float64))))
  diff = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok])))
  return diff / scale if scale > 0 else diff


def to_host(torch, y, on_device):
  if on_device:
    assert isinstance(y, torch.Tensor) and y.is_cuda
    return y.cpu().numpy()
  assert isinstance(y, np.ndarray)
  return y


def int_samples(n, c, seed):
  """Integer-valued samples over the whole int16 range (float32 squares above 2^24 round)."""
  rng = np.random.default_rng(seed)
  x = rng.integers(-32768, 32768, size=(n, c)).astype(np.float64)
  x[::97] = 32767.0
  x[5::101] = -32768.0
  return x


def as_kind(torch, x, kind):
  dtype = {'f32': np.float32, 'f64': np.float64, 'i16': np.int16}[kind.replace('dev_', '')]
  a = np.ascontiguousarray(x, dtype=dtype)
  return torch.from_numpy(a).cuda() if kind.startswith('dev_') else a


def run_op(obj, op, data):
  return obj.compute_intensity(data) if op == 'intensity' else obj.audio_resample(data)


def check_buffer(p, hst):
  assert p._buff_dtype == hst.buff.dtype, (p._buff_dtype, hst.buff.dtype)
  got = p._buff.cpu().numpy()
  assert got.shape == hst.buff.shape, (got.shape, hst.buff.shape)
  np.testing.assert_array_equal(got, hst.buff.astype(np.float64))


# ------------------------------------------------------------------------------------------------ intensity
def intensity_scenarios(c):
  """(label, fs_in, fs_out, window, exponent, user buffer rows, frames, call lengths or None for one call)."""
  return (
      [('short%d' % f, 1000, f, 1, 1, 0, 700, None) for f in (990, 330, 141, 110)] +
      [('long', 44100, 2, 5, float(np.log10(2)), 0, 220500, None),          # 2.5 s windows (110 250 rows)
       ('upsample', 100, 350, 2.5, 0.5, 0, 300, None),                      # windows of 0 or 1 rows
       ('buffer', 1000, 100, 1, 1, 37, 323, (23, 300)),                     # 37 buffered rows, spans of 10
       ('stream', 8000, 100, 1.5, float(np.log10(2)), 0, 4726, (517, 0, 1, 2, 3000, 1, 2, 1203)),
       ('pass', 100, 100, 1, 1, 0, 250, (100, 1, 2, 147)),                  # the pass-through
       ('pass03', 100, 100, 1, 0.3, 0, 250, None)])


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('c', CHANNELS)
def test_intensity_sweep(pp, torch, c, kind, op):
  on_dev = kind.startswith('dev_')
  worst = {'host': 0.0, 'f32': 0.0}       # float64 outputs; the float32 pass-through
  for label, fs_in, fs_out, window, exponent, brows, frames, calls in intensity_scenarios(c):
    x = int_samples(frames, c, seed=7 * c + len(label))
    buff = int_samples(brows, c, seed=3) ** 2 if brows else None
    p = pp.AudioFeatures('s', fs_in, fs_out, window=window, exponent=exponent,
                         buff=None if buff is None else buff.copy())
    hst = ha.HostAudioFeatures(fs_in, fs_out, window, exponent, buff, exact=True)
    s = 0
    for i, m in enumerate(calls or (frames,)):
      piece = x[s:s + m] if c > 1 else x[s:s + m, 0]
      s += m
      try:
        with np.errstate(over='ignore', invalid='ignore'):
          want = run_op(hst, op, as_kind(torch, piece, kind.replace('dev_', '')))
      except ValueError:           # numpy's transposition quirk: the call no longer matches the buffer
        with pytest.raises(ValueError):
          run_op(p, op, as_kind(torch, piece, kind))
        continue
      got = to_host(torch, run_op(p, op, as_kind(torch, piece, kind)), on_dev)
      d = dist(got, want)
      key = 'f32' if want.dtype == np.float32 else 'host'
      assert d <= (TOL_F32 if key == 'f32' else TOL), (label, i, d)
      worst[key] = max(worst[key], d)
      check_buffer(p, hst)
  parity_log.record('audio_sweep_intensity_c%d_%s_%s' % (c, kind, op), **worst)


def span_stats(win, nb, c):
  """Row lengths and start residues (mod 4, in elements) of the spans of x the windows cover."""
  lengths, residues, straddle = set(), set(), 0
  for t1, t2 in win:
    x1, x2 = max(t1, nb) - nb, t2 - nb
    if x2 > x1:
      lengths.add(int(x2 - x1))
      residues.add(int(x1 * c % 4))
    straddle += int(t1 < nb < t2)
  return lengths, residues, straddle


@pytest.mark.parametrize('square', (True, False))
@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('c', CHANNELS)
def test_intensity_span_edges(dev, torch, c, dtype, square):
  """Spans of 1 to 9 rows starting at every residue mod 4 the layout allows, with a carried buffer that the
  first windows straddle; window indices from the kernel exact, means against the exact restatement."""
  n, nb, fs_in = 700, 13, 1000
  x = int_samples(n, c, seed=c)
  buf = int_samples(nb, c, seed=11) ** 2
  xd = torch.from_numpy(x.astype(dtype)).cuda()
  bd = torch.from_numpy(buf).cuda()
  sq = (x.astype(np.float32) ** 2).astype(np.float64) if square else x
  cat = np.concatenate([buf, sq])
  lengths, residues, straddle, worst = set(), set(), 0, 0.0
  for fs_out in SHORT_FS_OUT:
    for window in (1, 1.37):
      rows = int(round(n / fs_in * fs_out))
      hw = 0.5 * window / fs_out
      got, win = dev.audio_intensity(xd, bd, rows, fs_in, fs_out, hw, square, square, 1, windows=True)
      win = win.cpu().numpy()
      np.testing.assert_array_equal(win, ha.windows_loop(nb + n, nb, rows, fs_in, fs_out, window))
      want = ha.window_means_exact(cat, win)
      if square:
        want = np.sqrt(want)
      d = dist(got.cpu().numpy(), want)
      assert d <= TOL, (fs_out, window, d)
      worst = max(worst, d)
      ln, rs, st = span_stats(win, nb, c)
      lengths |= ln
      residues |= rs
      straddle += st
  g = math.gcd(c, 4)
  assert set(range(1, 10)) <= lengths, sorted(lengths)
  assert residues == set(range(0, 4, g)), sorted(residues)
  assert straddle > 0
  parity_log.record('audio_sweep_span_edges_c%d_%s_%s' % (c, dtype, 'sq' if square else 'raw'), host=worst)


def routes(torch, x, c, dtype):
  """(name, device view of x, reaches the 16-B kernel): aligned, row-offset and element-offset views (all
  contiguous: AudioFeatures passes them on as they are)."""
  n = x.shape[0]
  tdt = getattr(torch, dtype)
  out = []
  base = torch.zeros(n * c + 64, dtype=tdt, device='cuda')
  v = base[:n * c].view(n, c)
  v.copy_(torch.from_numpy(x.astype(dtype)))
  out.append(('aligned', v))
  for k in (1, 2, 3):
    rows = torch.zeros((n + k, c), dtype=tdt, device='cuda')
    rows[k:] = torch.from_numpy(x.astype(dtype))
    out.append(('row%d' % k, rows[k:]))
    flat = torch.zeros(n * c + 8, dtype=tdt, device='cuda')
    e = flat[k:k + n * c].view(n, c)
    e.copy_(torch.from_numpy(x.astype(dtype)))
    out.append(('elem%d' % k, e))
  return [(name, t, c in (1, 2, 4) and t.data_ptr() % 16 == 0) for name, t in out]


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('c', (1, 2, 4))
def test_intensity_routes(pp, dev, torch, c, dtype, op):
  """Every device layout meets the bound: aligned views take the 16-B kernel, offset views the lane-per-channel
  one, and a channel slice of a wider tensor (row stride > channels) the lane-per-channel kernel with that stride
  through device.audio_intensity; AudioFeatures copies such a slice first."""
  n, fs_in, fs_out, window, nb = 3000, 1000, 100, 2, 25
  rng = np.random.default_rng(100 + c)
  x = rng.standard_normal((n, c)).astype(dtype).astype(np.float64)   # not integer-valued: fsum sums
  buff = rng.standard_normal((nb, c)) ** 2
  with np.errstate(over='ignore'):
    want = run_op(ha.HostAudioFeatures(fs_in, fs_out, window, 1, buff, exact=True), op, x.astype(dtype))
  worst, seen = {}, set()
  for name, v, vec in routes(torch, x, c, dtype):
    assert v.is_contiguous()
    p = pp.AudioFeatures('r', fs_in, fs_out, window=window, buff=buff.copy())
    got = run_op(p, op, v).cpu().numpy()
    worst[name] = dist(got, want)
    seen.add(vec)
  assert seen == {True, False}, 'both intensity kernels must be reached'
  # a row-strided channel slice; the other columns are NaN, so reading one of them would show
  square = op == 'intensity'
  wide = torch.full((n, c + 3), float('nan'), dtype=getattr(torch, dtype), device='cuda')
  wide[:, 1:1 + c] = torch.from_numpy(x.astype(dtype))
  view = wide[:, 1:1 + c]
  assert view.stride() == (c + 3, 1)
  rows = int(round(n / fs_in * fs_out))
  got, win = dev.audio_intensity(view, torch.from_numpy(buff).cuda(), rows, fs_in, fs_out, 0.5 * window / fs_out,
                                 square, square, 1, windows=True)
  np.testing.assert_array_equal(win.cpu().numpy(), ha.windows_loop(nb + n, nb, rows, fs_in, fs_out, window))
  worst['strided'] = dist(got.cpu().numpy(), want)
  p = pp.AudioFeatures('r', fs_in, fs_out, window=window, buff=buff.copy())
  worst['strided_public'] = dist(run_op(p, op, view).cpu().numpy(), want)
  parity_log.record('audio_sweep_routes_c%d_%s_%s' % (c, dtype, op), host=max(worst.values()), **worst)
  assert max(worst.values()) <= TOL, worst


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('kind', ('f64', 'dev_f64', 'f32', 'dev_f32'))
@pytest.mark.parametrize('c', (1, 2, 3, 4))
def test_intensity_non_finite(pp, torch, c, kind, op):
  """float64 samples beyond float32's range (inf once cast), samples whose float32 square overflows, infs and
  NaNs: NaN poisons exactly the windows that hold one, inf gives inf (NaN with -inf in a plain resample)."""
  n, fs_in, fs_out, window = 2000, 1000, 100, 1.5
  x = int_samples(n, c, seed=40 + c)
  big = kind.endswith('f64')
  specials = [(101, 0, 5e38 if big else 3e19), (333, c - 1, -4e38 if big else -2e19), (650, 0, 1e20),
              (900, c // 2, np.nan), (1203, c - 1, np.inf), (1206, c - 1, -np.inf), (1500, 0, np.nan),
              (1777, c // 2, 2e19)]
  for r, ch, v in specials:
    x[r, ch] = v
  with np.errstate(over='ignore', invalid='ignore'):
    xk = x.astype(np.float64 if big else np.float32)
    hst = ha.HostAudioFeatures(fs_in, fs_out, window, 1, exact=True)
    want = run_op(hst, op, xk)
  p = pp.AudioFeatures('n', fs_in, fs_out, window=window)
  got = to_host(torch, run_op(p, op, as_kind(torch, xk, kind)), kind.startswith('dev_'))
  assert not np.isfinite(want).all() and np.isfinite(want).any()
  d = dist(got, want)
  # the windows away from the large samples, at their own scale
  calm = np.array([not (np.abs(x[max(t1, 0):t2]) > 1e6).any() for t1, t2 in hst.windows])
  dc = dist(got[calm], want[calm])
  parity_log.record('audio_sweep_non_finite_c%d_%s_%s' % (c, kind, op), host=max(d, dc))
  assert d <= TOL and dc <= TOL, (d, dc)
  check_buffer(p, hst)


# ------------------------------------------------------------------------------------------------ spectrogram
def host_spectrogram(wave, **kw):
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    return ha.spectrogram(wave, **kw)


def check_spectrogram(got, f, wave, kw):
  want, want_f = host_spectrogram(wave, **kw)
  assert got.dtype == np.float64
  np.testing.assert_array_equal(f, want_f)
  return dist(got, want) * 255


@pytest.mark.parametrize('name', [c[0] for c in ha.SPECTROGRAM_SWEEP])
def test_spectrogram_sweep(pp, name):
  wave, kw = ha.sweep_case(name)
  s, f = pp.AudioFeatures('s', 16000, 16000).compute_spectrogram(wave, **kw)
  assert isinstance(s, np.ndarray)
  seg, _, nfft, frames = ha.spectrogram_shape(wave.shape[0], kw['segment_size'], kw['n_overlap'], kw['n_trans'])
  assert s.shape == (nfft // 2 + 1, frames)
  d = check_spectrogram(s, f, wave, kw)
  parity_log.record('audio_sweep_spectrogram_%s' % name, host=d)
  assert d <= SPEC_TOL


SPEC_KW = (dict(), dict(segment_size=100, n_overlap=3, n_trans=3, smoothing_filter=(.5, .5)))


@pytest.mark.parametrize('kw', range(len(SPEC_KW)))
@pytest.mark.parametrize('kind', ('i16', 'f64', 'dev_f32', 'dev_f64', 'dev_strided', 'dev_offset', 'nan',
                                  'dev_nan', 'zeros'))
def test_spectrogram_inputs(pp, torch, kind, kw):
  kw = SPEC_KW[kw]
  n = 3001
  rng = np.random.default_rng(9)
  wave = ha.spectrogram_input('inputs', n)
  if kind == 'i16':
    wave = rng.integers(-32768, 32768, size=n).astype(np.int16)
  elif kind in ('nan', 'dev_nan'):
    wave[777] = np.nan
  elif kind == 'zeros':
    wave = np.zeros(n)
  if kind == 'dev_f32':
    arg = torch.from_numpy(wave.astype(np.float32)).cuda()
  elif kind in ('dev_f64', 'dev_nan'):
    arg = torch.from_numpy(wave).cuda()
  elif kind == 'dev_strided':
    stereo = torch.from_numpy(np.stack([wave, -wave[::-1]], axis=1).astype(np.float32)).cuda()
    arg = stereo[:, 0]
    assert arg.stride() == (2,)
  elif kind == 'dev_offset':
    base = torch.from_numpy(np.concatenate([[1e3, -1e3, 1e3], wave]).astype(np.float32)).cuda()
    arg = base[3:]
    assert arg.data_ptr() % 16 != 0
  else:
    arg = wave
  s, f = pp.AudioFeatures('s', 16000, 16000).compute_spectrogram(arg, **kw)
  s = to_host(torch, s, kind.startswith('dev_'))
  d = check_spectrogram(s, f, wave, kw)
  if kind in ('nan', 'dev_nan', 'zeros'):
    assert np.isnan(s).all()
  parity_log.record('audio_sweep_spectrogram_input_%s_%d' % (kind, len(kw)), host=d)
  assert d <= SPEC_TOL


def test_spectrogram_table_cache(pp):
  """Interleaved (segment, nfft) pairs, one of them first reached by a wave shorter than its segment (seg shrunk
  to the wave's length), each against the host; then the first call again, bit for bit."""
  calls = [(2500, dict(segment_size=64, n_overlap=4, n_trans=2)),          # (64, 128)
           (120, dict()),                                                    # (120, 512): seg shrunk from 128
           (2500, dict(segment_size=64, n_overlap=4, n_trans=4)),          # (64, 256)
           (2500, dict(segment_size=120, n_overlap=8, n_trans=4.27)),      # (120, 512) again, a full segment
           (2500, dict(segment_size=128, n_overlap=2, n_trans=1)),         # (128, 128)
           (2500, dict(segment_size=120, n_overlap=8, n_trans=2.14)),      # (120, 256)
           (2500, dict(segment_size=37, n_overlap=2, n_trans=3)),          # (37, 111)
           (1000, dict(segment_size=64, n_overlap=2, n_trans=2))]          # (64, 128) again
  p = pp.AudioFeatures('c', 16000, 16000)
  first, worst = None, 0.0
  for i, (n, kw) in enumerate(calls):
    wave = ha.spectrogram_input('cache%d' % n, n)
    s, f = p.compute_spectrogram(wave, **kw)
    d = check_spectrogram(s, f, wave, kw)
    assert d <= SPEC_TOL, (i, d)
    worst = max(worst, d)
    if i == 0:
      first = s
  wave = ha.spectrogram_input('cache2500', 2500)
  again, _ = p.compute_spectrogram(wave, **calls[0][1])
  np.testing.assert_array_equal(again, first)
  parity_log.record('audio_sweep_spectrogram_cache', host=worst)


def test_spectrogram_60s_every_cell(pp, torch):
  """The DESIGN section 13 timing case: 60 s at 16 kHz, the reference's defaults, all 257 x 60 001 cells."""
  wave = ha.spectrogram_input('time', 60 * 16000).astype(np.float32)
  s, f = pp.AudioFeatures('t', 16000, 16000).compute_spectrogram(torch.from_numpy(wave).cuda())
  s = s.cpu().numpy()
  assert s.shape == (257, 60001)
  d = check_spectrogram(s, f, wave, {})
  parity_log.record('audio_sweep_spectrogram_60s', host=d)
  assert d <= SPEC_TOL
