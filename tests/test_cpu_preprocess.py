"""CPU side of the Preprocessor drop-in (telluride_decoding_amd.preprocess): the NumPy Butterworth designer
against scipy, parameter parsing and the reference's check_params errors, the resample indices against the
reference's own (G16, bit-exact), the public surface against the reference's, and a host float64
restatement of the whole chain (tests/host_preprocess.py) against G16."""
import json
import os

import numpy as np
import pytest

from telluride_decoding_amd import iir
from telluride_decoding_amd import preprocess as pp
from tests import host_preprocess as hp
from tests import surface

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ('a', 'b', 'c', 'd')


@pytest.fixture(scope='module')
def g16(load_golden):
  return load_golden('g16_preprocess')


DESIGNS = [(2, 1, 'hp', 1000), (4, 0.5, 'hp', 128), (4, 30, 'lp', 128), (10, 37.5, 'lp', 1000),
           (10, 24, 'lp', 500), (4, 0.1, 'hp', 1000), (2, 0.5, 'hp', 100), (3, 5, 'hp', 250), (5, 40, 'lp', 250),
           (1, 10, 'lp', 100)]


@pytest.mark.parametrize('order,cutoff,btype,fs', DESIGNS)
def test_designer_matches_scipy(order, cutoff, btype, fs):
  signal = pytest.importorskip('scipy.signal')
  want = signal.butter(order, cutoff, btype, output='sos', fs=fs)
  got = iir.butter_sos(order, cutoff, btype, fs)
  assert got.shape == want.shape
  np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
  np.testing.assert_allclose(iir.sosfilt_zi(got), signal.sosfilt_zi(want), rtol=0, atol=1e-12)


def test_designer_matches_g16_cascades(g16):
  for name in CASES:
    kw = json.loads(str(g16[name + '_kwargs']))
    p = pp.Preprocessor('g', kw.pop('fs_in'), kw.pop('fs_out'), **kw)
    np.testing.assert_allclose(p.sos, g16[name + '_sos'], rtol=0, atol=1e-12)


def test_designer_rejects_cutoff_at_nyquist():
  with pytest.raises(ValueError):
    iir.butter_sos(2, 50, 'hp', 100)


def test_channel_string_parsing():
  assert pp.parse_channel_numbers('0-3,7') == [0, 1, 2, 3, 7]
  assert pp.parse_channel_numbers('7,0-3,2') == [0, 1, 2, 3, 7]
  assert pp.parse_channel_numbers('5') == [5]
  p = pp.Preprocessor('eeg', 100, 100, channel_numbers='4-6,1')
  assert p.channel_numbers == [1, 4, 5, 6]
  assert pp.Preprocessor('eeg', 100, 100, channel_numbers=[3, 1]).channel_numbers == [3, 1]


def test_name_params_string():
  p = pp.Preprocessor('eeg(highpass_cutoff=1;highpass_order=2;channel_numbers=0-31)', 100, 100)
  assert p.name == 'eeg'
  assert p.highpass_cutoff == 1 and p.highpass_order == 2
  assert p.channel_numbers == list(range(32))
  np.testing.assert_allclose(p.sos, iir.butter_sos(2, 1, 'hp', 100), rtol=0, atol=0)
  q = pp.Preprocessor('x', 100, 100)
  q.init_from_string(100, 'env(highpass_cutoff=0.5;highpass_order=3;channel_numbers=0)')
  assert q.name == 'env' and q.highpass_order == 3 and q.channel_numbers == [0]
  with pytest.raises(ValueError):
    pp.Preprocessor('eeg(highpass_cutoff)', 100, 100)
  with pytest.raises(ValueError):
    pp.Preprocessor('eeg(no_such_key=1)', 100, 100)


def test_automatic_antialias_lowpass():
  p = pp.Preprocessor('eeg', 1000, 100)
  assert p.lowpass_cutoff == 37.5 and p.lowpass_order == 10
  assert p.sos.shape == (5, 6)
  q = pp.Preprocessor('eeg', 1000, 100, lowpass_cutoff=80, lowpass_order=2)   # above the new Nyquist
  assert q.lowpass_cutoff == 37.5 and q.lowpass_order == 10
  r = pp.Preprocessor('eeg', 1000, 100, lowpass_cutoff=20, lowpass_order=2)
  assert r.lowpass_cutoff == 20 and r.sos.shape == (1, 6)
  assert pp.Preprocessor('eeg', 100, 100).sos is None


@pytest.mark.parametrize('kwargs,err', [
    (dict(name=3), TypeError),
    (dict(fs_in=0), ValueError),
    (dict(fs_out=-1), ValueError),
    (dict(highpass_cutoff=-1), ValueError),
    (dict(highpass_order=-1), ValueError),
    (dict(lowpass_cutoff=-1), ValueError),
    (dict(lowpass_order=-1), ValueError),
    (dict(ref_channels=3), ValueError),
    (dict(channels_to_ref=(1, 2)), ValueError),
    (dict(channel_numbers=3.5), ValueError),
    (dict(data_std=0), ValueError),
    (dict(data_std=None), TypeError),
    (dict(pre_context=-1), ValueError),
    (dict(post_context=-1), ValueError),
])
def test_check_params_errors(kwargs, err):
  args = dict(name='eeg', fs_in=100, fs_out=100)
  args.update(kwargs)
  with pytest.raises(err):
    pp.Preprocessor(**args)


@pytest.mark.parametrize('name', ['a', 'c'])
def test_resample_indices_bit_exact(g16, name):
  kw = json.loads(str(g16[name + '_kwargs']))
  n = g16[name + '_x'].shape[0]
  idx, nxt = pp.resample_indices(n, kw['fs_in'], kw['fs_out'])
  np.testing.assert_array_equal(idx, g16[name + '_idx'])
  assert nxt == int(g16[name + '_whole_next'])


def test_resample_indices_upsampling_repeats_rows():
  idx, _ = pp.resample_indices(10, 64, 100)
  assert idx.shape == (16,) and np.all(np.diff(idx) >= 0) and idx[-1] == 9


def test_surface_matches_reference():
  with open(os.path.join(HERE, 'golden', 'g16_preprocess_surface.json')) as f:
    want = json.load(f)
  got = surface.module_surface(pp)['Preprocessor']
  assert got['bases'] == want['bases']
  for name, rows in want['members'].items():
    assert name in got['members'], name
    assert got['members'][name] == rows, name


@pytest.mark.parametrize('name', CASES)
def test_host_restatement_against_g16(g16, name):
  """The chain restated in float64 NumPy (the package's designer, scipy's recurrence) reproduces the
  reference's outputs, whole and streamed, and its final filter states."""
  kw = str(g16[name + '_kwargs'])
  x = g16[name + '_x']
  scale = np.max(np.abs(x))
  h = hp.HostPreprocessor(kw)
  got = h.process(x)
  want = g16[name + '_whole']
  assert got.shape == want.shape
  assert np.max(np.abs(got - want)) <= 1e-9 * scale
  if h.stages:
    assert np.max(np.abs(h.state() - g16[name + '_whole_state'])) <= 1e-9 * scale
  h = hp.HostPreprocessor(kw)
  s = 0
  for i, m in enumerate(g16[name + '_calls']):
    got = h.process(x[s:s + m], reset=(i == int(g16[name + '_reset_at'])))
    want = g16['%s_call%d' % (name, i)]
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-9 * scale
    s += m
  if h.stages:
    assert np.max(np.abs(h.state() - g16[name + '_stream_state'])) <= 1e-9 * scale


def test_reference_paths_agree():
  """The two host reference filters (scipy's sosfilt, the NumPy recurrence) agree on a small hard case: a
  high-pass order 5 at 0.5 Hz and a low-pass order 7 at 3.75 Hz at 1 kHz, DC-offset input."""
  signal = pytest.importorskip('scipy.signal')
  sos = np.concatenate([iir.butter_sos(5, 0.5, 'hp', 1000), iir.butter_sos(7, 3.75, 'lp', 1000)])
  rng = np.random.default_rng(3)
  x = 2.0 + rng.standard_normal((3000, 3))
  zi = iir.sosfilt_zi(sos)[:, :, None] * x[0]
  y_np, z_np = hp.sosfilt(sos, x, zi)
  y_sp, z_sp = signal.sosfilt(sos, x, axis=0, zi=zi)
  scale = float(np.max(np.abs(x)))
  d = max(float(np.max(np.abs(y_np - y_sp))), float(np.max(np.abs(z_np - z_sp)))) / scale
  assert d <= 1e-12, d
  assert hp.REF_PATH == 'scipy'
  np.testing.assert_array_equal(hp.sosfilt_ref(sos, x, zi)[0], y_sp)


def test_process_files_rejects_empty_file_with_filter():
  p = pp.Preprocessor('eeg', 100, 100, highpass_cutoff=1, highpass_order=2)
  x = np.ones((10, 2), np.float32)
  with pytest.raises(ValueError, match='empty file'):
    p.process_files(x, [0, 4, 4, 10])
