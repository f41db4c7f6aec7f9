"""CPU side of the raw-recording readers (ingest_brainvision, ingest_edf), through their host routes: the public
surface and every value of the reference's own BrainVision recording against the reference's results (G20,
tests/golden/make_brainvision.py), the reference's three tests restated, INT_16 / VECTORIZED files and EDF files
against the readers of tests/host_raw.py and against values written out here, the files that are turned down, and
the declarations of the new C entries."""
import json
import os

import numpy as np
import pytest

from telluride_decoding_amd import _lib
from telluride_decoding_amd import device
from telluride_decoding_amd import ingest
from telluride_decoding_amd import ingest_brainvision
from telluride_decoding_amd import ingest_edf
from tests import host_raw as hr
from tests import surface

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
NEW_ENTRIES = ('td_raw_decode', 'td_raw_route', 'td_columns_assemble', 'td_columns_route')

EXPECTED_NAMES = ['Fp1', 'Fz', 'F3', 'F7', 'FT9', 'FC5', 'FC1', 'C3', 'T7', 'TP9', 'CP5', 'CP1', 'Pz', 'P3', 'P7', 'O1',
                  'Oz', 'O2', 'P4', 'P8', 'TP10', 'CP6', 'CP2', 'C4', 'T8', 'FT10', 'FC6', 'FC2', 'F4', 'F8', 'Fp2',
                  'AF7', 'AF3', 'AFz', 'F1', 'F5', 'FT7', 'FC3', 'C1', 'C5', 'TP7', 'CP3', 'P1', 'P5', 'PO7', 'PO3',
                  'POz', 'PO4', 'PO8', 'P6', 'P2', 'CPz', 'CP4', 'TP8', 'C6', 'C2', 'FC4', 'FT8', 'F6', 'AF8', 'AF4',
                  'F2', 'FCz', 'TRIG', 'EOG']


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
  """These tests are about the host route, wherever they run."""
  monkeypatch.setattr(ingest_brainvision.device, 'gpu_available', lambda: False)


@pytest.fixture(scope='module')
def g20():
  return dict(np.load(os.path.join(GOLDEN, 'g20_brainvision.npz')))


def loaded(directory, name):
  bv = ingest_brainvision.BvBrainDataFile(name)
  bv.load_all_data(directory)
  return bv


# ---------------------------------------------------------------- BrainVision: the reference's recording
def test_surface_matches_reference():
  with open(os.path.join(GOLDEN, 'g20_brainvision_surface.json')) as f:
    want = json.load(f)
  got = surface.module_surface(ingest_brainvision)
  assert set(want) == {'parse_bv_keywords', 'parse_bv_header', 'read_bv_file', 'BvBrainDataFile'}
  for name, rows in want.items():
    if isinstance(rows, list):
      assert got.get(name) == rows, name
    else:
      assert got[name]['bases'] == rows['bases'], name
      for member, member_rows in rows['members'].items():
        assert got[name]['members'].get(member) == member_rows, (name, member)


def test_read_bv_file(g20):
  header, data = ingest_brainvision.read_bv_file(os.path.join(GOLDEN, 'brainvision_test.vhdr'))
  assert {'Common Infos', 'Binary Infos', 'Channel Infos'} <= set(header)
  assert header['Common Infos']['SamplingInterval'] == 2000
  assert header['Common Infos']['NumberOfChannels'] == 65
  assert data.shape == (5, 65) and data.dtype == np.float32
  assert np.array_equal(data.view(np.uint32), g20['data'].view(np.uint32))
  assert json.loads(json.dumps(header)) == json.loads(str(g20['header_json']))
  assert list(header['Channel Infos']) == list(json.loads(str(g20['header_json']))['Channel Infos'])
  # the '.vhdr' may be left off
  _, again = ingest_brainvision.read_bv_file(os.path.join(GOLDEN, 'brainvision_test'))
  assert np.array_equal(again.view(np.uint32), data.view(np.uint32))


def test_brainvision_data_file(g20):
  bv = loaded(GOLDEN, 'brainvision_test.vhdr')
  assert bv.signal_names == EXPECTED_NAMES == json.loads(str(g20['names_json']))
  assert bv.signal_fs('foo') == 500 == float(g20['signal_fs'])
  assert bv.find_channel_index() == 63 == int(g20['index_default'])
  assert bv.find_channel_index('TRIG') == 63 == int(g20['index_TRIG'])
  assert bv.find_channel_index('C3') == 7 == int(g20['index_C3'])
  assert bv.signal_values('CH1') is None and int(g20['missing_is_none']) == 1
  assert bv.find_channel_resolution('CH1') is None
  with pytest.raises(ValueError):
    bv.signal_values(7)
  trig = bv.signal_values('TRIG')
  assert trig is not None and trig.shape == (5,)
  for i, name in enumerate(EXPECTED_NAMES):
    got, want = bv.signal_values(name), g20['values_%02d' % i]
    assert got.dtype == want.dtype == np.float32 and hr.same_bits(got, want), name
  with pytest.raises(IOError):
    ingest_brainvision.BvBrainDataFile('brainvision_test.vhdr').load_all_data(os.path.join(GOLDEN, 'no_such_dir'))


def test_brain_experiment(g20):
  df = ingest_brainvision.BvBrainDataFile('brainvision_test.vhdr')
  sound = {'audio_data': np.zeros((1000, 1), np.float32), 'audio_sr': 16000}
  experiment = ingest.BrainExperiment({'subj01_1ksamples': [sound, df]}, GOLDEN, GOLDEN)
  experiment.load_all_data()
  summary = experiment.summary()
  assert 'Found 1 trials' in summary
  assert 'Trial subj01_1ksamples: 65 EEG channels with 0.01s of eeg data' in summary
  assert summary.replace(GOLDEN, '<dir>') == str(g20['summary'])


def test_keywords_and_header_parsing():
  section = 'Common Infos]\n; a comment\nA=1\nB = 2.5 \nC=text=more\n\nno equals sign\nD=1e3\n'
  got = ingest_brainvision.parse_bv_keywords(section)
  assert list(got.items()) == [('A', 1), ('B', 2.5), ('C', 'text=more'), ('D', 1000.0)]
  assert isinstance(got['A'], int) and isinstance(got['D'], float)
  with pytest.raises(TypeError):
    ingest_brainvision.parse_bv_header('[Channel Infos]\nCh1=5\n')
  header = ingest_brainvision.parse_bv_header('junk\n[Comment]\nline one\nline two\n[Binary Infos]\nBinaryFormat=INT_16\n')
  assert header['Comment'] == ['', 'line one', 'line two', '']
  assert header['Binary Infos'] == {'BinaryFormat': 'INT_16'}


# ---------------------------------------------------------------- BrainVision: what the reference does not read
@pytest.mark.parametrize('binary_format', ['IEEE_FLOAT_32', 'INT_16'])
@pytest.mark.parametrize('orientation', ['MULTIPLEXED', 'VECTORIZED'])
def test_formats_against_the_numpy_reader(tmp_path, binary_format, orientation):
  path, samples, factors = hr.synth_brainvision(str(tmp_path), 'rec', 7, 33, binary_format, orientation, seed=4)
  names, rate, want = hr.read_brainvision_numpy(path)
  assert hr.same_bits(want, hr.scaled_channels(samples, factors))       # (the two oracles agree)
  header, data = ingest_brainvision.read_bv_file(path)
  assert data.shape == (33, 7) and data.dtype == np.float32
  plain = samples.view(np.float32) if samples.dtype == np.uint32 else samples.astype(np.float32)
  assert hr.same_bits(data, plain)
  bv = loaded(str(tmp_path), 'rec')
  assert bv.signal_names == names and bv.signal_fs('x') == rate
  for c, name in enumerate(names):
    with np.errstate(all='ignore'):
      got = bv.signal_values(name)
    assert got.dtype == np.float32 and hr.same_bits(got, want[c]), name


def test_files_that_are_turned_down(tmp_path):
  rng = np.random.default_rng(0)
  samples = hr.float_patterns(rng, 12).reshape(4, 3)
  factors = hr.resolutions(3)
  d = str(tmp_path)
  with pytest.raises(ValueError, match='ASCII'):
    ingest_brainvision.read_bv_file(hr.write_brainvision(d, 'ascii', samples, factors, data_format='ASCII'))
  with pytest.raises(ValueError, match='INT_32'):
    ingest_brainvision.read_bv_file(hr.write_brainvision(d, 'int32', samples, factors, binary_format='INT_32'))
  with pytest.raises(ValueError, match='SIDEWAYS'):
    ingest_brainvision.read_bv_file(hr.write_brainvision(d, 'side', samples, factors, orientation='SIDEWAYS'))
  cut = hr.write_brainvision(d, 'cut', samples, factors)
  with open(os.path.join(d, 'cut.eeg'), 'r+b') as f:
    f.truncate(4 * 3 * 4 - 2)
  with pytest.raises(ValueError):
    ingest_brainvision.read_bv_file(cut)
  with pytest.raises(ValueError):
    loaded(d, 'cut')


# ---------------------------------------------------------------- EDF
def hand_made_signals():
  """Two records; three ordinary signals of 3 samples and, second in the file, an annotation signal of 5."""
  return [
      {'label': 'Fp1', 'digital': np.array([[-32768, 0, 32767], [1, -1, 1000]], np.int16),
       'physical_min': -32768, 'physical_max': 32767, 'digital_min': -32768, 'digital_max': 32767},
      {'label': 'EDF Annotations', 'digital': np.array([[11, 12, 13, 14, 15], [16, 17, 18, 19, 20]], np.int16),
       'physical_min': -1, 'physical_max': 1, 'digital_min': -32768, 'digital_max': 32767},
      {'label': 'TRIG', 'digital': np.array([[-32768, 32767, 3], [-5, 0, 2]], np.int16),
       'physical_min': -16384, 'physical_max': 16383.5, 'digital_min': -32768, 'digital_max': 32767},
      {'label': 'Cz', 'digital': np.array([[-32768, 32767, 0], [7, -7, 100]], np.int16),
       'physical_min': 0, 'physical_max': 65535, 'digital_min': -32768, 'digital_max': 32767},
  ]


HAND_MADE_VALUES = np.array([[-32768.0, 0.0, 32767.0, 1.0, -1.0, 1000.0],
                             [-16384.0, 16383.5, 1.5, -2.5, 0.0, 1.0],
                             [0.0, 65535.0, 32768.0, 32775.0, 32761.0, 32868.0]])


@pytest.fixture
def edf_host_route(monkeypatch):
  monkeypatch.setattr(ingest_edf.device, 'gpu_available', lambda: False)


@pytest.mark.parametrize('records_field', [None, -1, 9])
def test_edf_hand_made_file(tmp_path, edf_host_route, records_field):
  path = hr.write_edf(str(tmp_path / 'hand.edf'), hand_made_signals(), records_field=records_field, duration=0.5,
                      reserved='EDF+C')
  got = ingest_edf.parse_edf_file(path)
  assert got['labels'] == ['Fp1', 'TRIG', 'Cz']
  assert isinstance(got['signals'], np.ndarray) and got['signals'].dtype == np.float64
  assert np.array_equal(got['signals'], HAND_MADE_VALUES)
  assert np.array_equal(got['sample_rates'], [6.0, 6.0, 6.0])
  assert got['header']['records'] == 2 and got['header']['record_duration'] == 0.5
  assert [h['label'] for h in got['signal_headers']] == got['labels']
  assert got['signal_headers'][1]['physical_max'] == 16383.5 and got['signal_headers'][1]['dimension'] == 'uV'
  assert got['signal_headers'][2]['transducer'] == 'electrode' and got['signal_headers'][2]['sample_rate'] == 6.0
  labels, rates, want = hr.read_edf_numpy(path)
  assert labels == got['labels'] and rates == [6.0] * 3 and hr.same_bits(got['signals'], want)

  edf = ingest_edf.EdfBrainDataFile('hand')
  edf.load_all_data(str(tmp_path))
  assert edf.signal_names == ['Fp1', 'TRIG', 'Cz'] and edf.find_channel_index() == 1
  assert edf.signal_fs('Cz') == 6.0 and np.array_equal(edf.signal_values('TRIG'), HAND_MADE_VALUES[1])


def test_edf_cut_off_file(tmp_path, edf_host_route):
  """A second record that is not whole is not read, whatever the header says."""
  path = hr.write_edf(str(tmp_path / 'cut.edf'), hand_made_signals(), drop_tail_bytes=2)
  got = ingest_edf.parse_edf_file(path)
  assert got['header']['records'] == 1 and np.array_equal(got['signals'], HAND_MADE_VALUES[:, :3])


def test_edf_synthetic_against_the_numpy_reader(tmp_path, edf_host_route):
  path, _ = hr.synth_edf(str(tmp_path / 'synth.edf'), 5, 4, 9, seed=2, annotations_at=2)
  got = ingest_edf.parse_edf_file(path)
  labels, rates, want = hr.read_edf_numpy(path)
  assert got['labels'] == labels and list(got['sample_rates']) == rates
  assert want.shape == (5, 36) and hr.same_bits(got['signals'], want)


def test_edf_files_that_are_turned_down(tmp_path, edf_host_route):
  with pytest.raises(ValueError, match=r'EDF\+D'):
    ingest_edf.parse_edf_file(hr.write_edf(str(tmp_path / 'd.edf'), hand_made_signals(), reserved='EDF+D'))
  with pytest.raises(ValueError, match='BDF'):
    ingest_edf.parse_edf_file(hr.write_edf(str(tmp_path / 'b.edf'), hand_made_signals(), version=b'\xffBIOSEMI'))
  unequal = hand_made_signals()
  unequal[3]['digital'] = np.zeros((2, 4), np.int16)
  with pytest.raises(ValueError, match='samples per record'):
    ingest_edf.parse_edf_file(hr.write_edf(str(tmp_path / 'u.edf'), unequal))
  with pytest.raises(IOError):
    ingest_edf.EdfBrainDataFile('none').load_all_data(str(tmp_path))
  with pytest.raises(IOError):
    ingest_edf.EdfBrainDataFile('none').load_all_data(str(tmp_path / 'no_such_dir'))


def test_only_the_new_reader_does_without_pyedflib(tmp_path, edf_host_route):
  hr.write_edf(str(tmp_path / 'hand.edf'), hand_made_signals())
  with pytest.raises(ImportError, match='pyedflib'):
    ingest.EdfBrainDataFile('hand').load_all_data(str(tmp_path))
  with pytest.raises(ImportError, match='pyedflib'):
    ingest.parse_edf_file(str(tmp_path / 'hand.edf'))
  assert issubclass(ingest_edf.EdfBrainDataFile, ingest.EdfBrainDataFile)
  ingest_edf.EdfBrainDataFile('hand').load_all_data(str(tmp_path))


# ---------------------------------------------------------------- the C entries
def test_the_entries_are_declared_bound_and_exported():
  lib = _lib.load()
  with open(_lib.HEADER) as f:
    text = f.read()
  for name in NEW_ENTRIES:
    assert name in _lib.header_symbols() and name in _lib.SIGNATURES
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    declaration = text[text.index('int %s(' % name):]
    declaration = declaration[:declaration.index(';')]
    assert declaration.count(',') + 1 == len(_lib.SIGNATURES[name]), name


def test_routes_answer_without_a_gpu():
  assert device.raw_route(1, 4, 256) == (True, 128)           # a 64-channel float32 frame: 65 dwords a row
  assert device.raw_route(1, 2, 2) == (True, 128)
  assert device.raw_route(500, 2, 64000) == (False, 0)        # an EDF record: runs of 1000 bytes
  assert device.raw_route(1, 4, 4096) == (False, 0)           # fewer than 16 records fit the staging area
  for w in (2, 4):
    threshold = 64 // w
    assert device.raw_route(threshold - 1, w, 64 * w)[0] and not device.raw_route(threshold, w, 64 * w)[0]
  for bad in ((0, 4, 256), (-1, 2, 256), (1, 3, 256), (8, 4, 16), (1, 4, 6)):
    with pytest.raises(ValueError):
      device.raw_route(*bad)
  assert device.columns_route(16, 1) and not device.columns_route(15, 1) and not device.columns_route(64, 2)
  with pytest.raises(ValueError):
    device.columns_route(0, 1)
