"""CPU side of the ingest drop-in (telluride_decoding_amd.ingest), through its host fallback: the public surface
and the host-side functions against the reference's own results (G19, tests/golden/make_ingest.py), the
reference's tests ported, the record template the device encoder works from, and the golden file written back
byte for byte."""
import collections
import json
import os
import pickle

import numpy as np
import pytest
import scipy.io.wavfile

from telluride_decoding_amd import device
from telluride_decoding_amd import ingest
from telluride_decoding_amd import tfrecord
from tests import host_ingest as hi
from tests import surface

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, 'golden', 'meg_subj01_400.tfrecords')

CLASSES = {
    'BrainSignal': ['__init__', 'data_type', 'fix_offset', 'name', 'signal', 'sr'],
    'BrainTrial': ['__init__', 'add_model_feature', 'adjust_data_sizes', 'assemble_brain_data', 'brain_data',
                   'filename', 'find_audio_trigger_times', 'find_cognionix_trigger_time', 'find_eeg_trigger_times',
                   'fix_eeg_offset', 'iterate_brain_channels', 'load_brain_data', 'load_sound', 'model_features',
                   'sound_data', 'sound_fs', 'summary_string', 'trial_name', 'write_data_as_tfrecords'],
    'BrainDataFile': ['__init__', 'data_type', 'filename', 'load_all_data', 'signal_fs', 'signal_names',
                      'signal_values'],
    'MemoryBrainDataFile': ['__init__', 'signal_fs', 'signal_names', 'signal_values'],
    'LocalCopy': ['__init__'],
    'EdfBrainDataFile': ['__init__', 'find_channel_index', 'load_all_data', 'signal_fs', 'signal_names',
                         'signal_values'],
    'BrainExperiment': ['__init__', 'add_sound_data', 'check_sound_eeg_files', 'delete_suffix',
                        'get_all_feature_data', 'iterate_trials', 'load_all_data', 'save_zscore_data', 'summary',
                        'trial_data', 'write_all_data', 'z_score_all_data', 'zscore_all_features'],
}
FUNCTIONS = ['assert_type', 'find_temporal_offset_via_linear_regression', 'find_temporal_offset_via_mode_histogram',
             'remove_close_times', 'find_mean_std', 'normalize_data', 'convert_data_to_tfrecords',
             'discover_feature_shapes', 'count_tfrecords', 'read_tfrecords', 'transform_tfrecords', 'parse_edf_file']


@pytest.fixture(autouse=True)
def host_fallback(monkeypatch):
  """These tests are about the NumPy path, also on a machine that has a GPU."""
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


@pytest.fixture(scope='module')
def g19(load_golden):
  return load_golden('g19_ingest')


def checked(g19, key, x):
  assert np.allclose(hi.checksum(x), g19[key + '_xsum'], rtol=1e-12, atol=0), key
  return x


# ---------------------------------------------------------------- surface
def test_surface_matches_reference():
  with open(os.path.join(HERE, 'golden', 'g19_ingest_surface.json')) as f:
    want = json.load(f)
  got = surface.module_surface(ingest)
  for name in FUNCTIONS:
    assert want[name] is not None and got.get(name) == want[name], name
  for name, members in CLASSES.items():
    assert got[name]['bases'] == want[name]['bases'], name
    assert sorted(want[name]['members']) == members, name
    for member, rows in want[name]['members'].items():
      assert got[name]['members'].get(member) == rows, (name, member)


def test_edf_needs_pyedflib(tmp_path):
  with pytest.raises(ImportError, match='pyedflib'):
    ingest.parse_edf_file(str(tmp_path / 'none.edf'))
  with pytest.raises(ImportError, match='pyedflib'):
    ingest.EdfBrainDataFile('none.edf').load_all_data(str(tmp_path))


# ---------------------------------------------------------------- host functions against the reference's results
@pytest.mark.parametrize('name', sorted(hi.close_times_cases()))
def test_remove_close_times(g19, name):
  times, min_time = hi.close_times_cases()[name]
  checked(g19, 'close_' + name, times)
  got = ingest.remove_close_times(times, min_time=min_time)
  assert isinstance(got, np.ndarray) and got.dtype == np.float64
  assert np.array_equal(got, g19['close_' + name])
  assert np.array_equal(ingest.remove_close_times(list(times), min_time), got)


def test_remove_close_times_reference_literal():
  onsets = np.array([1.1, 2.4, 3.5, 6.7, 25.8, 30.4, 87.2, 90.2])
  times = np.sort(np.concatenate((onsets, onsets + 0.1)))
  assert np.sum(onsets - ingest.remove_close_times(times, min_time=0.2)) == 0


@pytest.mark.parametrize('name', sorted(hi.regression_cases()))
def test_offset_via_linear_regression(g19, name):
  audio, eeg = hi.regression_cases()[name]
  checked(g19, 'regress_' + name, np.concatenate((audio, eeg)))
  offset, outliers = ingest.find_temporal_offset_via_linear_regression(audio, eeg, verbose=False)
  assert offset == g19['regress_' + name][0] and outliers == int(g19['regress_' + name][1])
  if name == 'reftest':
    assert abs(offset - 1.3) < 1e-5


@pytest.mark.parametrize('name', sorted(hi.histogram_cases()))
def test_offset_via_mode_histogram(g19, name):
  a, e, max_time, fs = hi.histogram_cases()[name]
  checked(g19, 'hist_' + name, np.concatenate((a, e)))
  got = ingest.find_temporal_offset_via_mode_histogram(a, e, max_time=max_time, fs=fs)
  assert got == float(g19['hist_' + name])
  assert ingest.find_temporal_offset_via_mode_histogram(list(a), list(e), max_time, fs) == got
  if name == 'reftest':
    assert abs(got - 1.42) <= 0.01
  if name == 'samples':
    assert got == 37 and isinstance(got, int)


def test_audio_trigger_edges(g19):
  sound, fs = hi.pulse_train()
  checked(g19, 'pulse', sound)
  trial = ingest.BrainTrial('pulses')
  trial.load_sound(sound, sound_fs=fs)
  got = trial.find_audio_trigger_times()
  assert np.array_equal(got, g19['pulse_times']) and len(got) == 6
  with pytest.raises(ValueError):
    trial.find_audio_trigger_times(3)
  with pytest.raises(ValueError):
    trial.load_sound(sound, sound_fs=0)


def test_eeg_trigger_edges_natus(g19, tmp_path):
  raw, sr = hi.natus_signal()
  checked(g19, 'natus', raw)
  trial = ingest.BrainTrial('natus')
  trial.load_brain_data(str(tmp_path), ingest.MemoryBrainDataFile({'TRIG': raw}, sr))
  times, raw_back, fixed = trial.find_eeg_trigger_times()
  assert np.array_equal(times, g19['natus_times']) and len(times) == 5
  assert np.array_equal(fixed, g19['natus_fixed']) and np.array_equal(raw_back[:, 0], raw)
  with pytest.raises(ValueError):
    trial.find_eeg_trigger_times('none')
  with pytest.raises(ValueError):
    trial.find_cognionix_trigger_time()
  with pytest.raises(IOError):
    trial.load_brain_data(str(tmp_path / 'missing'), ingest.MemoryBrainDataFile({'TRIG': raw}, sr))


def test_fix_offset(g19):
  for i, (signal, sr, seconds) in enumerate(hi.fix_offset_cases()):
    s = ingest.BrainSignal('s', signal, sr)
    s.fix_offset(seconds)
    want = g19['offset_%d' % i]
    assert s.signal.shape == want.shape and s.signal.dtype == want.dtype and np.array_equal(s.signal, want), i
  with pytest.raises(ValueError):
    s.fix_offset(-1)
  with pytest.raises(ValueError):
    ingest.BrainSignal('s', [1, 2], 0)


def test_assemble_brain_data(g19, tmp_path):
  chans, sr, request = hi.assemble_channels()
  checked(g19, 'assemble', np.concatenate([np.asarray(d, np.float64).ravel() for _, d in chans]))
  trial = ingest.BrainTrial('assemble')
  trial.load_brain_data(str(tmp_path), ingest.MemoryBrainDataFile(collections.OrderedDict(chans), sr))
  trial.assemble_brain_data(list(request))
  eeg = trial.model_features['eeg']
  assert eeg.dtype == np.float32 and eeg.shape == (55, 5)
  assert hi.same_bits(eeg, g19['assemble_eeg'])
  # the columns follow brain_data (TRIG, Fp2, pair, O1), not the request (O1, pair, TRIG, Fp2)
  assert np.array_equal(eeg[:, 0], chans[0][1][:55].astype(np.float32))
  assert np.array_equal(eeg[:, 4], chans[4][1][:55])
  trial.assemble_brain_data(', '.join(request))
  assert hi.same_bits(trial.model_features['eeg'], g19['assemble_eeg_csv'])
  assert int(g19['assemble_dup_raises']) == 1 and int(g19['assemble_missing_raises']) == 1
  with pytest.raises(ValueError):
    trial.assemble_brain_data(['TRIG', 'TRIG', 'Fp2'])
  with pytest.raises(ValueError):
    trial.assemble_brain_data('TRIG, FOO, BAR')
  with pytest.raises(TypeError):
    trial.assemble_brain_data(('TRIG',))


def test_adjust_data_sizes(g19):
  data = hi.adjust_inputs()
  checked(g19, 'adjust', np.concatenate([v.ravel().astype(np.float64) for v in data.values()]))
  got = ingest.BrainTrial('adjust').adjust_data_sizes(dict(data))
  assert sorted(got) == sorted(data)
  for k, v in got.items():
    assert hi.same_bits(v, g19['adjust_' + k]), k
    assert v.shape[0] == 100
  with pytest.raises(ValueError):
    ingest.BrainTrial('adjust').adjust_data_sizes([1, 2])


def memory_experiment(directory, offset=None):
  audio, fs, eeg, frame_sr = hi.memory_experiment_inputs()
  if offset is not None:
    audio = audio[:fs]
  df = ingest.MemoryBrainDataFile(collections.OrderedDict(eeg), frame_sr)
  exp = ingest.BrainExperiment({'trial_2': [{'audio_data': audio, 'audio_sr': fs}, df]}, directory, directory,
                               frame_rate=frame_sr)
  return exp, eeg, frame_sr


def test_summary_strings(g19, tmp_path):
  exp, eeg, _ = memory_experiment(str(tmp_path))
  exp.load_all_data()
  assert exp.summary().replace(str(tmp_path), '<dir>') == str(g19['summary_loaded'])
  for trial in exp.iterate_trials():
    trial.assemble_brain_data([k for k, _ in eeg])
  assert exp.summary().replace(str(tmp_path), '<dir>') == str(g19['summary_assembled'])


@pytest.mark.parametrize('case', hi.G19_MOMENT_CASES, ids=[c[0] for c in hi.G19_MOMENT_CASES])
def test_find_mean_std_host(g19, case):
  """float64 whatever the data; no further from the truth than the reference is, up to float64 rounding."""
  name, rows, width, dtype = case
  arrays = hi.moments_data(name, rows, width, dtype)
  checked(g19, 'moments_' + name, np.concatenate(arrays))
  for columnwise in (False, True):
    mean, std = ingest.find_mean_std(arrays, columnwise=columnwise)
    t_mean, t_std = hi.moments_truth(arrays, columnwise)
    if columnwise:
      assert mean.dtype == np.float64 and std.dtype == np.float64 and mean.shape == (1, width) == std.shape
      r_mean, r_std = g19['moments_%s_mean' % name], g19['moments_%s_std' % name]
    else:
      assert type(mean) is np.float64 and type(std) is np.float64
      r_mean, r_std = g19['moments_%s_all' % name]
    scale = np.mean(np.abs(np.concatenate(arrays)), axis=0 if columnwise else None)
    assert np.all(np.abs(mean - t_mean) <= np.abs(r_mean - t_mean) + 1e-12 * scale)
    assert np.all(np.abs(std - t_std) <= np.abs(r_std - t_std) + 1e-12 * t_std)


def test_normalize_data_host():
  a = hi.fill_bits((65, 3), np.float32, 1, specials=False)
  mean, std = np.float64(0.25), np.float64(1.75)
  assert hi.same_bits(ingest.normalize_data(a, mean, std), (a - mean) / std)
  assert hi.same_bits(ingest.normalize_data(a, 0.25, 0.0), a - 0.25)
  cm, cs = np.array([[0.5, -1.0, 2.0]]), np.array([[0.0, 0.0, 0.0]])
  assert hi.same_bits(ingest.normalize_data(a, cm, cs), a - cm)


# ---------------------------------------------------------------- the reference's tests, ported
def test_brain_signal():
  data = np.arange(10)
  s = ingest.BrainSignal('test_name', data, 4, 'test_source')
  assert (s.name, s.data_type, s.sr) == ('test_name', 'test_source', 4)
  assert np.all(np.reshape(data, (-1, 1)) == s.signal)
  s.fix_offset(1)
  assert s.signal[0] == 4 and s.signal[-1] == 9
  s = ingest.BrainSignal('test', np.reshape(np.arange(20), (10, -1)), 4)
  s.fix_offset(1)
  assert len(s.signal.shape) == 2 and s.signal[0, 0] == 8 and s.signal[0, 1] == 9
  with pytest.raises(TypeError):
    ingest.BrainSignal(42, data, 4, 'test_source')


def test_memory_brain_data_file():
  channels = {'one': np.arange(10) + 100, 'two': np.arange(10) + 200}
  df = ingest.MemoryBrainDataFile(channels, 4)
  assert set(df.signal_names) == set(channels)
  assert df.signal_fs('one') == 4 and df.signal_fs('two') == 4
  assert np.all(df.signal_values('one') == channels['one']) and np.all(df.signal_values('two') == channels['two'])
  assert df.signal_values('three') is None and str(df) == "MemoryBrainDataFile('in_memory')"
  with pytest.raises(ValueError):
    ingest.MemoryBrainDataFile({'bad': np.zeros((2, 2, 2))}, 4)
  with pytest.raises(ValueError):
    ingest.MemoryBrainDataFile(channels, 0)


def test_brain_trial(tmp_path):
  """The reference's test with an in-memory recording in the place of its EDF file (pyedflib is not here), and
  a .wav written for it."""
  rng = np.random.default_rng(3)
  sound_dir = tmp_path / 'meg'
  sound_dir.mkdir()
  scipy.io.wavfile.write(str(sound_dir / 'subj01_1ksamples.wav'), 16000,
                         (rng.standard_normal(16001) * 3000).astype(np.int16))
  trial = ingest.BrainTrial('meg/subj01_1ksamples.wav')
  assert trial.trial_name == 'meg/subj01_1ksamples'
  trial.load_sound('meg/subj01_1ksamples.wav', sound_dir=str(tmp_path))
  assert trial.sound_fs == 16000 and trial.sound_data.shape == (16001, 1) and trial.sound_data.dtype == np.float32
  names = 'TRIG, Fp2, F3, F4, F7, F8, C3, C4, T7, T8, P3, P4, P7, P8, O1, O2'.split(', ')
  channels = collections.OrderedDict((k, rng.standard_normal(66 * 512)) for k in names + ['Snore', 'EKG'])
  trial.load_brain_data(str(tmp_path), ingest.MemoryBrainDataFile(channels, 512.0))
  summary = trial.summary_string()
  assert '18 EEG channels' in summary and 'with 66s of eeg data' in summary
  assert '1.00006s of audio data' in summary
  found = list(trial.iterate_brain_channels())
  assert len(found) == 18 and 'TRIG' in [c.name for c in found]
  assert 'eeg' not in trial.model_features
  trial.assemble_brain_data(names)
  assert trial.model_features['eeg'].shape == (66 * 512, len(names))
  tf_dir = tmp_path / 'out'
  (tf_dir / 'meg').mkdir(parents=True)
  trial.model_features['eeg'] = trial.model_features['eeg'][:300]       # (the Python writer is slow)
  tf_file = trial.write_data_as_tfrecords(str(tf_dir))
  shapes = ingest.discover_feature_shapes(tf_file)
  assert shapes['eeg'] == (len(names), 'float32')
  assert ingest.count_tfrecords(tf_file) == (300, False)
  with pytest.raises(ValueError):
    trial.assemble_brain_data('TRIG, FOO, BAR')
  with pytest.raises(ValueError):
    trial.assemble_brain_data(['TRIG', 'TRIG', 'F3'])
  with pytest.raises(ValueError):
    ingest.BrainTrial('none').load_sound('none.wav', sound_dir=str(tmp_path))


def test_mean_std():
  rng = np.random.default_rng(5)
  a, b = rng.standard_normal((3, 5)), rng.standard_normal((3, 5))
  mean, std = ingest.find_mean_std([a, b], columnwise=False)
  both = np.concatenate((a.ravel(), b.ravel()))
  assert abs(mean - np.mean(both)) < 1e-7 and abs(std - np.std(both)) < 1e-7
  mean, std = ingest.find_mean_std([ingest.normalize_data(a, mean, std), ingest.normalize_data(b, mean, std)])
  assert abs(mean) < 1e-7 and abs(std - 1.0) < 1e-7


def test_mean_std_columnwise():
  rng = np.random.default_rng(6)
  a, b = rng.standard_normal((3, 5)), rng.standard_normal((3, 5))
  mean, std = ingest.find_mean_std([a, b], columnwise=True)
  both = np.concatenate((a, b), axis=0)
  np.testing.assert_allclose(np.mean(both, axis=0, keepdims=True)[0], mean[0])
  np.testing.assert_allclose(np.std(both, axis=0, keepdims=True)[0], std[0])
  mean, std = ingest.find_mean_std([ingest.normalize_data(a, mean, std), ingest.normalize_data(b, mean, std)],
                                   columnwise=True)
  np.testing.assert_allclose(mean[0], np.zeros_like(mean[0]), atol=1e-8)
  np.testing.assert_allclose(std[0], np.ones_like(std[0]))


def test_brain_memory_experiment(tmp_path):
  exp, eeg, frame_sr = memory_experiment(str(tmp_path))
  exp.load_all_data()
  summary = exp.summary()
  assert 'Found 1 trials' in summary and 'Trial trial_2: 2 EEG channels with 2s of eeg data' in summary
  for trial in exp.iterate_trials():
    trial.assemble_brain_data([k for k, _ in eeg])
    assert trial.model_features['eeg'].shape == (2 * frame_sr, 2)
  files = exp.write_all_data(str(tmp_path))
  assert files == [os.path.join(str(tmp_path), 'trial_2.tfrecords')]
  assert ingest.count_tfrecords(files[0]) == (2 * frame_sr, False)
  data = ingest.read_tfrecords(files[0])
  np.testing.assert_allclose(data['eeg'], np.stack([eeg[0][1], eeg[1][1]], axis=1))


def test_brain_memory_experiment2(tmp_path):
  exp, eeg, frame_sr = memory_experiment(str(tmp_path), offset=1.0)
  exp.load_all_data()
  assert 'Trial trial_2: 2 EEG channels with 2s of eeg data' in exp.summary()
  for trial in exp.iterate_trials():
    trial.fix_eeg_offset(1.0)
    trial.assemble_brain_data([k for k, _ in eeg])
    assert trial.model_features['eeg'].shape == (frame_sr, 2)
  files = exp.write_all_data(str(tmp_path))
  assert len(files) == 1 and ingest.count_tfrecords(files[0])[1] == 0
  data = ingest.read_tfrecords(files[0])
  np.testing.assert_allclose(data['eeg'], np.stack([eeg[0][1][frame_sr:], eeg[1][1][frame_sr:]], axis=1))


def test_brain_experiment_zscore_and_save(tmp_path):
  """z_score_all_data over two trials of uneven length, 'ones' left alone; the saved moments load back."""
  rng = np.random.default_rng(8)
  trials = {}
  for name, n in (('a', 40), ('b', 55)):
    trials[name] = [{'intensity': (5 + 2 * rng.standard_normal((n, 1))).astype(np.float32),
                     'ones': np.ones((n, 1), np.float32)}]
  exp = ingest.BrainExperiment(trials, str(tmp_path), str(tmp_path))
  exp.load_all_data()
  raw = [t.model_features['intensity'].copy() for t in exp.iterate_trials()]
  exp.z_score_all_data()
  mean, std = ingest.find_mean_std(raw)
  for t, r in zip(exp.iterate_trials(), raw):
    assert hi.same_bits(t.model_features['intensity'], (r - mean) / std)
    assert np.all(t.model_features['ones'] == 1)
  assert exp.get_all_feature_data('none') == [] and exp.trial_data('none') is None
  exp.save_zscore_data(str(tmp_path / 'z.pkl'))
  with open(str(tmp_path / 'z.pkl'), 'rb') as f:
    saved = pickle.load(f)
  assert saved == {'mean': {'intensity': mean}, 'std': {'intensity': std}}
  with pytest.raises(TypeError):
    ingest.BrainExperiment([1], None, None)
  with pytest.raises(TypeError):
    ingest.BrainExperiment({'a': 'not a list'})
  assert ingest.BrainExperiment.delete_suffix('x.wav', '.wav') == 'x'


def test_tfrecord_transform(tmp_path):
  positive = np.arange(5, dtype=np.float32).reshape(-1, 1)
  negative = -positive
  trial = ingest.BrainTrial('Trial 01')
  trial.add_model_feature('positive', positive)
  trial.add_model_feature('negative', negative)
  tf_dir = str(tmp_path)
  first = trial.write_data_as_tfrecords(tf_dir)
  data = ingest.read_tfrecords(first)
  assert sorted(data) == ['negative', 'positive']
  np.testing.assert_equal(data['positive'], positive)
  np.testing.assert_equal(data['negative'], negative)
  new_file = ingest.transform_tfrecords(first, tf_dir, 'New Trial 01', [lambda d: ('two', 2 * d['positive'])])
  assert new_file == os.path.join(tf_dir, 'New Trial 01.tfrecords')
  data = ingest.read_tfrecords(new_file)
  assert sorted(data) == ['negative', 'positive', 'two']
  np.testing.assert_equal(data['positive'], positive)
  np.testing.assert_equal(data['negative'], negative)
  np.testing.assert_equal(data['two'], 2 * positive)
  assert ingest.read_tfrecords(new_file, start_frame=2, frame_count=2)['two'].tolist() == [[0], [0], [4], [6]]


# ---------------------------------------------------------------- the writer
def test_record_template_of_the_golden_file():
  with open(GOLDEN_FILE, 'rb') as f:
    first = f.read(650)
  template, layout = tfrecord.record_template({'meg': 148, 'envelope': 1})
  assert len(template) == 650 and int.from_bytes(template[:8], 'little') == 634
  want = tfrecord._float_layout(memoryview(first)[12:12 + 634])
  assert [(k, off - 12, n) for k, off, n in layout] == want
  assert sorted((off, n) for _, off, n in layout) == [(33, 1), (54, 148)]
  skeleton = np.ones(650, bool)
  skeleton[646:] = False
  for _, off, n in layout:
    skeleton[off:off + 4 * n] = False
  got, ref = np.frombuffer(template, np.uint8), np.frombuffer(first, np.uint8)
  assert np.array_equal(got[skeleton], ref[skeleton]) and not got[~skeleton].any()
  assert ingest.device_record_plan({'meg': np.zeros((2, 148), np.float32),
                                    'envelope': np.zeros((2, 1))}) == (template, layout)
  assert ingest.device_record_plan({'meg': np.zeros((2, 148), np.float32), 'n': np.zeros((2, 1), np.int32)}) is None


def test_golden_file_round_trip_host(tmp_path):
  data = tfrecord.read_file(GOLDEN_FILE)
  out = str(tmp_path / 'back.tfrecords')
  ingest.convert_data_to_tfrecords(out, data)
  with open(out, 'rb') as f, open(GOLDEN_FILE, 'rb') as g:
    got, want = f.read(), g.read()
  assert len(want) == 260000 and got == want


def test_writer_errors_and_integers(tmp_path):
  out = str(tmp_path / 'x.tfrecords')
  with pytest.raises(ValueError):
    ingest.convert_data_to_tfrecords(out, {'a': np.zeros((3, 1)), 'b': np.zeros((4, 1))})
  with pytest.raises(ValueError):
    ingest.convert_data_to_tfrecords(out, {'a': np.zeros(3)})
  with pytest.raises(ValueError):
    ingest.convert_data_to_tfrecords(out, {'a': np.zeros((3, 1), np.complex64)})
  with pytest.raises(ValueError):
    ingest.convert_data_to_tfrecords(out, {'a': np.array([['x'], ['y']])})
  with pytest.raises(TypeError):
    ingest.convert_data_to_tfrecords(out, [1])
  ints = np.array([[0, -1], [1 << 40, 127], [128, -(1 << 62)]], np.int64)
  floats = np.arange(6, dtype=np.float64).reshape(3, 2) / 3
  ingest.convert_data_to_tfrecords(out, {'count': ints, 'x': floats})
  recs = [tfrecord.parse_example(r) for r in tfrecord.iter_records(out, verify=True)]
  assert [r['count'].dtype for r in recs] == [np.int64] * 3
  assert np.array_equal(np.stack([r['count'] for r in recs]), ints)
  assert np.array_equal(np.stack([r['x'] for r in recs]), floats.astype(np.float32))
  assert ingest.discover_feature_shapes(out) == {'count': (2, 'int64'), 'x': (2, 'float32')}
  # the reversed write of the host path
  trial = ingest.BrainTrial('rev')
  trial.add_model_feature('eeg', floats)
  trial.add_model_feature('intensity', floats[:, :1])
  back = ingest.read_tfrecords(trial.write_data_as_tfrecords(str(tmp_path), reverse_data_for_test=True))
  assert np.array_equal(back['eeg'], floats[::-1].astype(np.float32))
  assert np.array_equal(back['intensity'], floats[:, :1].astype(np.float32))


def test_route_predicate():
  """device.tfrecord_route: the staged groups start 16-byte aligned and fit 48 KB; past that, the large route."""
  for stride in (17, 24, 650, 651, 652, 656, 1024, 3071, 3072, 3073, 6000, 16410, 49152, 49153, 80030):
    staged, group, lanes = device.tfrecord_route(stride)
    smallest = 16 // np.gcd(stride, 16)
    assert staged == (smallest * stride <= 48 * 1024), stride
    if staged:
      assert group % smallest == 0 and (group * stride) % 16 == 0 and group * stride <= 48 * 1024
      assert 1 <= group <= 256 and group * lanes <= 256 and lanes & (lanes - 1) == 0
    else:
      assert group == 0 and lanes == 256
  with pytest.raises(ValueError):
    device.tfrecord_route(16)
