"""CPU side of the BioSemi BDF reader (ingest_bdf) through its host route: seeded files against the independent
reader of tests/host_bdf.py bit for bit, the unscaled 'Status' signal, the recovered record count, the files that
are turned down, BdfBrainDataFile through BrainTrial with find_status_trigger_times against events written out
here, the declarations of the new C entries and the plan of the onset kernels."""
import os

import numpy as np
import pytest

from telluride_decoding_amd import _lib
from telluride_decoding_amd import device
from telluride_decoding_amd import ingest
from telluride_decoding_amd import ingest_bdf
from telluride_decoding_amd import ingest_edf
from tests import host_bdf as hb
from tests import host_raw as hr

NEW_ENTRIES = ('td_raw24_decode', 'td_code_onsets_plan', 'td_code_onsets_count', 'td_code_onsets_fill')


@pytest.fixture(autouse=True)
def bdf_host_route(monkeypatch):
  """These tests are about the host route, wherever they run."""
  monkeypatch.setattr(ingest_bdf.device, 'gpu_available', lambda: False)


# ---------------------------------------------------------------- against the independent reader
@pytest.mark.parametrize('channels', [1, 5])
@pytest.mark.parametrize('records,n', [(1, 1), (3, 5), (2, 256), (4, 85)])
def test_against_the_numpy_reader(tmp_path, channels, records, n):
  for annotations_at in (None, 0, (channels + 1) // 2, channels + 1):      # none, first, in the middle, last
    path, signals = hb.synth_bdf(str(tmp_path / 'synth.bdf'), channels, records, n, seed=3, annotations_at=annotations_at)
    got = ingest_bdf.parse_bdf_file(path)
    labels, rates, want = hb.read_bdf_numpy(path)
    assert got['labels'] == labels == ['A%03d' % (c + 1) for c in range(channels)] + ['Status']
    assert list(got['sample_rates']) == rates == [float(n)] * (channels + 1)
    assert isinstance(got['signals'], np.ndarray) and got['signals'].dtype == np.float64
    assert want.shape == (channels + 1, records * n) and hr.same_bits(got['signals'], want)
    assert got['header']['records'] == records and [h['label'] for h in got['signal_headers']] == labels
    # the patterns 0x7fffff, 0x800000, 0xffffff are in the file
    first = next(s for s in signals if s['label'] == 'A001')['digital'].reshape(-1)
    assert list(first[:3]) == [0x7fffff, -0x800000, -1][:first.size]


def test_status_is_served_unscaled(tmp_path):
  path, signals = hb.synth_bdf(str(tmp_path / 's.bdf'), 2, 3, 40, seed=1)
  got = ingest_bdf.parse_bdf_file(path)
  status = got['signal_headers'][2]
  assert status['label'] == 'Status' and (status['physical_min'], status['physical_max']) == (-262144.0, 262143.0)
  assert np.array_equal(got['signals'][2], signals[2]['digital'].reshape(-1).astype(np.float64))
  assert (got['signals'][2] < 0).all()                             # (bit 23 is set throughout)
  # an ordinary signal with the same ranges is scaled
  assert not np.array_equal(got['signals'][0], signals[0]['digital'].reshape(-1).astype(np.float64))
  # a label that merely contains the word is an ordinary signal
  signals[2]['label'] = 'Status2'
  again = ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 't.bdf'), signals))
  assert hr.same_bits(again['signals'], hb.read_bdf_numpy(str(tmp_path / 't.bdf'))[2])
  assert not np.array_equal(again['signals'][2], got['signals'][2])


@pytest.mark.parametrize('records_field', [-1, 9])
def test_record_count_is_recovered(tmp_path, records_field):
  path, signals = hb.synth_bdf(str(tmp_path / 'cut.bdf'), 3, 4, 11, seed=2, annotations_at=1,
                               records_field=records_field, extra_tail=b'\x01\x02\x03\x04\x05')
  got = ingest_bdf.parse_bdf_file(path)
  assert got['header']['records'] == 4 and got['signals'].shape == (4, 44)
  assert hr.same_bits(got['signals'], hb.read_bdf_numpy(path)[2])
  # a header that tells the truth about a file whose last record is not whole
  path, _ = hb.synth_bdf(str(tmp_path / 'short.bdf'), 3, 4, 11, seed=2, drop_tail_bytes=2)
  short = ingest_bdf.parse_bdf_file(path)
  assert short['header']['records'] == 3 and short['signals'].shape == (4, 33)


def ordinary(label, digital, **ranges):
  entry = {'label': label, 'digital': np.asarray(digital, np.int32), 'physical_min': -262144, 'physical_max': 262143,
           'digital_min': -8388608, 'digital_max': 8388607}
  entry.update(ranges)
  return entry


def test_files_that_are_turned_down(tmp_path):
  two = [ordinary('A1', [[1, 2, 3]]), ordinary('A2', [[4, 5, 6]])]
  with pytest.raises(ValueError, match=r'BDF\+D'):
    ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 'd.bdf'), two, reserved='BDF+D'))
  assert ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 'c.bdf'), two, reserved='BDF+C'))['labels'] == ['A1', 'A2']
  with pytest.raises(ValueError, match='samples per record'):
    ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 'u.bdf'), [two[0], ordinary('A2', [[4, 5, 6, 7]])]))
  with pytest.raises(ValueError, match='empty physical or digital range'):
    ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 'e.bdf'), [two[0], ordinary('A2', [[4, 5, 6]], physical_max=-262144)]))
  with pytest.raises(ValueError, match='empty physical or digital range'):
    ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 'f.bdf'), [two[0], ordinary('A2', [[4, 5, 6]], digital_min=8388607)]))
  with pytest.raises(ValueError, match='record duration'):
    ingest_bdf.parse_bdf_file(hb.write_bdf(str(tmp_path / 'z.bdf'), two, duration=0))
  # an EDF file: the message says where EDF files are read
  edf = hr.write_edf(str(tmp_path / 'plain.edf'), [{'label': 'Fp1', 'digital': np.array([[1, 2, 3]], np.int16),
                                                    'physical_min': -1, 'physical_max': 1, 'digital_min': -32768,
                                                    'digital_max': 32767}])
  with pytest.raises(ValueError, match='ingest_edf'):
    ingest_bdf.parse_bdf_file(edf)
  with pytest.raises(ValueError, match='ingest_edf'):
    ingest_bdf.read_bdf_header(edf)
  with pytest.raises(IOError):
    ingest_bdf.BdfBrainDataFile('none').load_all_data(str(tmp_path))
  with pytest.raises(IOError):
    ingest_bdf.BdfBrainDataFile('none').load_all_data(str(tmp_path / 'no_such_dir'))


def test_edf_reader_still_turns_bdf_down(tmp_path, monkeypatch):
  """The pin of tests/test_cpu_raw_ingest.py restated: BDF has a module of its own, ingest_edf does not read it."""
  monkeypatch.setattr(ingest_edf.device, 'gpu_available', lambda: False)
  path, _ = hb.synth_bdf(str(tmp_path / 'b.bdf'), 2, 2, 4)
  with pytest.raises(ValueError, match='BDF'):
    ingest_edf.parse_edf_file(path)
  main, signals, size = ingest_bdf.read_bdf_header(path)
  assert main['signals'] == 3 and main['header_bytes'] == 1024 and size == 1024 + 2 * 3 * 4 * 3
  assert signals[2]['label'] == 'Status' and signals[0]['samples_per_record'] == 4


# ---------------------------------------------------------------- through a trial
STATUS_LOW = [5, 5, 0, 0, 7, 9, 9, 0, 3, 3, 0x10003, 2, 0, 0, 1, 1]
#             ^ sample 0      ^  ^ 7 -> 9   ^     ^ bit 16 alone changes    ^
STATUS_EVENTS = {0xffff: ([0, 4, 5, 8, 11, 14], [5, 7, 9, 3, 2, 1]),
                 0x1: ([0, 4, 8, 14], [1, 1, 1, 1]),           # 5 -> 0 -> 7 -> 9 -> 0 -> 3 -> 3 -> 2: the low bit
                 0xffffff: None}                               # (filled in below: bit 23 takes part)


def status_signal():
  """STATUS_LOW under BioSemi's status bits, bit 23 among them: every stored number is negative."""
  value = np.array(STATUS_LOW, np.int64) | 0x900000
  return (value - (1 << 24)).astype(np.int32)


def test_trial_and_status_trigger_times(tmp_path):
  digital = status_signal()
  assert (digital < 0).all()
  rng = np.random.default_rng(0)
  signals = [ordinary('A1', hb.int24_patterns(rng, 16).reshape(2, 8), physical_max=262150),
             ordinary('Status', digital.reshape(2, 8)),
             ordinary('BDF Annotations', np.zeros((2, 3), np.int32)),
             ordinary('A2', hb.int24_patterns(rng, 16).reshape(2, 8), physical_min=-262147)]
  hb.write_bdf(str(tmp_path / 'rec.bdf'), signals, duration=0.5)                  # 16 Hz
  trial = ingest.BrainTrial('trial')
  trial.load_brain_data(str(tmp_path), ingest_bdf.BdfBrainDataFile('rec'))
  assert list(trial.brain_data) == ['A1', 'Status', 'A2']
  assert trial.brain_data['Status'].sr == 16.0
  trial.assemble_brain_data(['A1', 'A2'])
  want = hb.read_bdf_numpy(str(tmp_path / 'rec.bdf'))[2]
  assert hr.same_bits(trial.model_features['eeg'], np.ascontiguousarray(want[[0, 2]].T.astype(np.float32)))

  for mask in (0xffff, 0x1):
    times, codes = trial.find_status_trigger_times(mask=mask)
    at, expected = STATUS_EVENTS[mask]
    assert times.dtype == np.float64 and codes.dtype == np.int64
    assert np.array_equal(times, np.array(at) / 16.0) and list(codes) == expected
    ref_at, ref_codes = hb.code_onsets_numpy(digital.astype(np.float64), mask)
    assert list(ref_at) == at and list(ref_codes) == expected                # (the oracle agrees with the list)
  # with every bit: the change of bit 16 alone at sample 10 is an event, and the returns to code 0 are events too,
  # because the status bits above keep the number from being 0
  times, codes = trial.find_status_trigger_times(mask=0xffffff)
  assert list(times * 16) == [0, 2, 4, 5, 7, 8, 10, 11, 12, 14]
  assert codes[0] == 0x900005 and codes[6] == 0x910003
  with pytest.raises(ValueError, match='channel name TRIG not in brain data'):
    trial.find_status_trigger_times('TRIG')

  # the times recover a planted offset between the sound's triggers and the recording's
  audio_times = np.array(STATUS_EVENTS[0xffff][0][1:]) / 16.0 - 0.25
  times, _ = trial.find_status_trigger_times()
  assert ingest.find_temporal_offset_via_mode_histogram(audio_times, times, fs=16) == 0.25


def test_experiment_summary(tmp_path):
  hb.synth_bdf(str(tmp_path / 'trial.bdf'), 4, 2, 32, seed=5)
  sound = {'audio_data': np.zeros((1000, 1), np.float32), 'audio_sr': 16000}
  experiment = ingest.BrainExperiment({'trial': [sound, ingest_bdf.BdfBrainDataFile('trial')]}, str(tmp_path), str(tmp_path))
  experiment.load_all_data()
  assert 'Trial trial: 5 EEG channels with 2s of eeg data' in experiment.summary()
  assert issubclass(ingest_bdf.BdfBrainDataFile, ingest.EdfBrainDataFile)


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


def test_code_onsets_plan_answers_without_a_gpu():
  chunk, groups = device.code_onsets_plan(0)
  assert chunk >= 64 and groups == 0
  for n in (1, 63, chunk - 1, chunk, chunk + 1, 3 * chunk + 1, 1 << 33):
    assert device.code_onsets_plan(n) == (chunk, -(-n // chunk))
  with pytest.raises(ValueError):
    device.code_onsets_plan(-1)


def test_existing_pins_still_hold():
  with pytest.raises(ValueError):
    device.raw_route(1, 3, 256)
  assert (device.RAW_INT16, device.RAW_FLOAT32) == (0, 1)
