"""Stage 1, ingestion: drop-in for the reference's ingest.py (same names, parameters, defaults, error types).

Recordings -- a sound plus EEG / MEG / ECoG channels -- are lined up in time, z-scored over all the trials of an
experiment and written as TFRecord files, one tf.train.Example per frame, which brain_data reads back.

  BrainSignal      one named signal [times, channels] with a sample rate (ingest.py:94-156)
  BrainTrial       one trial = one TFRecord file: sound, signals, model features (ingest.py:274-647)
  BrainDataFile    where a trial's signals come from: MemoryBrainDataFile, EdfBrainDataFile (ingest.py:653-824)
  BrainExperiment  every trial: load, z-score, summarise, write (ingest.py:832-1058)

What differs from the reference:
  * A feature array is a NumPy array or a device tensor (preprocess._is_device_tensor's convention: what
    Preprocessor.resample and AudioFeatures.compute_intensity return).  A device tensor stays one through
    add_model_feature, z_score_all_data, assemble_brain_data and adjust_data_sizes, up to the write.
  * With a GPU (device.gpu_available()) three operations run on it, for NumPy inputs as well: the joint moments
    of find_mean_std (device.ingest_moments), normalize_data (device.ingest_normalize) and the file image of
    convert_data_to_tfrecords (device.tfrecord_encode: one launch, one copy, one write per trial).  Without one
    everything is NumPy and tfrecord.write_file.  Trigger edges, offset estimation, remove_close_times and the
    bookkeeping are NumPy either way.
  * find_mean_std sums in float64 and returns float64 (see there).
  * save_zscore_data writes its pickle in binary mode (the reference's text mode cannot hold one).
  * discover_feature_shapes returns {name: (width, dtype name)} (tfrecord.discover_feature_shapes), not
    tf.io.FixedLenFeature objects: TensorFlow is not a dependency.
  * EdfBrainDataFile and parse_edf_file import pyedflib when used and raise an ImportError that says so;
    ingest_edf has an EdfBrainDataFile and a parse_edf_file that need no pyedflib and decode the file on the GPU;
    ingest_bdf has the same for BioSemi BDF files (24-bit samples), whose 'Status' events
    BrainTrial.find_status_trigger_times finds on the device.
  * assemble_brain_data builds 'eeg' from float32 / float64 device tensors in one launch
    (device.columns_assemble) instead of one strided copy per channel.
  * BrainVision recordings are read by ingest_brainvision, a module of its own as in the reference.
    regression_data (downloads data sets) and add_trigger (stimulus preparation) are not here.
"""
import collections
import logging
import os
import pickle
import shutil
import tempfile

import numpy as np

from telluride_decoding_amd import device
from telluride_decoding_amd import tfrecord

_BIG = 1 << 31


def _torch():
  import torch
  return torch


def _is_device_tensor(data):
  try:
    torch = _torch()
  except ImportError:
    return False
  return isinstance(data, torch.Tensor) and data.is_cuda


def _as_feature(data):
  """A device tensor as it is, anything else through np.asarray."""
  return data if _is_device_tensor(data) else np.asarray(data)


def _host_array(data):
  return data.cpu().numpy() if _is_device_tensor(data) else np.asarray(data)


def _float_tensor(data):
  """`data` as a float32 / float64 device tensor; other dtypes become float64 (what numpy's arithmetic with a
  float64 mean makes of them)."""
  torch = _torch()
  if _is_device_tensor(data):
    return data if data.dtype in (torch.float32, torch.float64) else data.to(torch.float64)
  arr = np.asarray(data)
  if arr.dtype not in (np.float32, np.float64):
    arr = arr.astype(np.float64)
  return torch.from_numpy(np.ascontiguousarray(arr)).to(device.default_handle().device)


def _rows_tensor(t):
  """The [rows, width] view the kernels take: rows contiguous, any row stride."""
  if t.dim() != 2:
    t = t.reshape(-1, 1) if t.dim() <= 1 else t.reshape(t.shape[0], -1)
  if t.shape[1] > 1 and t.stride(1) != 1:
    t = t.contiguous()
  return t


def _all_float_device_tensors(signals):
  """Whether device.columns_assemble takes them: float32 / float64 device tensors, within its limits."""
  if not signals or len(signals) > device.COLUMNS_MAX_SOURCES or sum(s.shape[1] for s in signals) > 65536:
    return False
  if not all(_is_device_tensor(s) for s in signals):
    return False
  torch = _torch()
  return all(s.dtype in (torch.float32, torch.float64) and s.shape[1] >= 1 for s in signals)


def _assemble_columns_loop(chosen, frames, width):
  """The first `frames` rows of the signals side by side as float32, one strided copy per signal: NumPy inputs,
  and host and device inputs mixed (then, and for device inputs of other dtypes, a device tensor)."""
  where = next((s.device for s in chosen if _is_device_tensor(s)), None)
  if where is None:
    eeg = np.zeros((frames, width), dtype=np.float32)
  else:
    torch = _torch()
    eeg = torch.zeros((frames, width), dtype=torch.float32, device=where)
  c = 0
  for s in chosen:
    piece = s[:frames, :]
    if where is not None and not _is_device_tensor(piece):
      piece = _torch().from_numpy(np.ascontiguousarray(piece, dtype=np.float32)).to(where)
    eeg[:, c:c + s.shape[1]] = piece
    c += s.shape[1]
  return eeg


def assert_type(var_name, var, expected_type):
  if not isinstance(var, expected_type):
    raise TypeError('%s must be of type %s, but got value %s of type %s' %
                    (var_name, expected_type, var, type(var)))


# ---------------------------------------------------------------- one signal
class BrainSignal(object):
  """One named brain signal, [times, channels] (1-D input becomes a column), NumPy or device tensor."""

  def __init__(self, name, signal, sample_rate, data_type=None):
    assert_type('name', name, str)
    if not sample_rate > 0.0:
      raise ValueError('a signal needs a sample rate above 0, not %s' % sample_rate)
    signal = _as_feature(signal)
    self._signal = signal.reshape(-1, 1) if len(signal.shape) == 1 else signal
    self._name = name
    self._sr = float(sample_rate)
    self._data_type = data_type
    self._time_zero = 0.0

  @property
  def signal(self):
    return self._signal

  @property
  def data_type(self):
    return self._data_type

  @property
  def sr(self):
    return self._sr

  @property
  def name(self):
    return self._name

  def fix_offset(self, offset_seconds):
    """Drops the first int(offset_seconds * sr) rows: the recording started before the sound did."""
    if offset_seconds < 0:
      raise ValueError('cannot remove a negative offset (%s s)' % offset_seconds)
    drop = int(offset_seconds * self._sr)
    if drop > 0:
      self._signal = self._signal[drop:]


# ---------------------------------------------------------------- trigger alignment (host)
def find_temporal_offset_via_linear_regression(audio_trigger_times, eeg_trigger_times, verbose=True):
  """(how far the eeg triggers lead the audio's, number of outliers): the intercept of a Theil-Sen line
  (scipy.stats.theilslopes, 90 %) of eeg over audio trigger times, paired in order; a point further than 0.1 s
  from the unit-slope line through that intercept is an outlier (ingest.py:168-201)."""
  import scipy.stats
  n = min(len(audio_trigger_times), len(eeg_trigger_times))
  audio, eeg = audio_trigger_times[:n], eeg_trigger_times[:n]
  fit = scipy.stats.theilslopes(eeg, audio, 0.90)
  slope, intercept = fit[0], fit[1]
  if verbose and abs(slope - 1.0) > 0.01:
    logging.warning('Theil-Sen slope is not 1: %s', fit)
  outliers = np.flatnonzero(abs(eeg - (audio + intercept)) > 0.1)
  if len(outliers):
    logging.info('outliers at %s, intercept %g', outliers, intercept)
  return intercept, len(outliers)


def find_temporal_offset_via_mode_histogram(audio_triggers, eeg_triggers, max_time=0, fs=0):
  """The most frequent difference eeg - audio over every pair of events (the smallest of them on a tie, as
  scipy.stats.mode).  With fs the times are first truncated to int32 samples and the answer is in seconds,
  otherwise it is int(mode) of the raw differences; max_time keeps |difference| < max_time * fs
  (ingest.py:204-239)."""
  audio, eeg = np.asarray(audio_triggers), np.asarray(eeg_triggers)
  if fs > 0:
    audio, eeg = (audio * fs).astype(np.int32), (eeg * fs).astype(np.int32)
  diffs = (eeg[None, :] - audio[:, None]).ravel()
  if max_time != 0:
    diffs = diffs[np.abs(diffs) < max_time * fs]
  values, counts = np.unique(diffs, return_counts=True)
  mode = int(values[np.argmax(counts)])
  logging.info('find_temporal_offset_via_mode_histogram: mode %g, mean %g', mode, np.mean(diffs))
  return mode / float(fs) if fs > 0 else mode


def remove_close_times(times, min_time=0.06):
  """Trigger onsets: of the sorted times, the first and every one more than min_time after its predecessor
  (kept or not), as a float array (ingest.py:242-269)."""
  t = np.sort(np.asarray(times, dtype=np.float64).ravel())
  if t.size == 0:
    raise IndexError('remove_close_times needs at least one time')
  keep = np.ones(t.size, bool)
  keep[1:] = t[1:] > t[:-1] + min_time
  return t[keep]


# ---------------------------------------------------------------- one trial
class BrainTrial(object):
  """One trial: a sound, its brain signals (by name, in the order loaded) and the model features that go to the
  trial's TFRecord file."""

  def __init__(self, trial_name):
    self._trial_name = trial_name.replace('.wav', '') if trial_name.endswith('.wav') else trial_name
    self._sound_data, self._sound_fs = None, None
    self._brain_data = collections.OrderedDict()
    self._model_features = {}

  @property
  def model_features(self):
    return self._model_features

  @model_features.setter
  def model_features(self, new_dict):
    assert_type('audio features for trial (new_dict)', new_dict, dict)
    self._model_features = new_dict

  @property
  def brain_data(self):
    return self._brain_data

  @property
  def sound_fs(self):
    return self._sound_fs

  @property
  def sound_data(self):
    return self._sound_data

  @sound_data.setter
  def sound_data(self, new_sound):
    self._sound_data = new_sound

  @property
  def filename(self):
    return 'dummy_brain_trial'

  @property
  def trial_name(self):
    return self._trial_name

  def add_model_feature(self, name, data):
    """Files `data` (a device tensor as it is, else np.asarray) under `name`."""
    assert_type('name', name, str)
    if not self._model_features:
      self._model_features = {}
    self._model_features[name] = _as_feature(data)

  def summary_string(self):
    """'<n> EEG channels with <s>s of eeg data, <s>s of audio data, <shape> samples of <feature> data.'"""
    text = '%d EEG channels' % len(self._brain_data)
    if self._brain_data:
      first = next(iter(self._brain_data.values()))
      if isinstance(first.signal, np.ndarray) or _is_device_tensor(first.signal):
        text += ' with %gs of eeg data' % (first.signal.shape[0] / float(first.sr))
      else:
        text += 'No EEG data'
      if self._sound_data is not None:
        text += ', %gs of audio data' % (self._sound_data.shape[0] / float(self._sound_fs))
      for k, v in self._model_features.items():
        text += ', %s samples of %s data' % (tuple(v.shape), k)
    return text + '.'

  def load_sound(self, sound_data, sound_fs=None, sound_dir=None):
    """The trial's waveform as [frames, channels]: from `sound_data`.wav in sound_dir (int16 scaled by 1 / 32767
    to float32; a missing file is a ValueError), or from an array, which needs sound_fs > 0."""
    if isinstance(sound_data, str):
      import scipy.io.wavfile
      path = os.path.join(sound_dir, sound_data)
      if not path.endswith('.wav'):
        path += '.wav'
      try:
        with LocalCopy(path) as local:
          fs, wave = scipy.io.wavfile.read(local)
      except FileNotFoundError:
        raise ValueError('Can not open %s to read audio waveform.' % path)
      self._sound_fs = fs
      self._sound_data = wave.reshape(wave.shape[0], -1).astype(np.float32) / 32767.0
    else:
      wave = _as_feature(sound_data)
      if sound_fs <= 0:
        raise ValueError('a sound needs a sample rate above 0, not %s' % sound_fs)
      self._sound_data, self._sound_fs = wave.reshape(wave.shape[0], -1), sound_fs

  def load_brain_data(self, eeg_dir, brain_data):
    """Every signal of one BrainDataFile becomes a BrainSignal of this trial; several files merge."""
    assert_type('brain_data', brain_data, BrainDataFile)
    if not os.path.exists(eeg_dir):
      raise IOError('brain data directory %s does not exist.' % eeg_dir)
    brain_data.load_all_data(eeg_dir)
    for name in brain_data.signal_names:
      self._brain_data[name] = BrainSignal(name, brain_data.signal_values(name), brain_data.signal_fs(name),
                                           data_type=brain_data.data_type)

  def iterate_brain_channels(self, data_type=None):
    for sig in self._brain_data.values():
      assert_type('a_brain_signal', sig, BrainSignal)
      if data_type is None or sig.data_type == data_type:
        yield sig

  def adjust_data_sizes(self, data_dict):
    """Every entry as [frames, width] (1-D becomes a column), trimmed to the fewest frames among them; the
    dictionary is changed in place and returned.  Device tensors are sliced, not copied."""
    if not isinstance(data_dict, dict):
      raise ValueError('adjust_data_sizes needs a dict, not %s' % type(data_dict))
    for k, v in data_dict.items():
      if len(v.shape) == 1:
        data_dict[k] = v.reshape(-1, 1)
    frames = min([_BIG] + [v.shape[0] for v in data_dict.values()])
    for k, v in data_dict.items():
      if v.shape[0] != frames:
        data_dict[k] = v[:frames, :]
    return data_dict

  def find_audio_trigger_times(self, channel_with_trigger=1):
    """Seconds at which the trigger channel of the sound rises from 0 to a positive value (a 0 is assumed
    before the first sample)."""
    assert_type('self._sound_data', self._sound_data, np.ndarray)
    if channel_with_trigger > self._sound_data.shape[1]:
      raise ValueError('Trigger channel (%d) too high.' % channel_with_trigger)
    trig = np.concatenate(([0.0], self._sound_data[:, channel_with_trigger]))
    rising = (trig[:-1] == 0) & (trig[1:] > 0)
    return np.flatnonzero(rising) / float(self._sound_fs)

  def find_eeg_trigger_times(self, channel_name='TRIG'):
    """(trigger times in seconds, the raw trigger signal, the level-corrected one).  Natus' correction of their
    EDF trigger values, floor(-0.0063606452364314 (x - 5151600) - 32768 + 0.5), gives byte codes whose low bit
    is the event; a time is where that bit goes from 0 to 1."""
    if channel_name not in self._brain_data:
      raise ValueError('channel name %s not in brain data %s.' % (channel_name, list(self._brain_data)))
    chan = self._brain_data[channel_name]
    raw = _host_array(chan.signal)
    fixed = np.floor(-0.0063606452364314 * (raw - 5151600) + (-32768) + 0.5)
    bit = fixed % 2
    rising = np.logical_and(np.logical_not(bit[:-1]), bit[1:])
    return np.nonzero(rising)[0] / float(chan.sr), raw, fixed

  def find_status_trigger_times(self, channel_name='Status', mask=0xffff):
    """(times in seconds float64, codes int64) of the events of a code channel such as BioSemi's 'Status': with
    code = int64(signal) & mask (truncation toward zero), an event is a sample whose code differs from the one
    before (a 0 is assumed before the first sample, as find_audio_trigger_times does) and is not 0.  A device
    signal is searched where it is (device.code_onsets) and only the events are copied back; a NumPy one by NumPy."""
    if channel_name not in self._brain_data:
      raise ValueError('channel name %s not in brain data %s.' % (channel_name, list(self._brain_data)))
    chan = self._brain_data[channel_name]
    if _is_device_tensor(chan.signal):
      signal = chan.signal
      if signal.dtype != _torch().float64:
        signal = signal.to(_torch().float64)
      at, codes = device.code_onsets(signal.reshape(signal.shape[0], -1)[:, 0], mask)
    else:
      code = np.asarray(chan.signal).reshape(chan.signal.shape[0], -1)[:, 0].astype(np.int64) & int(mask)
      at = np.flatnonzero((code != np.concatenate(([0], code[:-1]))) & (code != 0))
      codes = code[at]
    return at / float(chan.sr), codes.astype(np.int64)

  def find_cognionix_trigger_time(self, channel_name='EXP32', level=8000):
    if channel_name not in self._brain_data:
      raise ValueError('channel name %s not in brain data %s.' % (channel_name, list(self._brain_data)))
    chan = self._brain_data[channel_name]
    above = np.nonzero(_host_array(chan.signal) > level)
    if above:
      return above[0 // float(chan.sr)]      # (as the reference: the indices above the level)
    return None

  def fix_eeg_offset(self, offset_seconds):
    """BrainSignal.fix_offset on every signal of the trial."""
    for sig in self._brain_data.values():
      sig.fix_offset(offset_seconds)

  def assemble_brain_data(self, eeg_channel_names):
    """The named channels (a list, or one comma-separated string) side by side as the float32 model feature
    'eeg', trimmed to the shortest of them.  Columns come in the order of brain_data, not of the request.  A
    duplicate or unknown name is a ValueError.  If any of the channels is a device tensor, so is the result; when
    all of them are float32 / float64 device tensors one launch builds it (device.columns_assemble), else one
    strided copy per channel does (_assemble_columns_loop): the same bits."""
    if not isinstance(eeg_channel_names, (str, list)):
      raise TypeError('eeg_channel_names must be a string or a list of strings.')
    if isinstance(eeg_channel_names, str):
      eeg_channel_names = [s.strip() for s in eeg_channel_names.split(',')]
    if len(set(eeg_channel_names)) != len(eeg_channel_names):
      raise ValueError('duplicate channel names in request: %s' % eeg_channel_names)
    for k in eeg_channel_names:
      if k not in self._brain_data:
        raise ValueError('Missing feature %s' % k)
    chosen = [s.signal for k, s in self._brain_data.items() if k in eeg_channel_names]
    frames = min([_BIG] + [s.shape[0] for s in chosen])
    width = sum(s.shape[1] for s in chosen)
    if frames > 0 and _all_float_device_tensors(chosen):
      eeg = device.columns_assemble([_rows_tensor(s) for s in chosen], frames)
    else:
      eeg = _assemble_columns_loop(chosen, frames, width)
    self._model_features['eeg'] = eeg

  def write_data_as_tfrecords(self, tf_dir, reverse_data_for_test=False):
    """Writes the model features, trimmed to a common length, to tf_dir/<trial name>.tfrecords and returns that
    name.  reverse_data_for_test writes the eeg rows back to front (data with no relation to the sound); on the
    device path the encoder reads them that way and nothing is copied."""
    assert_type('tf_dir', tf_dir, str)
    data = self.adjust_data_sizes(dict(self._model_features))
    flipped = ()
    if reverse_data_for_test:
      data['eeg']                      # (a KeyError without eeg data, as in the reference)
      flipped = ('eeg',)
    filename = os.path.join(tf_dir, self._trial_name + '.tfrecords')
    _write_tfrecords(filename, data, flipped)
    return filename


# ---------------------------------------------------------------- where signals come from
class BrainDataFile(object):
  """Abstract source of one trial's signals: names, values and sample rates."""

  def __init__(self, data_filename, data_type=None):
    self._data_filename = data_filename
    self._data_type = data_type

  @property
  def filename(self):
    return self._data_filename

  @property
  def data_type(self):
    return self._data_type

  def __str__(self):
    return "%s('%s')" % (type(self).__name__, self._data_filename)

  @property
  def signal_names(self):
    raise NotImplementedError

  def signal_values(self, name):
    raise NotImplementedError

  def signal_fs(self, _):
    raise NotImplementedError

  def load_all_data(self, _):
    pass


class MemoryBrainDataFile(BrainDataFile):
  """Signals held in a dict {channel name: 1-D or 2-D array (NumPy or device tensor)}, all at one rate."""

  def __init__(self, trial_dict, sr=64, data_type=None, name='in_memory'):
    assert_type('trial_dict', trial_dict, dict)
    if sr <= 0.0:
      raise ValueError('Sample rate must be > 0.')
    for channel_name, channel_data in trial_dict.items():
      assert_type('channel_name', channel_name, str)
      shape = tuple(_as_feature(channel_data).shape)
      if len(shape) > 2:
        raise ValueError('Bad MemoryBrainDataFile shape for %s(%s)' % (channel_name, shape))
    self._my_data_dict = trial_dict
    self._my_sr = sr
    BrainDataFile.__init__(self, name, data_type=data_type)

  @property
  def signal_names(self):
    return list(self._my_data_dict)

  def signal_values(self, name):
    return self._my_data_dict.get(name)

  def signal_fs(self, _):
    return self._my_sr


class LocalCopy(object):
  """Context manager: a temporary local copy of a file, for readers (wav, EDF) that want a plain path."""

  def __init__(self, remote_filename):
    self._remote_filename = remote_filename

  def __enter__(self):
    suffix = os.path.splitext(self._remote_filename)[1]
    self._fp = tempfile.NamedTemporaryFile(suffix=suffix)
    self._name = self._fp.name
    shutil.copyfile(self._remote_filename, self._name)
    return self._name

  def __exit__(self, exception_type, exception_value, traceback):
    self._fp.close()


def _pyedflib():
  try:
    import pyedflib
  except ImportError:
    raise ImportError('reading EDF files needs the pyedflib package, which is not installed')
  return pyedflib


def parse_edf_file(sample_edf_file):
  """{'labels', 'signals' [signal, samples], 'sample_rates', 'header', 'signal_headers'} of an EDF file
  (ingest.py:746-772).  Needs pyedflib."""
  pyedflib = _pyedflib()
  with pyedflib.EdfReader(sample_edf_file) as f:
    if not f:
      logging.error('Can not read EDF data from %s', sample_edf_file)
      return None
    count = f.signals_in_file
    signals = np.zeros((count, f.getNSamples()[0]))
    for i in range(count):
      signals[i, :] = f.readSignal(i)
    return {'labels': f.getSignalLabels(), 'signals': signals,
            'sample_rates': np.array(f.getSampleFrequencies()), 'header': f.getHeader(),
            'signal_headers': f.getSignalHeaders()}


class EdfBrainDataFile(BrainDataFile):
  """Signals from an EDF file (ingest.py:775-824).  Needs pyedflib."""

  def __init__(self, filename, data_type=None, **kwds):
    self._edf_dict = {}
    super(EdfBrainDataFile, self).__init__(filename, data_type=data_type, **kwds)

  def load_all_data(self, data_dir):
    _pyedflib()
    if not os.path.exists(data_dir):
      raise IOError('Data_dir does not exist:', data_dir)
    path = os.path.join(data_dir, self._data_filename)
    if not path.endswith('.edf'):
      path += '.edf'
    if not os.path.exists(path):
      raise IOError('Can not open %s for reading' % path)
    with LocalCopy(path) as local:
      self._edf_dict = parse_edf_file(local)

  @property
  def signal_names(self):
    return self._edf_dict['labels']

  def signal_values(self, name):
    assert_type('name', name, str)
    return self._edf_dict['signals'][self.find_channel_index(name)]

  def signal_fs(self, name):
    assert_type('name', name, str)
    return self._edf_dict['sample_rates'][self.find_channel_index(name)]

  def find_channel_index(self, desired_label='TRIG'):
    """Row of the signal with that label, None when there is none."""
    if 'labels' not in self._edf_dict:
      raise ValueError('Can not find labels among: %s' % list(self._edf_dict))
    labels = list(self._edf_dict['labels'])
    return labels.index(desired_label) if desired_label in labels else None


# ---------------------------------------------------------------- the experiment
class BrainExperiment(object):
  """Every trial of an experiment.  trial_dict: {trial name: [sound, BrainDataFile, ...]}, the sound a .wav name
  in sound_dir or a dict of features ('audio_data' with 'audio_sr' is the waveform); several BrainDataFiles of
  one trial (simultaneous recordings) merge into one BrainTrial."""

  @staticmethod
  def delete_suffix(filename, suffix):
    return filename.replace(suffix, '') if filename.endswith(suffix) else filename

  def __init__(self, trial_dict, sound_dir=None, eeg_dir=None, frame_rate=64):
    if not isinstance(trial_dict, dict):
      raise TypeError('the trials come as a dictionary, not %s' % trial_dict)
    if sound_dir:
      assert_type('sound_dir', sound_dir, str)
    if eeg_dir:
      assert_type('eeg_dir', eeg_dir, str)
    for k, v in trial_dict.items():
      assert_type('Trial name', k, str)
      assert_type('Trial data', v, list)
    self._trial_dict = trial_dict
    self._sound_dir, self._eeg_dir, self._frame_rate = sound_dir, eeg_dir, frame_rate
    self._data_dict = {}
    self._feature_mean, self._feature_std = {}, {}

  def trial_data(self, key):
    return self._data_dict.get(key)

  def add_sound_data(self, sound_dict, trial):
    """'audio_data' + 'audio_sr' of sound_dict become the trial's waveform (and leave the dict); what remains
    becomes its model features."""
    assert_type('Sound dictionary', sound_dict, dict)
    assert_type('Trial argument', trial, BrainTrial)
    if 'audio_data' in sound_dict and 'audio_sr' in sound_dict:
      trial.load_sound(sound_dict.pop('audio_data'), sound_dict.pop('audio_sr'))
    if sound_dict:
      trial.model_features = sound_dict

  def iterate_trials(self):
    for trial in self._data_dict.values():
      yield trial

  def load_all_data(self, verbose=False):
    """Builds the BrainTrial of every entry of the trial dictionary."""
    for trial_name, entries in self._trial_dict.items():
      assert_type('trial_name', trial_name, str)
      trial = BrainTrial(trial_name)
      sound = entries[0]
      if isinstance(sound, str):
        if verbose:
          logging.info('load_all_data %s: sound from %s', trial_name, sound)
        trial.load_sound(sound, sound_dir=self._sound_dir)
      elif isinstance(sound, dict):
        self.add_sound_data(sound, trial)
      else:
        raise TypeError('Can not process %s for sounds.' % type(sound))
      for source in entries[1:]:
        trial.load_brain_data(self._eeg_dir, source)
      self._data_dict[trial_name] = trial

  def check_sound_eeg_files(self):
    """IOError unless every trial's .wav is in sound_dir (and the .edf of every BrainTrial entry in eeg_dir)."""
    assert_type('self._trial_dict', self._trial_dict, dict)
    for trial_name, entries in self._trial_dict.items():
      if not os.path.exists(os.path.join(self._sound_dir, trial_name + '.wav')):
        raise IOError('Can not find %s in %s' % (trial_name, self._sound_dir))
      for entry in entries if isinstance(entries, list) else [entries]:
        if isinstance(entry, BrainTrial):
          edf = entry.filename + '.edf'
          if not os.path.exists(os.path.join(self._eeg_dir, edf)):
            raise IOError('Can not find %s in %s' % (edf, self._eeg_dir))

  def summary(self):
    lines = ['Experiment summary:',
             '  Reading sound from: %s' % self._sound_dir,
             '  Reading EEG data from: %s' % self._eeg_dir,
             '  Found %d trials' % len(self._trial_dict)]
    lines += ['    Trial %s: %s' % (name, trial.summary_string()) for name, trial in self._data_dict.items()]
    return '\n'.join(lines) + '\n'

  def get_all_feature_data(self, feature_name):
    return [t.model_features[feature_name] for t in self._data_dict.values()
            if feature_name in t.model_features]

  def zscore_all_features(self, feature_name, mean, std):
    """normalize_data(feature, mean, std) in every trial that has the feature."""
    if abs(std) == 1e-10:
      std = 1.0
    for trial in self._data_dict.values():
      features = trial.model_features
      if feature_name in features:
        features[feature_name] = normalize_data(features[feature_name], mean, std)
      trial.model_features = features

  def z_score_all_data(self):
    """Every feature of the first trial's list (but 'ones') is brought to mean 0 and standard deviation 1 over
    all the trials together.  Per feature: one moments call over every trial, one normalise launch per trial;
    device tensors never leave the device.  The moments are kept for save_zscore_data."""
    first = next(iter(self._data_dict.values()))
    for name in list(first.model_features):
      if name == 'ones':
        continue
      mean, std = find_mean_std(self.get_all_feature_data(name))
      self._feature_mean[name], self._feature_std[name] = mean, std
      self.zscore_all_features(name, mean, std)

  def save_zscore_data(self, filename):
    """Pickles {'mean': {feature: mean}, 'std': {feature: std}} of z_score_all_data (binary mode), for scaling
    the data at inference."""
    with open(filename, 'wb') as fp:
      pickle.dump({'mean': self._feature_mean, 'std': self._feature_std}, fp)

  def write_all_data(self, tf_dir):
    """One TFRecord file per trial in tf_dir; returns their names."""
    return [trial.write_data_as_tfrecords(tf_dir) for trial in self.iterate_trials()]


# ---------------------------------------------------------------- z-scoring
def find_mean_std(data_list, columnwise=False):
  """(mean, std) of all the arrays of the list together: of every entry, or per column ([1, width] arrays) when
  columnwise.  The reference's two passes (ingest.py:1061-1091) -- the sum gives the mean, then the centred
  squares are summed -- but always summed in float64 and always returned as float64 (np.float64, or float64
  [1, width]).  That is deliberately more exact than the reference, which adds float32 data up with a float32
  np.sum.  The one-pass sum-of-squares formula is never used: it cancels on EEG with a DC offset.  With a GPU
  both passes run there over all the arrays at once (device.ingest_moments), for NumPy arrays too."""
  if device.gpu_available():
    tensors = [_rows_tensor(_float_tensor(d)) for d in data_list]
    if not columnwise and len({int(t.shape[1]) for t in tensors}) > 1:
      tensors = [t.reshape(-1, 1) for t in tensors]        # (widths may only differ for the whole-matrix moments)
    width = int(tensors[0].shape[1])
    out = device.ingest_moments(tensors).cpu().numpy()
    if columnwise:
      return out[2:2 + width].reshape(1, width).copy(), out[2 + width:].reshape(1, width).copy()
    return np.float64(out[0]), np.float64(out[1])
  arrays = [_host_array(d) for d in data_list]
  axis = {'axis': 0, 'keepdims': True} if columnwise else {}
  count = sum(a.shape[0] if columnwise else a.size for a in arrays)
  mean = sum(np.sum(a, dtype=np.float64, **axis) for a in arrays) / count
  squares = sum(np.sum((a.astype(np.float64) - mean) ** 2, **axis) for a in arrays)
  std = np.sqrt(squares / count)
  if columnwise:
    return np.asarray(mean, np.float64), np.asarray(std, np.float64)
  return np.float64(mean), np.float64(std)


def normalize_data(a, data_mean, data_std):
  """(a - data_mean) / data_std in the dtypes NumPy gives those operands; an all-zero data_std (artificial data)
  only centres (ingest.py:1094-1112).  With a GPU the arithmetic runs there (device.ingest_normalize: correctly
  rounded subtraction and division, so the bits are NumPy's).  Device tensor in, device tensor out; NumPy in,
  NumPy out."""
  divide = bool(np.max(np.abs(data_std)) > 0.0)
  was_tensor = _is_device_tensor(a)
  if device.gpu_available():
    t = _float_tensor(a)
    shape = tuple(t.shape)
    t = _rows_tensor(t)
    width = int(t.shape[1])
    # the dtypes of numpy's two steps, from an empty array of a's dtype and trailing shape
    probe = np.empty((0,) + shape[1:], np.float64 if t.dtype == _torch().float64 else np.float32)
    centred = probe - data_mean
    result = centred / data_std if divide else centred
    sizes = {int(np.size(data_mean)), int(np.size(data_std))}
    per_column = (sizes == {width} and len(shape) == 2 and np.shape(data_mean)[-1:] == (width,) and
                  np.shape(data_std)[-1:] == (width,))
    if (centred.shape == probe.shape and result.shape == probe.shape and
        centred.dtype in (np.float32, np.float64) and result.dtype in (np.float32, np.float64) and
        (sizes == {1} or per_column)):
      out = device.ingest_normalize(t, data_mean, data_std, centred.dtype == np.float64,
                                    result.dtype == np.float64, divide).reshape(shape)
      return out if was_tensor else out.cpu().numpy()
  # NumPy: no GPU, or operands the kernel does not take (a broadcast that changes the shape, other dtypes)
  centred = _host_array(a) - data_mean
  out = centred / data_std if divide else centred
  return _torch().from_numpy(np.ascontiguousarray(out)).to(a.device) if was_tensor else out


# ---------------------------------------------------------------- TFRecord files
def device_record_plan(data_dict):
  """(template, [(name, payload byte offset, floats)]) (tfrecord.record_template) when the device encoder takes
  the trial -- every feature a 2-D float32 / float64 array of at least one column, at most 16 features -- else
  None: an integer (or any other) feature has no fixed record layout and goes to the host writer."""
  widths = {}
  for k, v in data_dict.items():
    if _is_device_tensor(v):
      ok = v.dtype in (_torch().float32, _torch().float64)
    else:
      ok = isinstance(v, np.ndarray) and v.dtype in (np.float32, np.float64)
    if not ok or len(v.shape) != 2 or v.shape[1] < 1:
      return None
    widths[k] = int(v.shape[1])
  if not widths or len(widths) > 16:
    return None
  return tfrecord.record_template(widths)


def _write_tfrecords(filename, data_dict, flipped=()):
  """convert_data_to_tfrecords, the features named in `flipped` written back to front."""
  assert_type('Input data_dict', data_dict, dict)
  first = next(iter(data_dict))
  frames = data_dict[first].shape[0]
  for k, v in data_dict.items():
    if v.shape[0] != frames:
      raise ValueError('Inconsistent shapes: %s %s vs %s %s' %
                       (k, tuple(v.shape), first, tuple(data_dict[first].shape)))
    if len(v.shape) != 2:
      raise ValueError('Not 2d shape for key %s: %s' % (k, tuple(v.shape)))
  plan = device_record_plan(data_dict) if (frames > 0 and device.gpu_available()) else None
  if plan is not None:
    template, layout = plan
    features = [(_rows_tensor(_float_tensor(data_dict[k])), offset, k in flipped) for k, offset, _ in layout]
    image = device.tfrecord_encode(template, features, frames)
    with open(filename, 'wb') as f:
      f.write(image.cpu().numpy().data)
    return
  host, only_floats = {}, True
  for k, v in data_dict.items():
    arr = _host_array(v)
    if arr.dtype not in (np.float64, np.float32, np.int64, np.int32):
      raise ValueError('Can\'t convert %s data to TFRecord: %s %s' % (k, type(arr), arr.dtype))
    only_floats = only_floats and arr.dtype.kind == 'f'
    host[k] = arr[::-1] if k in flipped else arr
  (tfrecord.write_file if only_floats else tfrecord.write_file_typed)(filename, host)


def convert_data_to_tfrecords(filename, data_dict):
  """Writes {feature: [frames, width]} as a TFRecord file of `frames` tf.train.Examples, every feature of a
  frame one packed list (ingest.py:1118-1172).  With a GPU a trial of float32 / float64 features (NumPy or
  device tensors) is encoded on the device: the whole file image in one launch (float64 rounded to float32 as
  astype does), one copy back, one write.  A trial with an int32 / int64 feature is written on the host, that
  feature as a packed Int64List; any other dtype is a ValueError."""
  _write_tfrecords(filename, data_dict)


def discover_feature_shapes(tfrecord_file_name):
  """{feature name: (width, dtype name)} of the file's first record: tfrecord.discover_feature_shapes'
  description, where the reference returns tf.io.FixedLenFeature([width], dtype) objects."""
  assert_type('tfrecord_file_name', tfrecord_file_name, str)
  shapes = tfrecord.discover_feature_shapes(tfrecord_file_name)
  if not shapes:
    raise ValueError('Could not read any data from tfrecord file.')
  return shapes


def count_tfrecords(tfrecord_file_name):
  """(records that parse, whether reading stopped at an error)."""
  assert_type('tfrecord_file_name', tfrecord_file_name, str)
  return tfrecord.count_tfrecords(tfrecord_file_name)


def read_tfrecords(tfrecord_file_name, start_frame=0, frame_count=512):
  """{feature: float32 [rows, width]} with rows = min(frames in the file, start_frame + frame_count); as in the
  reference (ingest.py:1245-1289) the rows before start_frame are there and zero."""
  assert_type('tfrecord_file_name', tfrecord_file_name, str)
  records = {}
  for k, v in tfrecord.read_file(tfrecord_file_name).items():
    rows = min(v.shape[0], start_frame + frame_count)
    out = np.zeros((rows, v.shape[1]), dtype=np.float32)
    out[start_frame:rows] = v[start_frame:rows]
    records[k] = out
  return records


def transform_tfrecords(input_file, new_tf_dir, trial_name, transforms):
  """Reads a TFRecord file whole, adds (name, data) = transform(data dictionary) for every transform in turn,
  and writes the result as new_tf_dir/<trial_name>.tfrecords; returns that name."""
  count, errors = count_tfrecords(input_file)
  if errors:
    raise ValueError('Found errors after reading %d records from %s.' % (count, input_file))
  data = read_tfrecords(input_file, frame_count=count)
  for transform in transforms:
    name, values = transform(data)
    data[name] = values
  trial = BrainTrial(trial_name)
  for k, v in data.items():
    trial.add_model_feature(k, v)
  return trial.write_data_as_tfrecords(new_tf_dir)
