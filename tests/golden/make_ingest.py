"""Golden G19: the reference's own ingest.py run through tests/golden/ref_shim on the inputs of
tests/host_ingest.py, stored as data for tests/test_cpu_ingest.py and tests/test_gpu_ingest.py.
   python tests/golden/make_ingest.py   (needs the reference's sources on REFERENCE_ROOT, default
/root/reference, and scipy)

The reference's module imports pyedflib and more of tensorflow than the shim has; neither is used by what runs
here, so this script puts stand-ins for them into sys.modules before the import (the shim's files stay as they
are).  The inputs are not stored: host_ingest regenerates them and G19 keeps their checksums.

g19_ingest.npz: remove_close_times, both offset estimators, the audio and the Natus trigger edges, fix_offset,
assemble_brain_data (result, and which bad requests raise), adjust_data_sizes, the summary strings of the
reference's test_brain_memory_experiment, and find_mean_std (whole and columnwise) on the G19 moment cases.
g19_ingest_surface.json: the reference's ingest signatures.
"""
import collections
import json
import os
import shutil
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, 'ref_shim'))
sys.path.insert(0, os.environ.get('REFERENCE_ROOT', '/root/reference'))
import numpy as np  # noqa: E402

sys.modules.setdefault('pyedflib', types.ModuleType('pyedflib'))
import tensorflow as tf  # noqa: E402  (the shim)

if not hasattr(tf, 'io'):
  tf.io = types.SimpleNamespace()
if not hasattr(tf.io, 'FixedLenFeature'):
  tf.io.FixedLenFeature = object
if not hasattr(tf.io, 'gfile'):
  tf.io.gfile = types.SimpleNamespace(exists=os.path.exists,
                                      copy=lambda src, dst, overwrite=False: shutil.copyfile(src, dst))

from telluride_decoding import ingest as ref  # noqa: E402
from tests import host_ingest as hi  # noqa: E402
from tests import surface  # noqa: E402


def main():
  out = {}
  for name, (times, min_time) in hi.close_times_cases().items():
    out['close_%s_xsum' % name] = hi.checksum(times)
    out['close_%s' % name] = np.asarray(ref.remove_close_times(times, min_time=min_time))
  for name, (audio, eeg) in hi.regression_cases().items():
    out['regress_%s_xsum' % name] = hi.checksum(np.concatenate((audio, eeg)))
    out['regress_%s' % name] = np.array(ref.find_temporal_offset_via_linear_regression(audio, eeg, verbose=False),
                                        np.float64)
  for name, (a, e, max_time, fs) in hi.histogram_cases().items():
    out['hist_%s_xsum' % name] = hi.checksum(np.concatenate((a, e)))
    out['hist_%s' % name] = np.float64(ref.find_temporal_offset_via_mode_histogram(a, e, max_time=max_time, fs=fs))

  sound, fs = hi.pulse_train()
  trial = ref.BrainTrial('pulses')
  trial.load_sound(sound, sound_fs=fs)
  out['pulse_xsum'] = hi.checksum(sound)
  out['pulse_times'] = np.asarray(trial.find_audio_trigger_times())

  raw, sr = hi.natus_signal()
  trial = ref.BrainTrial('natus')
  trial.load_brain_data(HERE, ref.MemoryBrainDataFile({'TRIG': raw}, sr))
  times, raw_back, fixed = trial.find_eeg_trigger_times()
  out['natus_xsum'] = hi.checksum(raw)
  out['natus_times'], out['natus_fixed'] = np.asarray(times), np.asarray(fixed)

  for i, (signal, sr, seconds) in enumerate(hi.fix_offset_cases()):
    s = ref.BrainSignal('s', signal, sr)
    s.fix_offset(seconds)
    out['offset_%d' % i] = np.asarray(s.signal)

  chans, sr, request = hi.assemble_channels()
  trial = ref.BrainTrial('assemble')
  trial.load_brain_data(HERE, ref.MemoryBrainDataFile(collections.OrderedDict(chans), sr))
  trial.assemble_brain_data(list(request))
  out['assemble_xsum'] = hi.checksum(np.concatenate([np.asarray(d, np.float64).ravel() for _, d in chans]))
  out['assemble_eeg'] = trial.model_features['eeg']
  trial.assemble_brain_data(', '.join(request))
  out['assemble_eeg_csv'] = trial.model_features['eeg']
  for key, bad in (('dup', ['TRIG', 'TRIG', 'Fp2']), ('missing', 'TRIG, FOO, BAR')):
    try:
      trial.assemble_brain_data(bad)
      out['assemble_%s_raises' % key] = np.int64(0)
    except ValueError:
      out['assemble_%s_raises' % key] = np.int64(1)

  data = hi.adjust_inputs()
  out['adjust_xsum'] = hi.checksum(np.concatenate([v.ravel().astype(np.float64) for v in data.values()]))
  for k, v in ref.BrainTrial('adjust').adjust_data_sizes(dict(data)).items():
    out['adjust_' + k] = v

  audio, fs, eeg, frame_sr = hi.memory_experiment_inputs()
  df = ref.MemoryBrainDataFile(collections.OrderedDict(eeg), frame_sr)
  exp = ref.BrainExperiment({'trial_2': [{'audio_data': audio, 'audio_sr': fs}, df]}, HERE, HERE,
                            frame_rate=frame_sr)
  exp.load_all_data()
  out['summary_loaded'] = np.array(exp.summary().replace(HERE, '<dir>'))
  for t in exp.iterate_trials():
    t.assemble_brain_data([k for k, _ in eeg])
  out['summary_assembled'] = np.array(exp.summary().replace(HERE, '<dir>'))

  for name, rows, width, dtype in hi.G19_MOMENT_CASES:
    arrays = hi.moments_data(name, rows, width, dtype)
    out['moments_%s_xsum' % name] = hi.checksum(np.concatenate(arrays))
    mean, std = ref.find_mean_std(arrays)
    out['moments_%s_all' % name] = np.array([mean, std], np.float64)
    mean, std = ref.find_mean_std(arrays, columnwise=True)
    out['moments_%s_mean' % name], out['moments_%s_std' % name] = np.asarray(mean), np.asarray(std)

  np.savez_compressed(os.path.join(HERE, 'g19_ingest.npz'), **out)
  with open(os.path.join(HERE, 'g19_ingest_surface.json'), 'w') as fp:
    json.dump(surface.module_surface(ref), fp, indent=1, sort_keys=True)
  print('wrote g19_ingest.npz, g19_ingest_surface.json')


if __name__ == '__main__':
  main()
