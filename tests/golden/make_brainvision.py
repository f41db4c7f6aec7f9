"""Golden G20: the reference's own ingest_brainvision.py run through tests/golden/ref_shim on its test recording
(tests/golden/brainvision_test.vhdr / .eeg / .vmrk, copies of the reference's test_data files), stored as data for
tests/test_cpu_raw_ingest.py and tests/test_gpu_raw_ingest.py.
   python tests/golden/make_brainvision.py   (needs the reference's sources on REFERENCE_ROOT, default
/root/reference, and scipy)

The reference reads through tf.io.gfile, which the shim does not have; this script supplies GFile and exists
stand-ins over the local file system (and the stand-ins make_ingest.py needs to import the reference's ingest)
before the import, so the shim's files stay as they are.

g20_brainvision.npz: read_bv_file's matrix and header (JSON), every channel's signal_values, signal_fs, the channel
indices the reference's test asks for, and the BrainExperiment summary of the recording with an in-memory sound.
g20_brainvision_surface.json: the reference's ingest_brainvision signatures.
"""
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
import tensorflow.compat.v2 as tf2  # noqa: E402


def _gfile(name, mode='r'):
  name = name.decode('utf-8') if isinstance(name, bytes) else name
  return open(name, mode) if 'b' in mode else open(name, mode, encoding='utf-8')


for module in (tf, tf2):
  if not hasattr(module, 'io'):
    module.io = types.SimpleNamespace()
  if not hasattr(module.io, 'FixedLenFeature'):
    module.io.FixedLenFeature = object
  module.io.gfile = types.SimpleNamespace(exists=os.path.exists, GFile=_gfile,
                                          copy=lambda src, dst, overwrite=False: shutil.copyfile(src, dst))

from telluride_decoding import ingest as ref_ingest  # noqa: E402
from telluride_decoding import ingest_brainvision as ref  # noqa: E402
from tests import surface  # noqa: E402

NAME = 'brainvision_test.vhdr'


def main():
  out = {}
  header, data = ref.read_bv_file(os.path.join(HERE, NAME))
  out['data'] = np.asarray(data)
  out['header_json'] = np.array(json.dumps(header))
  bv = ref.BvBrainDataFile(NAME)
  bv.load_all_data(HERE)
  names = bv.signal_names
  out['names_json'] = np.array(json.dumps(names))
  for i, name in enumerate(names):
    out['values_%02d' % i] = np.asarray(bv.signal_values(name))
  out['signal_fs'] = np.float64(bv.signal_fs('foo'))
  out['index_default'] = np.int64(bv.find_channel_index())
  out['index_TRIG'] = np.int64(bv.find_channel_index('TRIG'))
  out['index_C3'] = np.int64(bv.find_channel_index('C3'))
  out['missing_is_none'] = np.int64(bv.signal_values('CH1') is None)

  sound = np.zeros((1000, 1), np.float32)
  exp = ref_ingest.BrainExperiment({'subj01_1ksamples': [{'audio_data': sound, 'audio_sr': 16000},
                                                         ref.BvBrainDataFile(NAME)]}, HERE, HERE)
  exp.load_all_data()
  out['summary'] = np.array(exp.summary().replace(HERE, '<dir>'))

  np.savez_compressed(os.path.join(HERE, 'g20_brainvision.npz'), **out)
  with open(os.path.join(HERE, 'g20_brainvision_surface.json'), 'w') as fp:
    json.dump(surface.module_surface(ref), fp, indent=1, sort_keys=True)
  print('wrote g20_brainvision.npz, g20_brainvision_surface.json')


if __name__ == '__main__':
  main()
