"""Golden G18: the reference's own preprocess.AudioFeatures (preprocess.py:589-755) run through
tests/golden/ref_shim, stored as data for tests/test_cpu_audio.py and tests/test_gpu_audio.py.
   python tests/golden/make_audio.py   (needs the reference's sources on REFERENCE_ROOT, default
/root/reference, and scipy)

The inputs are not stored: tests/host_audio.py regenerates them (integer draws for the intensity cases) and
checks them against the stored checksums; a spectrogram wider than 64 frames keeps every 5th frame.

g18_audio.npz: every intensity case of tests/host_audio.py (16 / 44.1 / 48 kHz to 64 / 100 Hz, window 1, 2.5
and 3, mono and stereo, the pass-through and the NaN case, a user buffer) whole and streamed in uneven calls
(1-frame mono calls among them), with the buffer left after each call; the reference test's Gaussian-windowed
440 Hz tone; the spectrogram cases (the default shape, the reference test's, (256, 4, 2), (100, 3, 3) with a
two-tap filter, a 120-sample wave, an all-zero wave) and which short waves raise.
g18_audio_surface.json: the reference's AudioFeatures signatures.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, 'ref_shim'))
sys.path.insert(0, os.environ.get('REFERENCE_ROOT', '/root/reference'))
import numpy as np  # noqa: E402

from absl import logging  # noqa: E402

logging.log_first_n = lambda *a, **k: None     # the shim has none; the reference only logs through it

from telluride_decoding import preprocess as ref_pre  # noqa: E402
from tests import host_audio as ha  # noqa: E402
from tests import surface  # noqa: E402


def user_buffer(name, rows, channels):
  rng = np.random.default_rng(sum(map(ord, name)) + 1)
  b = np.round(1000 * rng.random((rows, channels))) ** 2
  return b.astype(np.float64 if name == 'passup' else np.float32)


def main():
  out = {}
  for name, fs_in, fs_out, window, exponent, c, n, calls, brows in ha.INTENSITY_CASES:
    x = ha.intensity_input(name, fs_in, c, n)
    out[name + '_xsum'] = ha.checksum(x)
    buff = user_buffer(name, brows, c) if brows else None
    if buff is not None:
      out[name + '_buff'] = buff
    p = ref_pre.AudioFeatures('g18', fs_in, fs_out, window=window, exponent=exponent,
                              buff=None if buff is None else buff.copy())
    out[name + '_whole'] = p.compute_intensity(x.copy())
    out[name + '_whole_buff'] = np.asarray(p._buff)
    p = ref_pre.AudioFeatures('g18', fs_in, fs_out, window=window, exponent=exponent,
                              buff=None if buff is None else buff.copy())
    out[name + '_calls'] = np.array(calls, np.int64)
    s = 0
    for i, m in enumerate(calls):
      piece = x[s:s + m]
      if c == 1:
        piece = piece[:, 0]           # mono calls as 1-D waves
      out['%s_call%d' % (name, i)] = p.compute_intensity(piece.copy())
      out['%s_buff%d' % (name, i)] = np.asarray(p._buff)
      s += m
    p = ref_pre.AudioFeatures('g18', fs_in, fs_out, window=window, exponent=exponent)
    out[name + '_resample'] = p.audio_resample(x.copy())
  x, _ = ha.tone_440()
  out['tone_xsum'] = ha.checksum(x)
  p = ref_pre.AudioFeatures('test', 16000, 100, window=1, exponent=np.log10(2), buff=None)
  out['tone_out'] = p.compute_intensity(x)
  p = ref_pre.AudioFeatures('g18', 16000, 100)
  for name, samples, seg, nov, ntr, smooth in ha.SPECTROGRAM_CASES:
    wave = ha.spectrogram_input(name, samples)
    kw = {k: v for k, v in (('segment_size', seg), ('n_overlap', nov), ('n_trans', ntr),
                            ('smoothing_filter', smooth)) if v is not None}
    out['spec_%s_xsum' % name] = ha.checksum(wave)
    out['spec_%s_kwargs' % name] = np.array(json.dumps(kw))
    with np.errstate(invalid='ignore', divide='ignore'):
      s, f = p.compute_spectrogram(wave, **kw)
    cols = ha.golden_columns(s.shape[1])
    out['spec_%s_shape' % name] = np.array(s.shape, np.int64)
    out['spec_%s_cols' % name] = cols
    out['spec_%s_out' % name], out['spec_%s_f' % name] = s[:, cols], f
  for name, samples in ha.SPECTROGRAM_RAISES:
    try:
      p.compute_spectrogram(ha.spectrogram_input(name, samples))
      out['spec_%s_raises' % name] = np.int64(0)
    except ValueError:
      out['spec_%s_raises' % name] = np.int64(1)
  np.savez_compressed(os.path.join(HERE, 'g18_audio.npz'), **out)
  with open(os.path.join(HERE, 'g18_audio_surface.json'), 'w') as fp:
    json.dump(surface.module_surface(ref_pre)['AudioFeatures'], fp, indent=1, sort_keys=True)
  print('wrote g18_audio.npz, g18_audio_surface.json')


if __name__ == '__main__':
  main()
