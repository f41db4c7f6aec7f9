"""Goldens G16 / G17: the reference's own preprocess.Preprocessor (preprocess.py:54-587, scipy's sosfilt
in float64) run through tests/golden/ref_shim, stored as data for tests/test_cpu_preprocess.py and
tests/test_gpu_preprocess.py.   python tests/golden/make_preprocess.py   (needs the reference's sources
on REFERENCE_ROOT, default /root/reference, and scipy)

G16 (g16_preprocess.npz): small cases, each whole and streamed in uneven calls (one with reset=True
mid-stream): inputs, per-call outputs, the cascade, the final filter states, _next_frame_idx and the
resample indices; a multi-file run and the preprocessed streams of a small fit.
G17 (g17_preprocess_long.npz): P1 (64 ch x 1e6 frames at 1000 Hz, high-pass 0.1 Hz order 4 + the automatic
order-10 low-pass, to 100 Hz, global re-reference, normalisation) -- its input regenerated from a seed with
synth, so only sampled output rows and the final states are stored.
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

from telluride_decoding import preprocess as ref_pre  # noqa: E402
from tests import surface  # noqa: E402
from tests.host_preprocess import P1, p1_input, p1_rows  # noqa: E402

# name -> (constructor kwargs, channels, frames, streamed call lengths, call index that passes reset=True)
CASES = {
    'a': (dict(fs_in=1000, fs_out=100, highpass_cutoff=1, highpass_order=2, channels_to_ref=[list(range(6))],
               data_mean=None, data_std=2), 6, 4000, [1230, 770, 2000], 2),
    'b': (dict(fs_in=128, fs_out=128, highpass_cutoff=0.5, highpass_order=4, lowpass_cutoff=30, lowpass_order=4,
               ref_channels=[[0], [5, 8]], channels_to_ref=[[1, 2, 3], [4, 6, 7, 3]], channel_numbers='0-3,7',
               pre_context=2, post_context=3), 9, 3000, [1000, 333, 1667], 1),
    'c': (dict(fs_in=500, fs_out=64), 4, 2503, [2503], None),
    'd': (dict(fs_in=100, fs_out=100, highpass_cutoff=0.5, highpass_order=2), 1, 1500, [700, 800], None),
}


def make(kw):
  kw = dict(kw)
  return ref_pre.Preprocessor('g16', kw.pop('fs_in'), kw.pop('fs_out'), **kw)


def states(p):
  hs = getattr(p, '_highpass_state', None) if p._highpass_sos is not None else None
  ls = getattr(p, '_lowpass_state', None) if p._lowpass_sos is not None else None
  return [s for s in (hs, ls) if s is not None]


def signal(rng, n, c, fs):
  t = np.arange(n)[:, None] / fs
  x = 3.0 + 0.5 * np.sin(2 * np.pi * 0.2 * t + np.arange(c)) + np.sin(2 * np.pi * 7 * t * (1 + np.arange(c) / 10))
  return (x + rng.standard_normal((n, c))).astype(np.float32)


def g16():
  rng = np.random.default_rng(16)
  out = {}
  for name, (kw, c, n, calls, reset_at) in CASES.items():
    x = signal(rng, n, c, kw['fs_in'])
    out[name + '_x'] = x
    out[name + '_kwargs'] = np.array(json.dumps(kw))
    p = make(kw)
    out[name + '_whole'] = np.asarray(p.process(x.copy()), np.float64)
    out[name + '_sos'] = np.concatenate([s for s in (p._highpass_sos, p._lowpass_sos) if s is not None])
    fs = states(p)
    out[name + '_whole_state'] = np.concatenate(fs) if fs else np.zeros((0, 2, c))
    out[name + '_whole_next'] = np.int64(p._next_frame_idx)
    out[name + '_data_mean'] = np.float64(p._data_mean)
    p = make(kw)
    s = 0
    out[name + '_calls'] = np.array(calls, np.int64)
    for i, m in enumerate(calls):
      y = p.process(x[s:s + m].copy(), reset=(i == reset_at))
      out['%s_call%d' % (name, i)] = np.asarray(y, np.float64)
      s += m
    fs = states(p)
    out[name + '_stream_state'] = np.concatenate(fs) if fs else np.zeros((0, 2, c))
    out[name + '_stream_next'] = np.int64(p._next_frame_idx)
    out[name + '_reset_at'] = np.int64(-1 if reset_at is None else reset_at)
    if kw['fs_out'] != kw['fs_in']:
      q = make(dict(fs_in=kw['fs_in'], fs_out=kw['fs_out']))
      out[name + '_idx'] = q.resample(np.arange(n, dtype=np.float64)[:, None])[:, 0].astype(np.int64)
  # case c: a second call after a misaligned first one raises (the reference's ValueError)
  p = make(CASES['c'][0])
  p.process(out['c_x'].copy())
  try:
    p.process(out['c_x'][:100].copy())
    out['c_second_raises'] = np.int64(0)
  except ValueError:
    out['c_second_raises'] = np.int64(1)
  # multi-file: case a's settings, two recordings, each processed as a fresh stream by ONE object
  xa = signal(rng, 3500, 6, 1000)
  out['multi_x'] = xa
  out['multi_offsets'] = np.array([0, 2000, 3500], np.int64)
  p = make(CASES['a'][0])
  for f in range(2):
    p.context_reset()
    p._next_frame_idx = 0
    a, b = out['multi_offsets'][f:f + 2]
    out['multi_out%d' % f] = np.asarray(p.process(xa[a:b].copy(), reset=True), np.float64)
  # a small fit: two recordings of 9-channel EEG at 128 Hz (case b's filters, re-reference and channels, no
  # context) and an envelope, preprocessed per file
  fit_kw = dict(CASES['b'][0])
  fit_kw.update(pre_context=0, post_context=0)
  out['fit_kwargs'] = np.array(json.dumps(fit_kw))
  for f, n in enumerate((2600, 2100)):
    eeg = signal(rng, n, 9, 128)
    env = (np.abs(eeg[:, :3]).mean(axis=1, keepdims=True) + 0.1 * rng.standard_normal((n, 1))).astype(np.float32)
    out['fit_eeg%d' % f], out['fit_env%d' % f] = eeg, env
    p = make(fit_kw)
    out['fit_pre%d' % f] = np.asarray(p.process(eeg.copy(), reset=True), np.float64)
  np.savez_compressed(os.path.join(HERE, 'g16_preprocess.npz'), **out)
  with open(os.path.join(HERE, 'g16_preprocess_surface.json'), 'w') as f:
    json.dump(surface.module_surface(ref_pre)['Preprocessor'], f, indent=1, sort_keys=True)
  print('wrote g16_preprocess.npz, g16_preprocess_surface.json')


def g17():
  x = p1_input()
  kw = dict(P1)
  p = make(kw)
  y = np.asarray(p.process(x), np.float64)
  rows = p1_rows(y.shape[0])
  np.savez_compressed(os.path.join(HERE, 'g17_preprocess_long.npz'), rows=rows, y_rows=y[rows],
                      n_out=np.int64(y.shape[0]), state=np.concatenate(states(p)),
                      data_mean=np.float64(p._data_mean), x_head=x[:4, :4].copy(),
                      x_sum=np.float64(x.astype(np.float64).sum()))
  print('wrote g17_preprocess_long.npz')


if __name__ == '__main__':
  g16()
  if '--no-long' not in sys.argv:
    g17()
