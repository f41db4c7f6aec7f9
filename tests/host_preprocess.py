"""Host float64 restatement of the preprocessing chain, for the CPU tests against G16 and the GPU sweep, and
P1's input.  The sequential filter is scipy.signal.sosfilt (the reference's own routine) where scipy imports,
else scipy's recurrence written out in NumPy (vectorised over channels, one Python step per frame: callers
shorten long inputs to NUMPY_MAX_ROWS on that path).  REF_PATH says which one runs.  Test infrastructure."""
import json

import numpy as np

from telluride_decoding_amd import iir
from telluride_decoding_amd import preprocess as pp


def sosfilt(sos, x, zi):
  """scipy.signal.sosfilt(sos, x, zi=zi, axis=0) in float64: (y, final state)."""
  z = np.array(zi, np.float64, copy=True)
  y = np.empty(x.shape, np.float64)
  for t in range(x.shape[0]):
    v = x[t].astype(np.float64)
    for s in range(sos.shape[0]):
      b0, b1, b2, _, a1, a2 = sos[s]
      out = b0 * v + z[s, 0]
      z[s, 0] = b1 * v - a1 * out + z[s, 1]
      z[s, 1] = b2 * v - a2 * out
      v = out
    y[t] = v
  return y, z


def _scipy_signal():
  try:
    import scipy.signal as ss
  except ImportError:
    return None
  return ss


REF_PATH = 'scipy' if _scipy_signal() is not None else 'numpy'
NUMPY_MAX_ROWS = 20000


def ref_rows(n):
  """The rows a long case keeps: all of them with scipy, at most NUMPY_MAX_ROWS on the NumPy path."""
  return n if REF_PATH == 'scipy' else min(n, NUMPY_MAX_ROWS)


def sosfilt_ref(sos, x, zi):
  """The float64 sequential reference filter: (y, final state), x [N, C], zi [S, 2, C]."""
  x = np.asarray(x, np.float64)
  zi = np.asarray(zi, np.float64)
  if REF_PATH == 'scipy':
    return _scipy_signal().sosfilt(sos, x, axis=0, zi=zi)
  return sosfilt(sos, x, zi)


class HostPreprocessor(object):
  """The reference's Preprocessor.process, restated on the host with the package's own designer."""

  def __init__(self, kwargs):
    kw = dict(json.loads(kwargs) if isinstance(kwargs, str) else kwargs)
    self.kw = kw
    spec = pp.Preprocessor('host', kw['fs_in'], kw['fs_out'],
                           **{k: v for k, v in kw.items() if k not in ('fs_in', 'fs_out')})
    self.stages = [(s, iir.sosfilt_zi(s)) for s in (spec._highpass_sos, spec._lowpass_sos) if s is not None]
    self.states = [None] * len(self.stages)
    self.spec = spec
    self.mean = kw.get('data_mean', 0)
    self.std = kw.get('data_std', 1)
    self.ctx = None
    self.next_idx = 0

  def process(self, x, reset=False):
    y = np.asarray(x)
    for i, (sos, zi) in enumerate(self.stages):
      if self.states[i] is None or reset:
        self.states[i] = y[0, :].astype(np.float64) * zi[:, :, None]
      y, self.states[i] = sosfilt_ref(sos, y, self.states[i])
    y = y.astype(np.float64)
    if self.kw['fs_out'] != self.kw['fs_in']:
      assert self.next_idx == 0
      idx, self.next_idx = pp.resample_indices(y.shape[0], self.kw['fs_in'], self.kw['fs_out'])
      y = y[idx]
    ref, chans = self.kw.get('ref_channels'), self.kw.get('channels_to_ref')
    if ref is not None or chans is not None:
      ref = ref if ref is not None else [range(y.shape[1])]
      chans = chans if chans is not None else [range(y.shape[1])]
      d = y.copy()
      y = y.copy()
      for r, ch in zip(ref, chans):
        y[:, list(ch)] -= np.mean(d[:, list(r)], axis=1, keepdims=True)
    if self.spec.channel_numbers:
      y = y[:, self.spec.channel_numbers]
    if self.mean is None:
      self.mean = np.mean(y)
    y = (y - self.mean) / self.std
    pre, post = self.kw.get('pre_context', 0), self.kw.get('post_context', 0)
    if pre == 0 and post == 0:
      return y
    if self.ctx is None:
      self.ctx = np.zeros((pre, y.shape[1]))
    cat = np.concatenate([self.ctx, y])
    self.ctx = cat[-(pre + post):]
    rows = cat.shape[0] - pre - post
    return np.concatenate([cat[b:b + rows] for b in range(pre + post + 1)], axis=1)

  def state(self):
    return np.concatenate(self.states) if self.states else None


def p1_input():
  """P1's input: 64 channels x 1e6 frames of synth's EEG plus a 2-unit offset and slow drift (float32)."""
  from telluride_decoding_amd import synth
  eeg, _, _ = synth.make_trials(17, 1, 1000000, 64)[0]
  t = np.arange(eeg.shape[0], dtype=np.float64)[:, None] / 1000.0
  return (eeg + 2.0 + 0.5 * np.sin(2 * np.pi * 0.05 * t)).astype(np.float32)


P1 = dict(fs_in=1000, fs_out=100, highpass_cutoff=0.1, highpass_order=4, channels_to_ref=[list(range(64))],
          data_mean=None, data_std=1)


def p1_rows(n_out):
  """The output rows G17 keeps: every 997th and the last 2 000."""
  return np.unique(np.concatenate([np.arange(0, n_out, 997), np.arange(n_out - 2000, n_out)]))
