"""Shared by the online DNN calibration tests (CPU and GPU): labelled white-noise stretches with a
host_online_dnn.glorot_model on them, the float64 prediction of online._HostDnnSession on a whole stretch, the LDS
formula of a launch restated, and banks built around given weights.  The twin of the sums, the closed form, the
two-pass route, the cuts and the walk of a cut are tests/host_online_calib.py's: the state is td_calib_online_push's.
Everything is computed once per key and shared: treat what these functions return as read-only."""
import numpy as np

from tests import host_online_dnn as hd

SEED = 4471
LDS_BUDGET = 160 * 1024                    # TD_FC_ONLINE_LDS_BYTES

_STRETCHES = {}


def host_pred(eeg, weights, pre, post):
  """The float64 prediction of every frame of a whole stretch, zero rows before and behind it: the method of
  online._HostDnnSession itself (so: the host calibration session's prediction, bit for bit)."""
  from telluride_decoding_amd import online
  frames, c = eeg.shape
  sess = online._HostDnnSession(dict(c=c, pre=pre, post=post, weights=weights), 1, 1, 'wta')
  rows = np.concatenate([np.zeros((pre, c)), np.asarray(eeg, np.float64), np.zeros((post, c))])
  return sess._predict(rows, 0, frames)


def stretch(shape, hidden, frames, seed=0, offset=1.0):
  """dict(c, pre, post, hidden, frames, eeg [frames, c], att [frames], unatt [frames] float32, weights, pred64):
  white-noise EEG, a glorot_model whose output bias is moved so that the prediction's mean is `offset` of its
  standard deviations, an attended envelope that follows the standardised prediction and an unattended one that
  does not, with means of offset and offset / 2 (the streams have unit scale)."""
  key = (tuple(shape), tuple(hidden), frames, seed, offset)
  if key not in _STRETCHES:
    c, pre, post = shape
    rng = np.random.default_rng(SEED + 7919 * seed + 31 * c + 5 * pre + post + 3 * len(hidden))
    eeg = rng.standard_normal((frames, c)).astype(np.float32)
    ws = hd.glorot_model(c, pre, post, hidden, seed=5 + seed)
    raw = host_pred(eeg, ws, pre, post)
    sd = float(raw.std())
    ws[-1] = (ws[-1] + np.float32(offset * sd - raw.mean())).astype(np.float32)
    pred = host_pred(eeg, ws, pre, post)
    att = (0.6 * (pred - pred.mean()) / sd + 0.8 * rng.standard_normal((frames,)) + offset).astype(np.float32)
    unatt = (rng.standard_normal((frames,)) + 0.5 * offset).astype(np.float32)
    for a in [eeg, att, unatt, pred] + ws:
      a.setflags(write=False)
    _STRETCHES[key] = dict(c=c, pre=pre, post=post, hidden=list(hidden), frames=frames, eeg=eeg, att=att,
                           unatt=unatt, weights=ws, pred64=pred)
  return _STRETCHES[key]


def constant_model(st, value=0.5):
  """The stretch's network with every weight zero and the output bias `value`: every prediction is `value`."""
  ws = [np.zeros_like(w) for w in st['weights']]
  ws[-1] = np.full_like(ws[-1], value)
  return ws


def bank(st, weights=None, reduction='first', lda=None, width=20, hop=10, kind='wta', stats=(0.1, 0.2, 0.9)):
  """An OnlineDecoder bank around the stretch's network -- `weights`: one model (None: the stretch's) or a list of
  models, one session each."""
  from telluride_decoding_amd import online
  models = [st['weights']] if weights is None else (weights if isinstance(weights[0], list) else [weights])
  decs = [hd.dnn_decoder(st['c'], st['pre'], st['post'], st['hidden'], ws, stats, reduction, lda) for ws in models]
  return online.OnlineDecoder(decs, width, hop, decoder_type=kind)


def lds_formula(c, pre, post, hidden, pass_):
  """bytes(pass) of a td_fccalib_online_push launch: 8 (4 pass) for the frames' {1, p, a, u}, then float32: two chunks
  of W1, the small parameters, the staged rows on an odd stride, the envelopes, the predictions, two activation
  buffers."""
  k = c * (pre + 1 + post)
  widths = [k] + list(hidden) + [1]
  ks, slices = hd.slices_of(k)
  nj = -(-widths[1] // 4) * 4
  g = min(slices, 4096 // (ks * nj))
  n_small = sum(widths[i] * widths[i + 1] + widths[i + 1] for i in range(len(widths) - 1)) - k * widths[1]
  lda = max(list(hidden) + [1]) | 1
  return 32 * pass_ + 4 * (2 * g * ks * nj + -(-n_small // 4) * 4 + (pass_ + pre + post) * (c | 1) +
                           2 * max(pass_, post) + pass_ + 2 * pass_ * lda)


def lds_plan(c, pre, post, hidden, emitted):
  """(frames per pass, bytes): 64 frames, fewer for a short push, halved (rounding up) until the budget holds."""
  pass_ = min(64, max(emitted, 1))
  while pass_ > 1 and lds_formula(c, pre, post, hidden, pass_) > LDS_BUDGET:
    pass_ = (pass_ + 1) // 2
  return pass_, lds_formula(c, pre, post, hidden, pass_)
