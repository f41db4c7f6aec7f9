"""Online attention decoding: EEG in chunks, decisions out, the state on the device.

The reference is built for streaming -- `Preprocessor.process(..., reset=False)`, `Decoder.infer_one` per
minibatch, stateful attention decoders -- because that is the application: a device that learns every few
hundred milliseconds whom the listener attends to.  `OnlineDecoder` is that loop's decoding stage for a
bank of S independent listeners: a push of n frames is ONE launch (td_online_push, one workgroup per
listener) that predicts the envelope from the EEG, scores it against both speakers with the decoder's
trained statistics, averages the scores over every window the push completes and decides.  Whatever a
session carries between pushes lives in its state block on the device.  However a recording is cut into
pushes, the results are those of the whole recording in one push, bit for bit.

The prediction of frame t needs the EEG up to t + post_context, so results run `post` frames behind the
input; `flush()` ends the recording (zero rows behind it, like the batch route's padding) and emits the rest.

    prep = preprocess.Preprocessor('eeg', 1000.0, 100.0, highpass_cutoff=1.0, lowpass_cutoff=8.0)
    online = OnlineDecoder.from_model_dir(model_dir, 'first', window_size=500, decoder_type='stepped')
    first = True
    for raw_eeg, env1, env2 in chunks:           # raw_eeg [n_raw, C] at 1 kHz, envelopes at 100 Hz
      eeg = prep.process(raw_eeg, reset=first)   # the filters carry their state too
      first = False
      result = online.push(eeg, env1, env2)
      for k, decision in enumerate(result.decisions[0]):
        print('window %d: speaker %d' % (result.first_window + k, 1 if decision else 2))
    result = online.flush()

A CCA experiment decodes the same way: a `CCADecoder` around a fitted `BrainModelCCA` (or the model directory
`decoding.py --dnn_regressor cca --saved_model_dir` wrote) gives a session whose push takes one block of audio
features per speaker, `online.push(eeg, feat1, feat2)`, and is ONE td_cca_online_push launch: the EEG view
centred and rotated once per frame, each speaker's view against it over the model's dims, then the same
windows and decisions.

So does the fully connected regressor: a `LinearRegressionDecoder` around a `brain_model.BrainModelDNN` (or the
model directory `decoding.py --dnn_regressor fullyconnected --saved_model_dir` wrote) gives a session whose push
is ONE td_fc_online_push launch -- the network on every emitted frame's lagged EEG, with the bits of
`device.mlp_forward` on the whole recording, then the same scores, windows and decisions.  A DNN knows its input
width but not its context: it comes from the decoder's decoding_model_params, else from the model's
add_metadata entry, else from the keyword arguments pre_context= / post_context=.

The stage in front of all three is `OnlinePreprocessor`: raw amplifier rows in pushes of ANY length -- 37 or 250
samples at 1 kHz for a 64 Hz model -- through a `preprocess.Preprocessor`'s filters, resample, re-reference, channel
selection and normalisation in ONE td_frontend_push launch per push for a bank of sessions, the filter state and the
resample phase on the device.  Its float32 device tensor goes into `OnlineDecoder.push` as it is:

    front = OnlinePreprocessor(prep)             # prep: the Preprocessor the model was trained behind
    for raw, env1, env2 in chunks:               # raw [n_raw, C] device tensor, any n_raw
      result = online.push(front.push(raw), env1, env2)

The envelopes come the same way: `OnlineAudioFeatures` takes the two speakers' audio (int16 as a sound card delivers
it, column k = speaker k) in pushes of any length and gives the intensity envelope of a `preprocess.AudioFeatures` at
the model's frame rate in ONE td_audio_online_push launch per push -- over any cut the frames of
compute_intensity(whole), which the batch call, whose window centres restart on every call, is not.  An envelope
frame needs half a window of future audio, so it trails the EEG frame of its index; `FrameJoin` lines the streams
up, on the device:

    eeg = front.push(raw)
    env = audio.push(pcm)                        # [S, m, 2] float32
    result = online.push(*join.push(eeg, env[..., 0], env[..., 1]))

The model itself can come from the chain: `OnlineRidgeFit` takes (eeg, target) rows in pushes of any length and
keeps the exact float64 moments of the lagged ridge regression in ONE td_fit_online_push launch per push;
`solve(lambdas)` gives ridge weights on the device and `OnlineDecoder.set_weights` takes them between pushes:

    fit.push(eeg, attended_envelope)             # during calibration, any chunk length
    w, b = fit.solve([0.1])
    online.set_weights(w[:, 0, :, 0], b[:, 0, 0])

and so can the statistics the new weights are scored with: `OnlineCalibration` takes a labelled stretch of (eeg,
attended envelope, unattended envelope) rows in pushes of any length -- ONE td_calib_online_push launch per push,
nothing stored per row -- and gives what infer_decoder.Decoder.train would: the correlation statistics, the scaled
LDA and d'; `OnlineDecoder.set_statistics` takes them between pushes:

    calib.push(eeg, attended_envelope, unattended_envelope)
    r = calib.finish()
    online.set_statistics(r.corr, r.lda)

A CCA bank trains the same way: `OnlineCCAFit` keeps the exact float64 moments of both lagged views in ONE
td_ccafit_online_push launch per push, `solve(lambdas, dims)` gives the reference's CCA model and the fitted stretch's
statistics on the device, and `OnlineDecoder.set_cca_model` takes them between pushes:

    cca_fit.push(eeg, attended_features)
    r = cca_fit.solve([1.0], dims=5)
    online.set_cca_model(r.mean_x, r.rot_x[:, 0], r.mean_y, r.rot_y[:, 0], corr=r.corr[:, 0])

and `OnlineCCACalibration` closes that chain as `OnlineCalibration` closes the linear one: a labelled stretch of (eeg,
attended features, unattended features) rows through the bank's current rotations in ONE td_ccacalib_online_push
launch per push gives the statistics of ONE correlator fed both classes and the scaled LDA over the dims columns --
one Cholesky solve, no eigenproblem --, and `OnlineDecoder.set_cca_statistics` takes them between pushes:

    cca_calib.push(eeg, attended_features, unattended_features)
    c = cca_calib.finish()
    online.set_cca_statistics(c.corr, c.lda)

A DNN bank cannot be fitted online, but it can be calibrated: `OnlineDNNCalibration` is `OnlineCalibration` with the
bank's network in front of the sums -- ONE td_fccalib_online_push launch per push, the prediction that of
td_fc_online_push bit for bit, the same state block and the same finish -- so a network trained offline on other
sessions is scored with the new listener's statistics and LDA:

    dnn_calib.push(eeg, attended_envelope, unattended_envelope)
    r = dnn_calib.finish()
    online.set_statistics(r.corr, r.lda)

Without a GPU (`device.gpu_available()` false) the same object runs a NumPy session with the same
semantics -- float64 throughout, window sums in frame order, td_online_plan's arithmetic -- so that the logic can
be built and tested anywhere.  (The state-space decoder has no host form: 'ssd' needs the GPU.)
"""
import collections

import numpy as np

from telluride_decoding_amd import _lib
from telluride_decoding_amd import attention_decoder
from telluride_decoding_amd import brain_model
from telluride_decoding_amd import device
from telluride_decoding_amd import infer_decoder

MAX_CHANNELS = device.ONLINE_MAX_CHANNELS
MAX_LAGS = device.ONLINE_MAX_LAGS
MAX_WINDOW = 65536                         # TD_ONLINE_MAX_WIDTH
DECODER_TYPES = ('wta', 'stepped', 'step', 'ssd')

OnlineResult = collections.namedtuple('OnlineResult', ['scores', 'decisions', 'first_window'])


def session_parameters(decoder, **context):
  """What one listener's session needs from its decoder, checked against the online path's limits.  A
  LinearRegressionDecoder gives dict(kind='linear', c, pre, post, w [lags c] float32, b float32, corr [2, 3]
  float64, lda [3] float64 or None, reduction); around a BrainModelDNN what dnn_session_parameters says; a
  CCADecoder what cca_session_parameters says (`context`: their keyword arguments)."""
  if isinstance(decoder, infer_decoder.CCADecoder):
    return cca_session_parameters(decoder, **context)
  if not isinstance(decoder, infer_decoder.LinearRegressionDecoder):
    raise ValueError('OnlineDecoder decodes with a LinearRegressionDecoder or a CCADecoder, not a %s.' %
                     type(decoder).__name__)
  model = decoder.decoding_model
  if isinstance(model, brain_model.BrainModelDNN):
    return dnn_session_parameters(decoder, **context)
  if context:
    raise TypeError('OnlineDecoder: %s is a CCA or DNN model\'s context; a linear model carries its own.' %
                    ', '.join(sorted(context)))
  if not isinstance(model, brain_model.BrainModelLinearRegression):
    raise ValueError('OnlineDecoder needs a BrainModelLinearRegression or a BrainModelDNN behind a '
                     'LinearRegressionDecoder, not a %s.' % type(model).__name__)
  if model.w_estimate is None:
    raise ValueError('OnlineDecoder needs a fitted model: BrainModelLinearRegression.fit first.')
  w = np.asarray(model.w_estimate, np.float32)
  w = w.reshape(w.shape[0], -1)
  if w.shape[1] != 1:
    raise ValueError('OnlineDecoder decodes one model output, not %d.' % w.shape[1])
  reduction = decoder._reduction
  if reduction not in device.ONLINE_REDUCTIONS:
    raise ValueError('OnlineDecoder reduces one output with %s, not with %r.' %
                     (', '.join(repr(r) for r in device.ONLINE_REDUCTIONS), reduction))
  c, pre, post = int(model._c1), int(model._pre), int(model._post)
  if not 1 <= c <= MAX_CHANNELS:
    raise ValueError('OnlineDecoder takes 1 to %d channels, not %d.' % (MAX_CHANNELS, c))
  if pre < 0 or post < 0 or pre + 1 + post > MAX_LAGS:
    raise ValueError('OnlineDecoder takes at most %d lags, not %d + 1 + %d.' % (MAX_LAGS, pre, post))
  if w.shape[0] != c * (pre + 1 + post):
    raise ValueError('The model has %d weights for %d channels x %d lags.' % (w.shape[0], c, pre + 1 + post))
  mean_x, mean_y, power = decoder._stat_vectors(1)
  stats = [float(mean_x[0]), float(mean_y[0]), float(power[0])]
  lda = None
  if reduction == 'lda':
    kw = decoder._reduce_kwargs()
    lda = np.array([float(np.reshape(kw['lda_w'], -1)[0]), float(kw['lda_slope']), float(kw['lda_intercept'])],
                   np.float64)
  return dict(kind='linear', c=c, pre=pre, post=post, w=w[:, 0].copy(), b=np.float32(np.reshape(model.b_estimate, -1)[0]),
              corr=np.array([stats, stats], np.float64), lda=lda, reduction=reduction)


CONTEXT_KEYS = ('pre_context', 'post_context', 'input2_pre_context', 'input2_post_context')


def cca_session_parameters(decoder, **context):
  """What one listener's session needs from a CCADecoder around a fitted cca.BrainModelCCA, checked against
  the limits of td_cca_online_push: dict(kind='cca', c, pre, post (the EEG view), c2, pre2, post2 (a speaker's
  feature block), dims, mean_x [k1], rot_x [k1, dims], mean_y [k2], rot_y [k2, dims] float32, corr [2, 3, dims]
  float64, lda [dims + 2] float64 or None, reduction).  The context is the decoder's decoding_model_params
  (pre_context, post_context, input2_pre_context, input2_post_context -- what infer.get_data_for_model builds
  its datasets from), else the model's add_metadata entry, else the keyword arguments of the same names."""
  model = decoder.decoding_model
  if model is None or not hasattr(model, 'rot_x') or not hasattr(model, '_input1_width'):
    raise ValueError('OnlineDecoder needs a cca.BrainModelCCA behind a CCADecoder, not a %s.' %
                     type(model).__name__)
  if model.rot_x is None:
    raise ValueError('OnlineDecoder needs a fitted CCA model: BrainModelCCA.fit first.')
  unknown = sorted(set(context) - set(CONTEXT_KEYS))
  if unknown:
    raise TypeError('OnlineDecoder: unknown context argument %s (the context is %s).' %
                    (', '.join(unknown), ', '.join(CONTEXT_KEYS)))
  carried = decoder.decoding_model_params or getattr(model, 'telluride_metadata', None) or {}
  if not isinstance(carried, dict) or not all(k in carried for k in CONTEXT_KEYS):
    carried = {k: context.get(k, 0) for k in CONTEXT_KEYS}
  if int(carried.get('input_offset', 0) or 0) != 0:
    raise ValueError('OnlineDecoder decodes with an input_offset of 0, not %s.' % (carried['input_offset'],))
  pre1, post1, pre2, post2 = (int(carried[k]) for k in CONTEXT_KEYS)
  rot_x, rot_y = np.asarray(model.rot_x, np.float32), np.asarray(model.rot_y, np.float32)
  mean_x, mean_y = np.asarray(model.mean_x, np.float32).reshape(-1), np.asarray(model.mean_y, np.float32).reshape(-1)
  k1, k2, dims = int(rot_x.shape[0]), int(rot_y.shape[0]), int(rot_x.shape[1])
  if min(pre1, post1, pre2, post2) < 0 or pre1 + 1 + post1 > MAX_LAGS or pre2 + 1 + post2 > MAX_LAGS:
    raise ValueError('OnlineDecoder takes at most %d lags in a view, not %d + 1 + %d and %d + 1 + %d.' %
                     (MAX_LAGS, pre1, post1, pre2, post2))
  if (k1 % (pre1 + 1 + post1) or k2 % (pre2 + 1 + post2) or rot_y.shape[1] != dims or mean_x.size != k1 or
      mean_y.size != k2):
    raise ValueError('The CCA model has rotations of %s and %s for contexts of %d + 1 + %d and %d + 1 + %d frames.' %
                     (rot_x.shape, rot_y.shape, pre1, post1, pre2, post2))
  c1, c2 = k1 // (pre1 + 1 + post1), k2 // (pre2 + 1 + post2)
  if not 1 <= c1 <= MAX_CHANNELS:
    raise ValueError('OnlineDecoder takes 1 to %d channels, not %d.' % (MAX_CHANNELS, c1))
  if not 1 <= c2 <= device.CCA_ONLINE_MAX_FEATURES:
    raise ValueError('OnlineDecoder takes 1 to %d features per speaker, not %d.' %
                     (device.CCA_ONLINE_MAX_FEATURES, c2))
  if not 1 <= dims <= device.CCA_ONLINE_MAX_DIMS:
    raise ValueError('OnlineDecoder takes 1 to %d dims, not %d.' % (device.CCA_ONLINE_MAX_DIMS, dims))
  reduction = decoder._reduction
  if reduction not in device.CCA_ONLINE_REDUCTIONS:
    raise ValueError('OnlineDecoder reduces the dims of a CCA model with %s, not with %r.' %
                     (', '.join(repr(r) for r in device.CCA_ONLINE_REDUCTIONS), reduction))
  if reduction == 'second' and dims < 2:
    raise ValueError('The reduction \'second\' needs at least 2 dims, not %d.' % dims)
  # (the rotations plus a pass of one frame must fit the workgroup's LDS: the library says so, with the budget)
  device.cca_online_lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, 1)
  mean_a, mean_b, power = decoder._stat_vectors(dims)
  stats = np.stack([mean_a, mean_b, power]).astype(np.float64)
  lda = None
  if reduction == 'lda':
    kw = decoder._reduce_kwargs()
    lda_w = np.asarray(kw['lda_w'], np.float64).reshape(-1)
    if lda_w.size != dims:
      raise ValueError('The LDA has %d weights for %d dims.' % (lda_w.size, dims))
    lda = np.concatenate([lda_w, [float(kw['lda_slope']), float(kw['lda_intercept'])]]).astype(np.float64)
  return dict(kind='cca', c=c1, pre=pre1, post=post1, c2=c2, pre2=pre2, post2=post2, dims=dims,
              mean_x=mean_x.copy(), rot_x=np.ascontiguousarray(rot_x), mean_y=mean_y.copy(),
              rot_y=np.ascontiguousarray(rot_y), corr=np.stack([stats, stats]), lda=lda, reduction=reduction)


DNN_CONTEXT_KEYS = ('pre_context', 'post_context')


def dnn_session_parameters(decoder, **context):
  """What one listener's session needs from a LinearRegressionDecoder around a brain_model.BrainModelDNN, checked
  against the limits of td_fc_online_push: dict(kind='dnn', c, pre, post, hidden (list), weights [W1, b1, W2, b2,
  ...] float32, params (the same, packed as td_mlp_* reads them), corr [2, 3] float64, lda [3] float64 or None,
  reduction).  A DNN model knows its input width, not its context: pre_context, post_context (and input_offset,
  which must be 0) come from the decoder's decoding_model_params, else from the model's add_metadata entry, else
  from the keyword arguments pre_context= / post_context=."""
  model = decoder.decoding_model
  unknown = sorted(set(context) - set(DNN_CONTEXT_KEYS))
  if unknown:
    raise TypeError('OnlineDecoder: unknown context argument %s (the context of a DNN model is %s).' %
                    (', '.join(unknown), ', '.join(DNN_CONTEXT_KEYS)))
  carried = decoder.decoding_model_params or getattr(model, 'telluride_metadata', None) or {}
  if not isinstance(carried, dict) or not all(k in carried for k in DNN_CONTEXT_KEYS):
    if not all(k in context for k in DNN_CONTEXT_KEYS):
      raise ValueError('A DNN model does not carry its context: give OnlineDecoder pre_context= and post_context= '
                       '(or a decoder whose decoding_model_params, or a model whose add_metadata entry, holds '
                       'them).')
    carried = {k: context[k] for k in DNN_CONTEXT_KEYS}
  if int(carried.get('input_offset', 0) or 0) != 0:
    raise ValueError('OnlineDecoder decodes with an input_offset of 0, not %s.' % (carried['input_offset'],))
  pre, post = (int(carried[k]) for k in DNN_CONTEXT_KEYS)
  if pre < 0 or post < 0 or pre + 1 + post > MAX_LAGS:
    raise ValueError('OnlineDecoder takes at most %d lags, not %d + 1 + %d.' % (MAX_LAGS, pre, post))
  weights = [np.asarray(w, np.float32) for w in model.get_weights()]
  hidden = [int(u) for u in model.num_hidden_list]
  k, outputs = int(weights[0].shape[0]), int(weights[-1].shape[0])
  if outputs != 1:
    raise ValueError('OnlineDecoder decodes one model output, not %d.' % outputs)
  if k % (pre + 1 + post):
    raise ValueError('The DNN model has %d inputs: no multiple of the %d + 1 + %d lags of its context.' %
                     (k, pre, post))
  c = k // (pre + 1 + post)
  if not 1 <= c <= MAX_CHANNELS:
    raise ValueError('OnlineDecoder takes 1 to %d channels, not %d.' % (MAX_CHANNELS, c))
  if k > device.DNN_ONLINE_MAX_INPUTS:
    raise ValueError('OnlineDecoder takes at most %d lagged inputs, not %d.' % (device.DNN_ONLINE_MAX_INPUTS, k))
  if len(hidden) > device.DNN_ONLINE_MAX_HIDDEN:
    raise ValueError('OnlineDecoder takes at most %d hidden layers, not %d.' %
                     (device.DNN_ONLINE_MAX_HIDDEN, len(hidden)))
  if any(not 1 <= u <= device.DNN_ONLINE_MAX_UNITS for u in hidden):
    raise ValueError('OnlineDecoder takes hidden layers of 1 to %d units, not %s.' %
                     (device.DNN_ONLINE_MAX_UNITS, hidden))
  reduction = decoder._reduction
  if reduction not in device.ONLINE_REDUCTIONS:
    raise ValueError('OnlineDecoder reduces one output with %s, not with %r.' %
                     (', '.join(repr(r) for r in device.ONLINE_REDUCTIONS), reduction))
  # (two chunks of W1, the small layers and a pass of one frame must fit the workgroup's LDS: the library says so)
  device.dnn_online_lds_bytes(c, pre, post, hidden, 1)
  mean_x, mean_y, power = decoder._stat_vectors(1)
  stats = [float(mean_x[0]), float(mean_y[0]), float(power[0])]
  lda = None
  if reduction == 'lda':
    kw = decoder._reduce_kwargs()
    lda = np.array([float(np.reshape(kw['lda_w'], -1)[0]), float(kw['lda_slope']), float(kw['lda_intercept'])],
                   np.float64)
  return dict(kind='dnn', c=c, pre=pre, post=post, hidden=hidden, weights=weights,
              params=np.concatenate([w.reshape(-1) for w in weights]).astype(np.float32),
              corr=np.array([stats, stats], np.float64), lda=lda, reduction=reduction)


def _cca_frame_score(a, b, stats, reduction, lda):
  """frame_scores_kernel over the dims columns, float64: a, b [frames, dims], stats [3, dims]."""
  v = (a - stats[0]) * (b - stats[1]) / stats[2]
  if reduction == 'first':
    return v[:, 0]
  if reduction == 'second':
    return v[:, 1]
  acc = np.zeros((v.shape[0],), np.float64)
  for c in range(v.shape[1]):                       # in column order
    if reduction == 'mean':
      acc = acc + v[:, c]
    elif reduction == 'mean-squared':
      acc = acc + np.where(v[:, c] > 0.0, v[:, c] * v[:, c], np.where(v[:, c] < 0.0, -v[:, c] * v[:, c], 0.0))
    else:
      acc = acc + v[:, c] * lda[c]
  if reduction == 'lda':
    return lda[-2] * acc + lda[-1]
  return acc / float(v.shape[1])


def _frame_score(truth, pred, stats, reduction, lda):
  v = (truth - stats[0]) * (pred - stats[1]) / stats[2]
  if reduction == 'first':
    return v
  if reduction == 'mean':
    return 0.0 + v
  if reduction == 'mean-squared':
    return 0.0 + np.where(v > 0.0, v * v, np.where(v < 0.0, -v * v, 0.0))
  return lda[1] * (v * lda[0]) + lda[2]


def _session_rows(tail, rows, post, flush, axis=0):
  """One stream of a NumPy session's push, its rows along `axis`: (what the push reads -- the old tail, the push and,
  on a flush, `post` zero rows, so that slot 0 is the tail's first row --, the next tail: the last len(tail) rows of
  old tail and push)."""
  both = np.concatenate([tail, rows], axis=axis)
  cut, pad = [slice(None)] * both.ndim, list(both.shape)
  cut[axis], pad[axis] = slice(both.shape[axis] - tail.shape[axis], None), post
  return np.concatenate([both, np.zeros(pad, both.dtype)], axis=axis) if flush else both, both[tuple(cut)]


def _session_frames(frames_before, n, post, flush):
  """(the first frame a push of n rows behind frames_before emits, how many, the slot of the first one's first row in
  what _session_rows reads) for frames that run `post` rows behind the input."""
  pl = device.online_plan(frames_before, n, post, 1, 1, flush)
  return pl.emitted_before, pl.emitted_after - pl.emitted_before, pl.emitted_before - (frames_before - post)


class _HostSession(object):
  """One listener's session in NumPy float64: the semantics of td_online_push, for machines without a GPU."""

  def __init__(self, params, width, hop, decoder):
    self.p, self.width, self.hop, self.decoder = params, width, hop, decoder
    self.reset()

  def reset(self):
    p = self.p
    self.tail = np.zeros((p['pre'] + p['post'], p['c']), np.float64)
    self.env_tail = np.zeros((p['post'], 2), np.float64)
    self.recent = np.zeros((0, 2), np.float64)      # the last `width` per-frame scores, oldest first
    self.step = 0.5

  def push(self, eeg, env, frames_before, flush):
    p = self.p
    c, pre, post = p['c'], p['pre'], p['post']
    n = eeg.shape[0]
    pl = device.online_plan(frames_before, n, post, self.width, self.hop, flush)
    rows, tail = _session_rows(self.tail, eeg, post, flush)
    envs, env_tail = _session_rows(self.env_tail, env, post, False)
    emitted = pl.emitted_after - pl.emitted_before
    # frame emitted_before + i reads rows[i0 + i : i0 + i + lags] and envs[i0 + i]: rows[0] is the EEG row
    # frames_before - pre - post, envs[0] the envelope row frames_before - post
    i0 = pl.emitted_before - (frames_before - post)
    w = p['w'].astype(np.float64)
    pred = np.zeros((emitted,), np.float64)
    for l in range(pre + 1 + post):                 # (lag, channel) order, whatever the push's length
      for ch in range(c):
        pred += rows[i0 + l:i0 + l + emitted, ch] * w[l * c + ch]
    pred = pred + float(p['b'])
    truth = envs[i0:i0 + emitted]
    frame = np.stack([_frame_score(truth[:, k], pred, p['corr'][k], p['reduction'], p['lda'])
                      for k in (0, 1)], axis=1).reshape(emitted, 2)
    scores, decisions = self._windows(frame, pl)
    self.tail, self.env_tail = tail, env_tail
    return scores, decisions, pred, frame, pl

  def _windows(self, frame, pl):
    """The windows a push completes from its per-frame scores [emitted, 2]: (scores, decisions)."""
    history = np.concatenate([self.recent, frame])   # frames [emitted_after - len(history), emitted_after)
    base = pl.emitted_after - history.shape[0]
    starts = (pl.first_window + np.arange(pl.new_windows)) * self.hop - base
    sums = np.zeros((pl.new_windows, 2), np.float64)
    for r in range(self.width):                      # in frame order
      sums += history[starts + r]
    scores = sums / float(self.width)
    decisions = np.zeros((pl.new_windows,), np.uint8)
    for i in range(pl.new_windows):
      if self.decoder == 'wta':
        decisions[i] = scores[i, 0] > scores[i, 1]
      elif self.decoder in ('stepped', 'step'):
        if scores[i, 0] > scores[i, 1]:
          self.step = min(0.9, self.step + 0.1)
        else:
          self.step = max(0.1, self.step - 0.1)
        decisions[i] = self.step > 0.5
    self.recent = history[max(0, history.shape[0] - self.width):]
    return scores, decisions


class _HostCcaSession(_HostSession):
  """One listener's CCA session in NumPy float64: the semantics of td_cca_online_push."""

  def reset(self):
    p = self.p
    self.delay = max(p['post'], p['post2'])
    self.tail = np.zeros((p['pre'] + self.delay, p['c']), np.float64)
    self.feat_tail = np.zeros((2, p['pre2'] + self.delay, p['c2']), np.float64)
    self.recent = np.zeros((0, 2), np.float64)
    self.step = 0.5

  @staticmethod
  def _project(rows, first, emitted, c, lags, mean, rot):
    """(x~ - mean) @ rot for the frames whose lagged rows start at rows[first + i], summed in (lag, channel)
    order whatever the push's length."""
    out = np.zeros((emitted, rot.shape[1]), np.float64)
    for l in range(lags):
      for ch in range(c):
        k = l * c + ch
        out += (rows[first + l:first + l + emitted, ch] - mean[k])[:, None] * rot[k][None, :]
    return out

  def push(self, eeg, feat, frames_before, flush):
    """eeg [n, c1], feat [2, n, c2]."""
    p = self.p
    c1, pre1, post1, c2, pre2, post2 = p['c'], p['pre'], p['post'], p['c2'], p['pre2'], p['post2']
    post = self.delay
    n = eeg.shape[0]
    pl = device.online_plan(frames_before, n, post, self.width, self.hop, flush)
    rows, tail = _session_rows(self.tail, eeg, post, flush)
    frows, feat_tail = _session_rows(self.feat_tail, feat, post, flush, axis=1)
    emitted = pl.emitted_after - pl.emitted_before
    # rows[0] is the EEG row frames_before - pre1 - post, frows[:, 0] the feature row frames_before - pre2 -
    # post: frame emitted_before + i reads rows[i0 + i : i0 + i + lags1] and frows[:, i0 + i : i0 + i + lags2]
    i0 = pl.emitted_before - (frames_before - post)
    mean_x, rot_x = p['mean_x'].astype(np.float64), p['rot_x'].astype(np.float64)
    mean_y, rot_y = p['mean_y'].astype(np.float64), p['rot_y'].astype(np.float64)
    a = self._project(rows, i0, emitted, c1, pre1 + 1 + post1, mean_x, rot_x)
    bs = [self._project(frows[k], i0, emitted, c2, pre2 + 1 + post2, mean_y, rot_y) for k in (0, 1)]
    frame = np.stack([_cca_frame_score(a, bs[k], p['corr'][k], p['reduction'], p['lda']) for k in (0, 1)],
                     axis=1).reshape(emitted, 2)
    scores, decisions = self._windows(frame, pl)
    self.tail, self.feat_tail = tail, feat_tail
    return scores, decisions, np.concatenate([a] + bs, axis=1), frame, pl


class _HostDnnSession(_HostSession):
  """One listener's DNN session in NumPy float64: the semantics of td_fc_online_push.  Only the prediction differs
  from _HostSession's: Dense layers on the frame's lagged rows, every sum in input order, ReLU between them."""

  def _predict(self, rows, first, emitted):
    p = self.p
    c, lags = p['c'], p['pre'] + 1 + p['post']
    ws = [w.astype(np.float64) for w in p['weights']]
    act = np.zeros((emitted, ws[0].shape[1]), np.float64)
    for l in range(lags):                            # (lag, channel) order, whatever the push's length
      for ch in range(c):
        act += rows[first + l:first + l + emitted, ch][:, None] * ws[0][l * c + ch][None, :]
    act = act + ws[1]
    for layer in range(1, len(ws) // 2):
      act = np.where(act <= 0.0, 0.0, act)
      w, b = ws[2 * layer], ws[2 * layer + 1]
      out = np.zeros((emitted, w.shape[1]), np.float64)
      for i in range(w.shape[0]):                    # in input order
        out += act[:, i][:, None] * w[i][None, :]
      act = out + b
    return act[:, 0]

  def push(self, eeg, env, frames_before, flush):
    p = self.p
    c, pre, post = p['c'], p['pre'], p['post']
    n = eeg.shape[0]
    pl = device.online_plan(frames_before, n, post, self.width, self.hop, flush)
    rows, tail = _session_rows(self.tail, eeg, post, flush)
    envs, env_tail = _session_rows(self.env_tail, env, post, False)
    emitted = pl.emitted_after - pl.emitted_before
    i0 = pl.emitted_before - (frames_before - post)   # (as _HostSession.push)
    pred = self._predict(rows, i0, emitted)
    truth = envs[i0:i0 + emitted]
    frame = np.stack([_frame_score(truth[:, k], pred, p['corr'][k], p['reduction'], p['lda'])
                      for k in (0, 1)], axis=1).reshape(emitted, 2)
    scores, decisions = self._windows(frame, pl)
    self.tail, self.env_tail = tail, env_tail
    return scores, decisions, pred, frame, pl


class _Bank(object):
  """What the seven online banks share: S sessions that run on the device (`_dev`: a dict with the handle 'h' and the
  zeroed uint8 'state' [S, bytes]) or as NumPy sessions (`_host`: a list of S objects with reset()), and refuse pushes
  once flushed.  A class gives FLUSHED, its sentence for that refusal."""
  FLUSHED = None

  def __init__(self, sessions, on_device):
    self.sessions, self._on_device = sessions, on_device
    self._dev = self._host = None
    self.flushed = False

  def _zero_state(self, h, nbytes):
    """A bank of fresh sessions: [S, nbytes] uint8 zeros on the handle's device."""
    torch = device._torch()
    return torch.zeros((self.sessions, nbytes), dtype=torch.uint8, device=h.device)

  def reset(self):
    """Zero state, not flushed (the class's own counters are its own reset's)."""
    self.flushed = False
    if self._dev is not None:
      self._dev['state'].zero_()
    if self._host is not None:
      for sess in self._host:
        sess.reset()

  def _refuse_flushed(self):
    if self.flushed:
      raise ValueError(self.FLUSHED)

  def _no_rows(self, width, dtype=np.float32):
    """What the NumPy sessions take for a flush without rows."""
    return np.zeros((self.sessions, 0, width), dtype)

  @staticmethod
  def _last_rows(sentence, *arrays):
    """Whether a flush carries last rows: all of `arrays` or none of them, else `sentence`."""
    given = [a is not None for a in arrays]
    if any(given) and not all(given):
      raise ValueError(sentence)
    return given[0]

  @staticmethod
  def _upload(h, a):
    """A host array [..., k] as a float32 device tensor of its shape (Handle.to_device takes two dimensions)."""
    return h.to_device(a.reshape(-1, a.shape[-1])).reshape(a.shape)


class OnlineDecoder(_Bank):
  """A bank of online decoding sessions, one per listener.

  decoders: one infer_decoder.LinearRegressionDecoder around a fitted BrainModelLinearRegression, or a list
  of S of them -- one listener each, with its own weights and trained statistics (the channel count and the
  context are the bank's: every decoder has the same).  The reduction, the correlation parameters and the
  LDA come from each decoder; both speakers are scored with the decoder's one set of statistics, as
  infer.run_reduction_test does.  window_step defaults to window_size // 2.  decoder_type: 'wta',
  'stepped' or 'ssd' (two launches per push: the windows, then td_decode_ssd_stream on them, device to
  device).

  Or one infer_decoder.CCADecoder around a fitted cca.BrainModelCCA, or a list of S of them (a bank is all
  linear or all CCA, with the same shapes, dims and reduction throughout): the push is then
  push(eeg, feat1, feat2) with one block of audio features [n, c2] / [S, n, c2] per speaker, the EEG view is
  projected once per frame and each speaker's view against the same rotations (td_cca_online_push), and the
  dims columns are scored and reduced as Decoder.infer_one does.  The context of the two views comes from the
  decoder's decoding_model_params (pre_context, post_context, input2_pre_context, input2_post_context), or
  from keyword arguments of those names when the model carries none; results run max(post_context,
  input2_post_context) frames behind the input.

  Or one LinearRegressionDecoder around a brain_model.BrainModelDNN with one output, or a list of S of them (a
  bank is all of one kind; a DNN bank shares channels, context, hidden layers and reduction): the push is the
  linear bank's push(eeg, env1, env2) and ONE td_fc_online_push launch, the prediction that of
  device.mlp_forward on the whole recording bit for bit.  The context comes from the decoder's
  decoding_model_params, the model's add_metadata entry, or the keyword arguments pre_context= / post_context=;
  sessions around bitwise-equal parameters read one copy of them.
  """
  FLUSHED = 'The session was flushed: reset() starts the next recording.'

  def __init__(self, decoders, window_size, window_step=None, decoder_type='wta', frame_rate=100.0,
               ssd_offset=0.0, **context):
    if isinstance(decoders, infer_decoder.Decoder) or not isinstance(decoders, (list, tuple)):
      decoders = [decoders]
    if not decoders:
      raise ValueError('OnlineDecoder needs at least one decoder.')
    self._params = [session_parameters(d, **context) for d in decoders]
    first = self._params[0]
    self.kind = first['kind']
    shape_keys = ('c', 'pre', 'post', 'c2', 'pre2', 'post2', 'dims', 'reduction')
    for p in self._params[1:]:
      if p['kind'] != self.kind:
        raise ValueError('A bank is all linear or all CCA or all DNN, not a %s decoder beside a %s one.' %
                         (p['kind'], self.kind))
      if self.kind == 'dnn' and p['hidden'] != first['hidden']:
        raise ValueError('Every DNN decoder of a bank has the same hidden layers: %s and %s.' %
                         (first['hidden'], p['hidden']))
      if self.kind == 'cca' and any(p[k] != first[k] for k in shape_keys):
        raise ValueError('Every CCA decoder of a bank has the same channels, features, contexts, dims and '
                         'reduction: %s and %s.' % (tuple(first[k] for k in shape_keys),
                                                    tuple(p[k] for k in shape_keys)))
      if (p['c'], p['pre'], p['post'], p['reduction']) != (first['c'], first['pre'], first['post'],
                                                           first['reduction']):
        raise ValueError('Every decoder of a bank has the same channels, context and reduction: %s and %s.' %
                         ((first['c'], first['pre'], first['post'], first['reduction']),
                          (p['c'], p['pre'], p['post'], p['reduction'])))
    window_size = int(window_size)
    if not 1 <= window_size <= MAX_WINDOW:
      raise ValueError('OnlineDecoder takes windows of 1 to %d frames, not %d.' % (MAX_WINDOW, window_size))
    window_step = window_size // 2 if window_step is None else int(window_step)
    if window_step < 1:
      raise ValueError('Window size %d gives a window step of %d.' % (window_size, window_step))
    if decoder_type not in DECODER_TYPES:
      raise ValueError('Unknown type (%s) requested from OnlineDecoder' % decoder_type)
    self.channels, self.pre, self.post = first['c'], first['pre'], first['post']
    self.reduction = first['reduction']
    self.delay = self.post                      # frames the results run behind the input
    if self.kind == 'dnn':
      self.hidden = list(first['hidden'])
    if self.kind == 'cca':
      self.features, self.pre2, self.post2, self.dims = first['c2'], first['pre2'], first['post2'], first['dims']
      self.delay = max(self.post, self.post2)
    self.window_size, self.window_step = window_size, window_step
    self.decoder_type = 'stepped' if decoder_type == 'step' else decoder_type
    self._ssd = None
    if self.decoder_type == 'ssd':
      self._ssd = attention_decoder.create_attention_decoder('ssd', window_step=window_step,
                                                             frame_rate=frame_rate, ssd_offset=ssd_offset)
    _Bank.__init__(self, len(self._params), device.gpu_available())
    if self._ssd is not None and not self._on_device:
      raise _lib.HotPathUnavailable('The state-space decoder has no host form: \'ssd\' needs the GPU.')
    self.reset()

  @classmethod
  def from_model_dir(cls, model_dir, reduction, window_size, **kwargs):
    """The session of a saved model directory (infer.load_model: the decoding model and the decoder's
    correlation and LDA parameters)."""
    from telluride_decoding_amd import infer
    return cls(infer.load_model(model_dir, reduction), window_size, **kwargs)

  # -- state -------------------------------------------------------------------------------------
  def _device_setup(self):
    h = device.default_handle()
    ps = self._params
    dev = dict(h=h)
    # the model: sessions around ONE model (bitwise-equal parameters for a DNN) read one copy of it
    names = {'cca': ('mean_x', 'rot_x', 'mean_y', 'rot_y'), 'dnn': ('params',)}.get(self.kind, ('w', 'b'))
    bits = lambda a: a.view(np.uint32) if self.kind == 'dnn' else a
    shared = all(np.array_equal(bits(p[k]), bits(ps[0][k])) for p in ps[1:] for k in names)
    models = ps[:1] if shared else ps
    if self.kind == 'cca':
      for k in names:
        dev[k] = self._upload(h, np.stack([p[k] for p in models]))
    elif self.kind == 'dnn':
      # (a row starts on a 16-byte boundary)
      count = int(ps[0]['params'].size)
      packed = np.zeros((len(models), -(-count // 4) * 4), np.float32)
      for i, p in enumerate(models):
        packed[i, :count] = p['params']
      dev['params'] = h.to_device(packed)[:, :count]
    else:
      dev['w'] = h.to_device(np.stack([p['w'] for p in models]))
      dev['b'] = h.to_device(np.array([[p['b']] for p in models], np.float32)).reshape(-1)
    # the statistics [S, 2, 3] (a CCA bank's [S, 2, 3, dims]), the LDA, the state
    corr = np.stack([p['corr'] for p in ps])
    dev['corr'] = h.to_device(corr.reshape(self.sessions, -1), np.float64).reshape(corr.shape)
    dev['lda'] = (h.to_device(np.stack([p['lda'] for p in ps]), np.float64)
                  if self.reduction == 'lda' else None)
    if self.kind == 'cca':
      nbytes = device.cca_online_state_bytes(self.channels, self.pre, self.post, self.features, self.pre2,
                                             self.post2, self.window_size)
    else:
      nbytes = device.online_state_bytes(self.channels, self.pre, self.post, self.window_size)
    dev['state'] = self._zero_state(h, nbytes)
    dev['ssd_state'] = device.ssd_state(self.sessions, handle=h) if self._ssd is not None else None
    return dev

  def reset(self):
    """A fresh recording: zero state, no frame pushed.  (Its own, not _Bank's: the device bank is set up here at the
    first call, the state-space decoder's state is zeroed too, and the NumPy sessions are rebuilt from the
    parameters set_weights and set_statistics may have replaced.)"""
    self.frames_pushed = 0
    self.flushed = False
    if self._on_device:
      if self._dev is None:
        self._dev = self._device_setup()
      else:
        self._dev['state'].zero_()
        if self._dev['ssd_state'] is not None:
          self._dev['ssd_state'].zero_()
    else:
      kind = self.decoder_type
      session = {'cca': _HostCcaSession, 'dnn': _HostDnnSession}.get(self.kind, _HostSession)
      self._host = [session(p, self.window_size, self.window_step, kind) for p in self._params]

  def tune(self, r1, r2):
    """For 'ssd': the state-space decoder's prior tuning on an initial attended / unattended stretch of
    window scores (StateSpaceAttentionDecoder.tune_log_normal_priors), for every session of the bank."""
    if self._ssd is None:
      raise ValueError('tune is the state-space decoder\'s: this session decodes with %r.' % self.decoder_type)
    self._ssd.tune(r1, r2)
    state = self._dev['ssd_state']
    if self.frames_pushed:
      # sessions that have seen windows: the running rho_d / mu_d sit behind the state's 8 arrays
      torch = device._torch()
      (rho_a, rho_u), (mu_a, mu_u) = self._ssd._prior
      base = int(state.shape[1]) - 8
      state[:, base + 1:base + 5] = torch.tensor([rho_a, rho_u, mu_a, mu_u], dtype=torch.float64,
                                                 device=state.device)

  def set_weights(self, w, b):
    """Replaces the weights of a LINEAR bank in place, between pushes: w [K] (every session takes it) or [S, K],
    b a scalar or [S], K = lags x channels in (lag, channel) order -- device tensors (copied device to device, no
    host copy: what OnlineRidgeFit.solve returns, sliced) or arrays.  A bank that shared one model copy holds S
    copies afterwards when S rows are given.  The session state, the score ring and the correlation statistics are
    untouched: the next push predicts with the new weights and scores them with the decoder's TRAINED statistics.
    Re-estimating those statistics, or the LDA, online was out of scope here and is OnlineCalibration's work: a
    decoder whose predictions change scale pushes a labelled stretch through it and takes the result with
    set_statistics, without a batch run."""
    if self.kind != 'linear':
      raise ValueError('OnlineDecoder.set_weights replaces the weights of a linear bank only, not of a %s bank.' %
                       self.kind)
    s, k = self.sessions, (self.pre + 1 + self.post) * self.channels
    w_shape, b_shape = tuple(w.shape), tuple(np.shape(b)) if not hasattr(b, 'is_cuda') else tuple(b.shape)
    rows = s if len(w_shape) == 2 else 1
    if w_shape not in ((k,), (s, k)) or b_shape not in (((), (1,)) if rows == 1 else ((s,),)):
      raise ValueError('OnlineDecoder.set_weights takes w [%d] with a scalar b, or w [%d, %d] with b [%d], not w %s '
                       'with b %s.' % (k, s, k, s, w_shape, b_shape))
    if not self._on_device:
      w = np.asarray(w.cpu() if hasattr(w, 'cpu') else w, np.float32).reshape(rows, k)
      b = np.asarray(b.cpu() if hasattr(b, 'cpu') else b, np.float32).reshape(rows)
      for i, p in enumerate(self._params):
        p['w'], p['b'] = w[i % rows].copy(), np.float32(b[i % rows])
      return
    # (the device bank is the truth from here on: self._params keeps what the bank was built from)
    d = self._dev
    torch = device._torch()
    conv = lambda a, shape: (a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a, np.float32))).to(
        device=d['h'].device, dtype=torch.float32).reshape(shape)
    w, b = conv(w, (rows, k)), conv(b, (rows,))
    if rows > int(d['w'].shape[0]):              # one shared copy becomes S copies
      d['w'], d['b'] = w.clone().contiguous(), b.clone().contiguous()
    else:
      d['w'].copy_(w.expand_as(d['w']))
      d['b'].copy_(b.expand_as(d['b']))

  def set_statistics(self, corr, lda=None):
    """Replaces the correlation statistics -- and, for reduction 'lda', the LDA -- of a linear or DNN bank in place,
    between pushes: corr {mean_truth, mean_pred, power} as [3] (every session and both speakers take it), [S, 3]
    (both speakers of a session) or [S, 2, 3]; lda {lda_w, slope, intercept} as [3] or [S, 3], required when the
    bank's reduction is 'lda' and not read otherwise -- device tensors (copied device to device, no host copy: what
    OnlineCalibration.finish returns) or arrays.  The weights, the session state, the score ring and the stepped /
    state-space decoder's state are untouched: the frames the next push emits are scored with the new parameters,
    so the first window that lies wholly behind the swap is that of a bank built with them."""
    if self.kind not in ('linear', 'dnn'):
      raise ValueError('OnlineDecoder.set_statistics replaces the statistics of a linear or DNN bank, not of a %s '
                       'bank (its statistics have one column per dim).' % self.kind)
    s = self.sessions
    shape_of = lambda a: tuple(a.shape) if hasattr(a, 'shape') else tuple(np.shape(a))
    if shape_of(corr) not in ((3,), (s, 3), (s, 2, 3)):
      raise ValueError('OnlineDecoder.set_statistics takes corr [3], [%d, 3] or [%d, 2, 3], not %s.' %
                       (s, s, shape_of(corr)))
    if lda is not None and shape_of(lda) not in ((3,), (s, 3)):
      raise ValueError('OnlineDecoder.set_statistics takes lda [3] or [%d, 3], not %s.' % (s, shape_of(lda)))
    if self.reduction == 'lda' and lda is None:
      raise ValueError('OnlineDecoder.set_statistics: a bank that reduces with \'lda\' needs lda '
                       '{lda_w, slope, intercept} beside corr.')
    if not self._on_device:
      host = lambda a: np.asarray(a.cpu() if hasattr(a, 'cpu') else a, np.float64)
      corr = host(corr)
      corr = np.broadcast_to(corr if corr.ndim == 3 else (corr[:, None, :] if corr.ndim == 2 else corr), (s, 2, 3))
      for i, p in enumerate(self._params):
        p['corr'] = corr[i].copy()
        if self.reduction == 'lda':
          p['lda'] = np.broadcast_to(host(lda), (s, 3))[i].copy()
      return
    # (the device bank is the truth from here on: self._params keeps what the bank was built from)
    d = self._dev
    torch = device._torch()
    conv = lambda a: (a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a, np.float64))).to(
        device=d['h'].device, dtype=torch.float64)
    corr = conv(corr)
    d['corr'].copy_((corr.unsqueeze(1) if corr.dim() == 2 else corr).expand_as(d['corr']))
    if self.reduction == 'lda':
      d['lda'].copy_(conv(lda).expand_as(d['lda']))

  def set_cca_model(self, mean_x, rot_x, mean_y, rot_y, corr=None, lda=None):
    """Replaces the model of a CCA bank in place, between pushes: mean_x [k1], rot_x [k1, dims], mean_y [k2], rot_y
    [k2, dims] (every session takes them) or with a leading [S] each; corr {mean_a, mean_b, power} as [3, dims]
    (every session and both speakers), [S, 3, dims] (both speakers of a session) or [S, 2, 3, dims], kept as it is
    when None; lda {weights, slope, intercept} as [dims + 2] or [S, dims + 2] -- a bank that reduces with 'lda' keeps
    its LDA unless one is given, the other reductions do not read it.  dims is the bank's.  Device tensors (copied
    device to device, no host copy: what OnlineCCAFit.solve returns, sliced) or arrays.  A bank that shared one model
    copy holds S copies afterwards when S models are given.  The session state, the score ring, the tails and the
    stepped / state-space decoder's state are untouched: the frames the next push emits are projected and scored
    with the new parameters, so the first window that lies wholly behind the swap is that of a bank built with
    them."""
    if self.kind != 'cca':
      raise ValueError('OnlineDecoder.set_cca_model replaces the model of a CCA bank only, not of a %s bank.' %
                       self.kind)
    s, dims = self.sessions, self.dims
    k1 = (self.pre + 1 + self.post) * self.channels
    k2 = (self.pre2 + 1 + self.post2) * self.features
    shape_of = lambda a: tuple(a.shape) if hasattr(a, 'shape') else tuple(np.shape(a))
    shapes = tuple(shape_of(a) for a in (mean_x, rot_x, mean_y, rot_y))
    one, many = ((k1,), (k1, dims), (k2,), (k2, dims)), ((s, k1), (s, k1, dims), (s, k2), (s, k2, dims))
    if shapes not in (one, many):
      raise ValueError('OnlineDecoder.set_cca_model takes mean_x %s, rot_x %s, mean_y %s and rot_y %s, or each with a '
                       'leading [%d], not %s.' % (one + (s, shapes)))
    rows = s if shapes == many else 1
    if corr is not None and shape_of(corr) not in ((3, dims), (s, 3, dims), (s, 2, 3, dims)):
      raise ValueError('OnlineDecoder.set_cca_model takes corr [3, %d], [%d, 3, %d] or [%d, 2, 3, %d], not %s.' %
                       (dims, s, dims, s, dims, shape_of(corr)))
    if lda is not None and shape_of(lda) not in ((dims + 2,), (s, dims + 2)):
      raise ValueError('OnlineDecoder.set_cca_model takes lda [%d] or [%d, %d], not %s.' %
                       (dims + 2, s, dims + 2, shape_of(lda)))
    names = ('mean_x', 'rot_x', 'mean_y', 'rot_y')
    model = dict(zip(names, (mean_x, rot_x, mean_y, rot_y)))
    if not self._on_device:
      host = lambda a, dtype: np.asarray(a.cpu() if hasattr(a, 'cpu') else a, dtype)
      for name, shape in zip(names, one):
        a = host(model[name], np.float32).reshape((rows,) + shape)
        for i, p in enumerate(self._params):
          p[name] = np.ascontiguousarray(a[i % rows])
      if corr is not None:
        corr = host(corr, np.float64)
        corr = np.broadcast_to(corr[:, None] if corr.ndim == 3 else corr, (s, 2, 3, dims))
        for i, p in enumerate(self._params):
          p['corr'] = corr[i].copy()
      if lda is not None and self.reduction == 'lda':
        for i, p in enumerate(self._params):
          p['lda'] = np.broadcast_to(host(lda, np.float64), (s, dims + 2))[i].copy()
      return
    # (the device bank is the truth from here on: self._params keeps what the bank was built from)
    d = self._dev
    torch = device._torch()
    conv = lambda a, dtype, np_dtype: (a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a, np_dtype))).to(
        device=d['h'].device, dtype=dtype)
    for name, shape in zip(names, one):
      a = conv(model[name], torch.float32, np.float32).reshape((rows,) + shape)
      if rows > int(d[name].shape[0]):            # one shared copy becomes S copies
        d[name] = a.clone().contiguous()
      else:
        d[name].copy_(a.expand_as(d[name]))
    if corr is not None:
      corr = conv(corr, torch.float64, np.float64)
      d['corr'].copy_((corr.unsqueeze(1) if corr.dim() == 3 else corr).expand_as(d['corr']))
    if lda is not None and self.reduction == 'lda':
      d['lda'].copy_(conv(lda, torch.float64, np.float64).expand_as(d['lda']))

  def set_cca_statistics(self, corr, lda=None):
    """Replaces the correlation statistics -- and, for reduction 'lda', the LDA -- of a CCA bank in place, between
    pushes: corr {mean_a, mean_b, power} as [3, dims] (every session and both speakers take it), [S, 3, dims] (both
    speakers of a session) or [S, 2, 3, dims]; lda {weights, slope, intercept} as [dims + 2] or [S, dims + 2], required
    when the bank's reduction is 'lda' and not read otherwise -- device tensors (copied device to device, no host
    copy: what OnlineCCACalibration.finish returns) or arrays.  The rotations, the session state, the score ring, the
    tails and the stepped / state-space decoder's state are untouched: the frames the next push emits are scored with
    the new parameters, so the first window that lies wholly behind the swap is that of a bank built with them."""
    if self.kind != 'cca':
      raise ValueError('OnlineDecoder.set_cca_statistics replaces the statistics of a CCA bank only, not of a %s '
                       'bank (set_statistics is that bank\'s).' % self.kind)
    s, dims = self.sessions, self.dims
    shape_of = lambda a: tuple(a.shape) if hasattr(a, 'shape') else tuple(np.shape(a))
    if shape_of(corr) not in ((3, dims), (s, 3, dims), (s, 2, 3, dims)):
      raise ValueError('OnlineDecoder.set_cca_statistics takes corr [3, %d], [%d, 3, %d] or [%d, 2, 3, %d], not %s.' %
                       (dims, s, dims, s, dims, shape_of(corr)))
    if lda is not None and shape_of(lda) not in ((dims + 2,), (s, dims + 2)):
      raise ValueError('OnlineDecoder.set_cca_statistics takes lda [%d] or [%d, %d], not %s.' %
                       (dims + 2, s, dims + 2, shape_of(lda)))
    if self.reduction == 'lda' and lda is None:
      raise ValueError('OnlineDecoder.set_cca_statistics: a bank that reduces with \'lda\' needs lda '
                       '{weights, slope, intercept} beside corr.')
    if not self._on_device:
      host = lambda a: np.asarray(a.cpu() if hasattr(a, 'cpu') else a, np.float64)
      corr = host(corr)
      corr = np.broadcast_to(corr[:, None] if corr.ndim == 3 else corr, (s, 2, 3, dims))
      for i, p in enumerate(self._params):
        p['corr'] = corr[i].copy()
        if self.reduction == 'lda':
          p['lda'] = np.broadcast_to(host(lda), (s, dims + 2))[i].copy()
      return
    # (the device bank is the truth from here on: self._params keeps what the bank was built from)
    d = self._dev
    torch = device._torch()
    conv = lambda a: (a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a, np.float64))).to(
        device=d['h'].device, dtype=torch.float64)
    corr = conv(corr)
    d['corr'].copy_((corr.unsqueeze(1) if corr.dim() == 3 else corr).expand_as(d['corr']))
    if self.reduction == 'lda':
      d['lda'].copy_(conv(lda).expand_as(d['lda']))

  # -- pushes ------------------------------------------------------------------------------------
  def _rows(self, *arrays):
    """Each of `arrays` -- host arrays or device tensors, [n, k] or [S, n, k] -- as float32 on the bank's side: device
    tensors when one of them is a tensor and the bank runs on the device, host arrays otherwise (the push uploads
    them)."""
    if self._on_device and any(hasattr(a, 'is_cuda') for a in arrays):
      torch = device._torch()
      where = self._dev['h'].device
      return [(a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a))).to(device=where, dtype=torch.float32)
              for a in arrays]
    return [np.asarray(a.cpu() if hasattr(a, 'cpu') else a, np.float32) for a in arrays]

  def _as_bank(self, eeg, env1, env2):
    """(eeg [S, n, C], env [S, n, 2]) as float32 host arrays or device tensors."""
    s, c = self.sessions, self.channels
    eeg, env1, env2 = self._rows(eeg, env1, env2)
    if eeg.ndim == 2:
      eeg = eeg[None]
    tensors = hasattr(eeg, 'is_cuda')
    stack = device._torch().stack if tensors else np.stack
    env = stack([env1.reshape(eeg.shape[0], -1), env2.reshape(eeg.shape[0], -1)], 2)
    if tensors:
      eeg = eeg.contiguous()
    if eeg.ndim != 3 or tuple(eeg.shape[0:3:2]) != (s, c) or tuple(env.shape) != (s, eeg.shape[1], 2):
      raise ValueError('A push is eeg [%d, n, %d] (or [n, %d] for one session) with two envelopes of n frames '
                       'each, not eeg %s with envelopes %s.' % (s, c, c, tuple(eeg.shape), tuple(env.shape[:2])))
    return eeg, env

  def _as_cca_bank(self, eeg, feat1, feat2):
    """(eeg [S, n, C], (feat1, feat2) [S, n, c2] each) as float32 host arrays or device tensors."""
    s, c, c2 = self.sessions, self.channels, self.features
    eeg, feat1, feat2 = (a[None] if a.ndim == 2 else a for a in self._rows(eeg, feat1, feat2))
    n = eeg.shape[1] if eeg.ndim == 3 else -1
    if (eeg.ndim != 3 or tuple(eeg.shape) != (s, n, c) or tuple(feat1.shape) != (s, n, c2) or
        tuple(feat2.shape) != (s, n, c2)):
      raise ValueError('A push is eeg [%d, n, %d] (or [n, %d] for one session) with two feature blocks [%d, n, %d] '
                       '(or [n, %d]), not eeg %s with features %s and %s.' %
                       (s, c, c, s, c2, c2, tuple(eeg.shape), tuple(feat1.shape), tuple(feat2.shape)))
    return eeg, (feat1, feat2)

  def push(self, eeg, env1, env2):
    """The next n frames of every session: eeg [n, C] / [S, n, C], env1 and env2 [n] / [S, n] (speaker 1,
    speaker 2) -- for a CCA bank each speaker's feature block [n, c2] / [S, n, c2] --, host arrays or device
    tensors.  Returns OnlineResult(scores [S, new, 2] float64, decisions [S, new] uint8 -- [S, new, 3] float64
    (p, lower, upper) for 'ssd' --, first_window) for the windows this push completes (host arrays)."""
    self._refuse_flushed()
    if self.kind == 'cca':
      eeg, env = self._as_cca_bank(eeg, env1, env2)
    else:
      eeg, env = self._as_bank(eeg, env1, env2)
    return self._advance(eeg, env, False)

  def flush(self):
    """The end of the recording: the last post_context frames are emitted as if zero rows followed.  After
    it the session refuses pushes until reset()."""
    self._refuse_flushed()
    result = self._advance(None, None, True)
    self.flushed = True
    return result

  def _advance(self, eeg, side, flush):
    """One push of the bank; side is env [S, n, 2], or a CCA bank's (feat1, feat2)."""
    n = 0 if eeg is None else int(eeg.shape[1])
    kind = 'none' if self.decoder_type == 'ssd' else self.decoder_type
    cca = self.kind == 'cca'
    if not self._on_device:
      # the NumPy sessions, one listener each
      if eeg is None:
        eeg = self._no_rows(self.channels)
        side = (self._no_rows(self.features),) * 2 if cca else self._no_rows(2)
      outs = []
      for i, sess in enumerate(self._host):
        mine = (np.stack([np.asarray(f[i], np.float64) for f in side]) if cca else
                np.asarray(side[i], np.float64))
        outs.append(sess.push(np.asarray(eeg[i], np.float64), mine, self.frames_pushed, flush))
      self.frames_pushed += n
      return OnlineResult(np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
                          outs[0][4].first_window)
    d = self._dev
    h = d['h']
    if cca:
      out = self._advance_cca(eeg, side, n, kind, flush)
    else:
      env = side
      if eeg is not None and not hasattr(eeg, 'is_cuda'):
        eeg, env = self._upload(h, eeg), self._upload(h, env)
      if n == 0:
        eeg = env = None
      if self.kind == 'dnn':
        out = device.dnn_online_push(eeg, env, d['params'], self.hidden, d['corr'], d['state'], self.frames_pushed,
                                     self.pre, self.post, self.window_size, self.window_step, self.reduction,
                                     d['lda'], kind, flush=flush, handle=h)
      else:
        out = device.online_push(eeg, env, d['w'], d['b'], d['corr'], d['state'], self.frames_pushed, self.pre,
                                 self.post, self.window_size, self.window_step, self.reduction, d['lda'], kind,
                                 flush=flush, handle=h)
    self.frames_pushed += n
    return self._finish(out)

  def _advance_cca(self, eeg, feats, n, kind, flush):
    """The CCA bank's push on the device: its CcaOnlinePush."""
    d = self._dev
    h = d['h']
    feat1 = feat2 = None
    if n == 0:
      eeg = None
    else:
      up = lambda a: a if hasattr(a, 'is_cuda') else self._upload(h, a)
      eeg, feat1, feat2 = up(eeg), up(feats[0]), up(feats[1])
    return device.cca_online_push(eeg, feat1, feat2, d['mean_x'], d['rot_x'], d['mean_y'], d['rot_y'], d['corr'],
                                  d['state'], self.frames_pushed, self.pre, self.post, self.pre2, self.post2,
                                  self.window_size, self.window_step, self.reduction, d['lda'], kind, flush=flush,
                                  handle=h)

  def _finish(self, out):
    """A device push's windows as an OnlineResult; for 'ssd' through td_decode_ssd_stream first."""
    d = self._dev
    h = d['h']
    new = out.plan.new_windows
    scores = out.scores.permute(1, 2, 0)
    if self._ssd is None:
      return OnlineResult(scores.cpu().numpy(), out.decisions.cpu().numpy(), out.plan.first_window)
    if new == 0:
      return OnlineResult(scores.cpu().numpy(), np.zeros((self.sessions, 0, 3)), out.plan.first_window)
    a = self._ssd
    offsets = np.arange(self.sessions + 1, dtype=np.int64) * new
    probs = device.decode_ssd(out.scores[0].reshape(-1), out.scores[1].reshape(-1), offsets, a.outer_iter,
                              a.inner_iter, a.newton_iter, a.k_f, a.k_b, a._offset, a._prior, handle=h,
                              state=d['ssd_state'])
    return OnlineResult(scores.cpu().numpy(), probs.reshape(self.sessions, new, 3).cpu().numpy(),
                        out.plan.first_window)


# ------------------------------------------------------------------------------------------------ the front end
FRONT_SHARED = ('fs_in', 'fs_out', 'highpass_cutoff', 'highpass_order', 'lowpass_cutoff', 'lowpass_order',
                'ref_channels', 'channels_to_ref', 'channel_numbers', 'pre_context', 'post_context')


def _plain(value):
  """Lists of lists / ranges as nested tuples, for comparing two Preprocessors' parameters."""
  if isinstance(value, (list, tuple, range, np.ndarray)):
    return tuple(_plain(v) for v in value)
  return value


def frontend_parameters(prep):
  """What a front-end session takes from a preprocess.Preprocessor, read and never written: dict(fs_in, fs_out,
  sos [S, 6] or None, zi [S, 2] or None, split, ref_channels, channels_to_ref, select, mean, std).  Refuses, naming
  the parameter: temporal context (the decoder adds its own), data_mean=None (a mean frozen from the first chunk
  depends on the cut: pass the training value), a data_std of 0 or None, more than 16 sections."""
  from telluride_decoding_amd import preprocess
  if not isinstance(prep, preprocess.Preprocessor):
    raise ValueError('OnlinePreprocessor is configured by a preprocess.Preprocessor, not a %s.' % type(prep).__name__)
  for key in ('pre_context', 'post_context'):
    if getattr(prep, key):
      raise ValueError('OnlinePreprocessor adds no temporal context (%s=%s): the decoder adds its own.' %
                       (key, getattr(prep, key)))
  if prep.data_mean is None:
    raise ValueError('OnlinePreprocessor needs data_mean: a mean frozen from the first chunk (data_mean=None) '
                     'depends on the cut; pass the training value.')
  if prep.data_std is None or float(prep.data_std) == 0.0 or not np.isfinite(float(prep.data_std)):
    raise ValueError('OnlinePreprocessor needs a finite data_std other than 0, not %s.' % (prep.data_std,))
  sos = prep.sos
  zi, split = None, 0
  if sos is not None:
    sos = np.ascontiguousarray(sos, np.float64)
    if sos.shape[0] > device.FRONTEND_MAX_SECTIONS:
      raise ValueError('OnlinePreprocessor filters with at most %d second-order sections, not %d.' %
                       (device.FRONTEND_MAX_SECTIONS, sos.shape[0]))
    zi = np.concatenate([np.asarray(z, np.float64) for z in (prep._highpass_zi, prep._lowpass_zi) if z is not None])
    split = prep._n_hp() if prep._lowpass_sos is not None else int(sos.shape[0])
  return dict(fs_in=float(prep.fs_in), fs_out=float(prep.fs_out), sos=sos, zi=zi, split=int(split),
              ref_channels=prep._ref_channels, channels_to_ref=prep._channels_to_ref,
              select=[int(v) for v in prep.channel_numbers] if prep.channel_numbers else None,
              mean=float(prep.data_mean), std=float(prep.data_std))


def host_frontend_plan(rows_before, n, fs_in, fs_out, flush=False):
  """td_frontend_plan in NumPy: (frames_before, frames_after, held, the frames whose row is among the rows pushed
  after this push).  The reference's float64 products in its order (preprocess.resample_indices)."""
  fs_in, fs_out = float(fs_in), float(fs_out)

  def total(rows):                                   # F(N)
    return int(rows) if fs_in == fs_out else int(np.round(float(rows) / fs_in * fs_out))

  def reach(rows):                                   # G(N): the frames j with r_j <= N - 1
    if rows <= 0 or fs_in == fs_out:
      return max(int(rows), 0)
    delta = 1.0 / fs_out
    row = lambda j: int(np.round(j * delta * fs_in))
    g = max(int(float(rows) / fs_in * fs_out), 0)
    while g > 0 and row(g - 1) > rows - 1:
      g -= 1
    while row(g) <= rows - 1:
      g += 1
    return g

  g0, f0, g1, f1 = reach(rows_before), total(rows_before), reach(rows_before + n), total(rows_before + n)
  e0 = min(g0, f0)
  e1 = max(e0, f1 if flush else min(g1, f1))
  return e0, e1, max(g1 - e1, 0), g1


def frame_rows(first, count, fs_in, fs_out):
  """The input rows r_j of the frames [first, first + count): rint((j * (1.0 / fs_out)) * fs_in), int64."""
  j = np.arange(first, first + count)
  if float(fs_in) == float(fs_out):
    return j.astype(np.int64)
  return np.round(j * (1.0 / float(fs_out)) * float(fs_in)).astype(np.int64)


def frontend_groups(cfg, c):
  """The re-reference groups [(reference channels, channels to re-reference)] of frontend_parameters' dict for rows
  of c channels (Preprocessor._groups: a missing side is every channel), checked against the row by name."""
  ref, chans = cfg['ref_channels'], cfg['channels_to_ref']
  groups = []
  if ref is not None or chans is not None:
    ref = [range(c)] if ref is None else ref
    chans = [range(c)] if chans is None else chans
    groups = [([int(v) for v in r], [int(v) for v in ch]) for r, ch in zip(ref, chans)]
  if len(groups) > device.FRONTEND_MAX_GROUPS:
    raise ValueError('OnlinePreprocessor re-references at most %d groups, not %d.' %
                     (device.FRONTEND_MAX_GROUPS, len(groups)))
  for name, lists in (('ref_channels', [g[0] for g in groups]), ('channels_to_ref', [g[1] for g in groups]),
                      ('channel_numbers', [cfg['select'] or []])):
    for values in lists:
      if any(not 0 <= v < c for v in values):
        raise ValueError('%s %s reaches outside a row of %d channels.' % (name, list(values), c))
  if any(not g[0] for g in groups):
    raise ValueError('ref_channels holds a group without a reference channel.')
  return groups


class _HostFrontSession(object):
  """One front-end session in NumPy float64: the semantics of td_frontend_push (the filter's multiply-adds are
  rounded twice here and once on the device)."""

  def __init__(self, cfg, c, groups, mean, std):
    self.cfg, self.c, self.groups, self.mean, self.std = cfg, c, groups, mean, std
    self.reset()

  def reset(self):
    sections = 0 if self.cfg['sos'] is None else self.cfg['sos'].shape[0]
    self.z = np.zeros((sections, 2, self.c), np.float64)
    self.held = np.zeros((self.c,), np.float64)
    self.last = np.zeros((self.c,), np.float64)

  def state(self):
    return np.concatenate([self.z.reshape(-1, self.c), self.held[None], self.last[None]])

  def _filter(self, x, reset):
    sos, zi, split = self.cfg['sos'], self.cfg['zi'], self.cfg['split']
    if sos is None:
      return x.copy()
    y = np.empty(x.shape, np.float64)
    z = self.z
    for t in range(x.shape[0]):
      v = x[t]
      base = v
      for i in range(sos.shape[0]):
        b0, b1, b2, _, a1, a2 = sos[i]
        if reset and t == 0:
          if i == split:
            base = v
          z[i, 0], z[i, 1] = base * zi[i, 0], base * zi[i, 1]
        out = b0 * v + z[i, 0]
        z[i, 0] = -a1 * out + (b1 * v + z[i, 1])
        z[i, 1] = -a2 * out + b2 * v
        v = out
      y[t] = v
    return y

  def push(self, x, rows_before, flush):
    """x [n, c] float64 -> [m, cs] float64."""
    cfg = self.cfg
    n = x.shape[0]
    y = self._filter(x, rows_before == 0)
    e0, e1, _, g1 = host_frontend_plan(rows_before, n, cfg['fs_in'], cfg['fs_out'], flush)
    src = np.minimum(rows_before + n - 1, frame_rows(e0, e1 - e0, cfg['fs_in'], cfg['fs_out'])) - rows_before
    rows = np.empty((e1 - e0, self.c), np.float64)
    for f, r in enumerate(src):
      rows[f] = y[r] if r >= 0 else (self.last if r == -1 else self.held)
    if n > 0:
      r = int(frame_rows(g1 - 1, 1, cfg['fs_in'], cfg['fs_out'])[0]) - rows_before
      if r >= 0:
        self.held = y[r].copy()
      self.last = y[n - 1].copy()
    out = rows.copy()
    for ref, chans in self.groups:
      total = np.zeros((rows.shape[0],), np.float64)
      for ch in ref:                                   # in list order
        total = total + rows[:, ch]
      out[:, list(chans)] -= (total / float(len(ref)))[:, None]      # (a channel listed twice: once)
    if cfg['select'] is not None:
      out = out[:, cfg['select']]
    return (out - self.mean) / self.std


class _FrontEnd(_Bank):
  """What the two front ends share: a bank configured by one object or a list of S, whose row width is known at the
  first push, and one push path.  A class gives
    NAME, OBJECTS     its name and what it is configured by, for the messages; SHARE: its sentence for two objects
                      that differ in a setting (key, the first's value, this one's)
    ROWS, WIDTH       what a push's argument and its width are called in the shape message
    DTYPES            the dtypes a push passes on as they are; a host array of another goes through HOST_CAST (a
                      device tensor through float32)
    COLUMN            whether one session's 1-D push is a column
    CAST_ERRSTATE     np.errstate's arguments around the NumPy sessions' float64 -> float32
    _parameters(object) -> cfg; _settings(object, cfg) -> {key: the value a bank shares}
    _setup(c)         the sessions, once the width is known
    _host_push(x or None, flush) -> float64 [S, m, cs]
    _to_device(host rows, h) -> tensor; _device_push(x or None, flush, want64) -> a push with out32, out64, plan."""
  DTYPES = ('float32', 'float64')
  HOST_CAST, COLUMN, CAST_ERRSTATE = np.float64, False, {}

  def __init__(self, objects, num_sessions):
    if not isinstance(objects, (list, tuple)):
      objects = [objects] * (1 if num_sessions is None else int(num_sessions))
    elif num_sessions is not None and int(num_sessions) != len(objects):
      raise ValueError('%s: %d %s for num_sessions=%d.' % (self.NAME, len(objects), self.OBJECTS, int(num_sessions)))
    if not objects:
      raise ValueError('%s needs at least one session.' % self.NAME)
    self._cfgs = [self._parameters(o) for o in objects]
    first = self._settings(objects[0], self._cfgs[0])
    for o, cfg in zip(objects[1:], self._cfgs[1:]):
      for key, value in self._settings(o, cfg).items():
        if _plain(value) != _plain(first[key]):
          raise ValueError(self.SHARE % (key, first[key], value))
    self._cfg = self._cfgs[0]
    _Bank.__init__(self, len(objects), device.gpu_available())
    self.fs_in, self.fs_out = self._cfg['fs_in'], self._cfg['fs_out']
    self.channels = None                         # the row's width: known at the first push
    self.rows_pushed = self.frames_emitted = 0
    self._tensors = False
    self._host_dtypes = [np.dtype(name) for name in self.DTYPES]
    self._device_dtypes = [getattr(device._torch(), name) for name in self.DTYPES] if self._on_device else None

  def reset(self):
    self.rows_pushed = self.frames_emitted = 0
    _Bank.reset(self)

  def _flush(self, want64):
    self._refuse_flushed()
    out = self._advance(None, True, want64)
    self.flushed = True
    return out

  def _advance(self, rows, flush, want64):
    on_dev_in = self._tensors if rows is None else hasattr(rows, 'is_cuda')
    self._tensors = on_dev_in                    # (a flush answers as the last push did)
    if rows is not None:
      if not on_dev_in:
        rows = np.asarray(rows)
        if rows.dtype not in self._host_dtypes:
          rows = rows.astype(self.HOST_CAST)
      if self.COLUMN and len(rows.shape) == 1 and self.sessions == 1:
        rows = rows.reshape(-1, 1)
      if len(rows.shape) == 2 and self.sessions == 1:
        rows = rows[None]
      if len(rows.shape) != 3 or int(rows.shape[0]) != self.sessions or (
          self.channels is not None and int(rows.shape[2]) != self.channels):
        width = self.channels or self.WIDTH
        raise ValueError('A push is %s [%d, n, %s] (or [n, %s] for one session), not %s.' %
                         (self.ROWS, self.sessions, width, width, tuple(rows.shape)))
      if self.channels is None:
        self._setup(int(rows.shape[2]))
    n = 0 if rows is None else int(rows.shape[1])
    if self.channels is None:                    # (a flush before any row)
      empty = np.zeros((self.sessions, 0, 0), np.float32)
      return (empty, empty.astype(np.float64)) if want64 else empty
    if not self._on_device:
      out64 = self._host_push(rows.cpu().numpy() if hasattr(rows, 'cpu') else rows, flush)
      self.rows_pushed += n
      self.frames_emitted += out64.shape[1]
      with np.errstate(**self.CAST_ERRSTATE):
        out32 = out64.astype(np.float32)
      if on_dev_in:
        out32, out64 = device._torch().from_numpy(out32), device._torch().from_numpy(out64)
      return (out32, out64) if want64 else out32
    x = None
    if n > 0:
      if on_dev_in:
        x = rows if rows.dtype in self._device_dtypes else rows.to(device._torch().float32)
        if x.stride(2) != 1 and self.channels > 1:
          x = x.contiguous()
      else:
        x = self._to_device(rows, self._dev['h'])
    out = self._device_push(x, flush, want64)
    self.rows_pushed += n
    self.frames_emitted = out.plan.frames_after
    out32, out64 = out.out32, out.out64
    if not on_dev_in:
      out32, out64 = out32.cpu().numpy(), out64.cpu().numpy() if want64 else None
    return (out32, out64) if want64 else out32


class OnlinePreprocessor(_FrontEnd):
  """The online EEG front end: a bank of S sessions that take raw rows in pushes of any length and give the
  conditioned float32 frames OnlineDecoder.push takes as `eeg` -- one td_frontend_push launch per push, the filter
  state and the resample phase on the device, and any cut of a recording gives the bytes of one push.

  preprocessors: one preprocess.Preprocessor (num_sessions sessions share it, default 1) or a list of S of them,
  which share everything except data_mean / data_std.  The objects are read, never written, and never run: the
  filters (high-pass sections, then low-pass ones), the stage split, the rates, the re-reference groups and the
  channel selection come from them.  The steps and their order are Preprocessor.process's; the output over any cut
  has the rows of process(whole, reset=True).  Refused by name: pre_context / post_context (the decoder adds its
  own), data_mean=None, a data_std of 0 or None, more than 16 sections; at the first push, a row of more than 128
  channels and selected or group channels outside it.

  Without a GPU the same object runs a NumPy float64 session of the same semantics."""

  NAME, OBJECTS, ROWS, WIDTH = 'OnlinePreprocessor', 'preprocessors', 'raw', 'C'
  SHARE = 'The sessions of a bank share everything except data_mean and data_std: %s is %s and %s.'
  FLUSHED = 'The front end was flushed: reset() starts the next recording.'
  _parameters = staticmethod(frontend_parameters)

  def __init__(self, preprocessors, num_sessions=None):
    _FrontEnd.__init__(self, preprocessors, num_sessions)
    self.sections = 0 if self._cfg['sos'] is None else int(self._cfg['sos'].shape[0])
    self.channels_out = None

  @staticmethod
  def _settings(prep, cfg):
    return dict((key, getattr(prep, key)) for key in FRONT_SHARED)

  # -- state -------------------------------------------------------------------------------------
  def _setup(self, c):
    cfg = self._cfg
    if not 1 <= c <= device.FRONTEND_MAX_CHANNELS:
      raise ValueError('OnlinePreprocessor takes rows of 1 to %d channels, not %d.' % (device.FRONTEND_MAX_CHANNELS, c))
    groups = frontend_groups(cfg, c)
    self.channels, self._groups = c, groups
    self.channels_out = len(cfg['select']) if cfg['select'] is not None else c
    if self.channels_out < 1:
      raise ValueError('channel_numbers selects no channel.')
    if not self._on_device:
      self._host = [_HostFrontSession(cfg, c, groups, k['mean'], k['std']) for k in self._cfgs]
      return
    h = device.default_handle()
    stats = np.array([[k['mean'], k['std']] for k in self._cfgs], np.float64)
    if np.all(stats == stats[0]):
      stats = stats[:1]                          # (one pair every session reads)
    nbytes = device.frontend_state_bytes(c, self.sections)
    self._dev = dict(h=h, mean=h.to_device(stats[:, 0:1], np.float64).reshape(-1),
                     std=h.to_device(stats[:, 1:2], np.float64).reshape(-1), state=self._zero_state(h, nbytes))

  def reset(self):
    """A fresh recording: zero state, no row pushed; the filters reset on the next push's first row."""
    _FrontEnd.reset(self)

  @property
  def state(self):
    """The sessions' state blocks [S, 2 sections + 2, C] float64 -- the filter state in scipy's zi layout
    (Preprocessor.filter_state's), the held row, the last row -- as a device tensor (a view) or a host array; None
    before the first push."""
    if self._dev is not None:
      return self._dev['state'].view(device._torch().float64).reshape(self.sessions, -1, self.channels)
    if self._host is not None:
      return np.stack([sess.state() for sess in self._host])
    return None

  # -- pushes ------------------------------------------------------------------------------------
  def push(self, raw, want64=False):
    """The next n raw rows of every session: raw [n, C] (one session) or [S, n, C], float32 or float64, a host
    array or a device tensor; n may be 0.  Returns the frames this push emits, [S, m, cs] float32 (m may be 0): a
    device tensor for a device tensor -- what OnlineDecoder.push takes as eeg, unchanged -- else a host array.
    want64: (the float32 frames, the same frames before the cast, float64)."""
    self._refuse_flushed()
    return self._advance(raw, False, want64)

  def flush(self, want64=False):
    """The end of the recording: emits the frames resample_indices counts for the rows pushed that no push has
    emitted yet (when upsampling, from the last row), as the pushes returned theirs.  After it the front end
    refuses pushes until reset()."""
    return self._flush(want64)

  def _host_push(self, x, flush):
    if x is None:
      x = self._no_rows(self.channels, np.float64)
    return np.stack([sess.push(np.asarray(x[i], np.float64), self.rows_pushed, flush)
                     for i, sess in enumerate(self._host)])

  @staticmethod
  def _to_device(raw, h):
    return device._torch().from_numpy(np.ascontiguousarray(raw)).to(h.device)

  def _device_push(self, x, flush, want64):
    cfg, d = self._cfg, self._dev
    return device.frontend_push(x, cfg['sos'], cfg['split'], cfg['zi'], cfg['fs_in'], cfg['fs_out'], self._groups,
                                cfg['select'], d['mean'], d['std'], d['state'], self.rows_pushed, c=self.channels,
                                flush=flush, want64=want64, handle=d['h'])


# ------------------------------------------------------------------------------------------------ the audio front end
AUDIO_SHARED = ('fs_in', 'fs_out', 'window', 'exponent')


def audio_parameters(features):
  """What an online audio session takes from a preprocess.AudioFeatures, read and never written: dict(fs_in,
  fs_out, window, exponent) as floats.  Refuses by name the reference's pass-through case (fs_out >= fs_in and
  window <= 1: compute_intensity returns its input there, there is nothing to compute) and a rate, window or
  exponent that is not a finite number."""
  from telluride_decoding_amd import preprocess
  if not isinstance(features, preprocess.AudioFeatures):
    raise ValueError('OnlineAudioFeatures is configured by a preprocess.AudioFeatures, not a %s.' %
                     type(features).__name__)
  cfg = dict((key, float(getattr(features, '_' + key))) for key in AUDIO_SHARED)
  for key in AUDIO_SHARED:
    if not np.isfinite(cfg[key]) or (key != 'exponent' and cfg[key] <= 0):
      raise ValueError('OnlineAudioFeatures needs a finite%s %s, not %s.' %
                       ('' if key == 'exponent' else ' positive', key, cfg[key]))
  if cfg['fs_out'] >= cfg['fs_in'] and cfg['window'] <= 1:
    raise ValueError('OnlineAudioFeatures: fs_out=%g >= fs_in=%g with window=%g <= 1 is the pass-through case: '
                     'compute_intensity returns its input there, there is nothing to compute.' %
                     (cfg['fs_out'], cfg['fs_in'], cfg['window']))
  return cfg


def audio_tail_rows(fs_in, fs_out, window):
  """K, the rows an online audio session carries: ceil((window / 2 + max(window / 2, 0.5)) fs_in / fs_out) + 2."""
  half = 0.5 * float(window)
  return int(np.ceil((half + max(half, 0.5)) * float(fs_in) / float(fs_out))) + 2


def audio_window(i, fs_in, fs_out, window):
  """(a_i, u_i) of frame i, unclamped: Python floats in the reference's order, half-even."""
  hw = 0.5 * window / fs_out
  t = float(i) / fs_out
  return int(round(fs_in * (t - hw))), int(round(fs_in * (t + hw)))


def host_audio_plan(rows_before, n, fs_in, fs_out, window, flush=False):
  """td_audio_online_plan in Python floats: (frames_before, frames_after, held, K)."""
  fs_in, fs_out, window = float(fs_in), float(fs_out), float(window)
  hw = 0.5 * window / fs_out
  upper = lambda i: audio_window(i, fs_in, fs_out, window)[1]

  def total(rows):                                   # F(N)
    return int(round(float(rows) / fs_in * fs_out))

  def reach(rows):                                   # G(N): the frames i with u_i <= N
    g = max(int((float(rows) / fs_in - hw) * fs_out), 0)
    while g > 0 and upper(g - 1) > rows:
      g -= 1
    while upper(g) <= rows:
      g += 1
    return g

  rows_after = rows_before + n
  e0 = min(reach(rows_before), total(rows_before))
  f1 = total(rows_after)
  e1 = max(e0, f1 if flush else min(reach(rows_after), f1))
  return e0, e1, f1 - e1, audio_tail_rows(fs_in, fs_out, window)


class _HostAudioSession(object):
  """One online audio session in NumPy: the semantics of td_audio_online_push -- float32 squares, float64 sums (in
  numpy's row order, where the device adds a lane's rows and then the butterfly), the tail of the last K rows."""

  def __init__(self, cfg, c):
    self.cfg, self.c = cfg, c
    self.k = audio_tail_rows(cfg['fs_in'], cfg['fs_out'], cfg['window'])
    self.reset()

  def reset(self):
    self.tail = np.zeros((self.k, self.c), np.float32)

  def push(self, x, rows_before, flush):
    """x [n, c] -> (frames [m, c] float64, windows [m, 2] int64)."""
    cfg = self.cfg
    n = x.shape[0]
    sq = np.asarray(x).astype(np.float32)
    sq = sq * sq
    rows = np.concatenate([self.tail, sq])             # row r of the recording at r - base
    base, rows_after = rows_before - self.k, rows_before + n
    e0, e1, _, _ = host_audio_plan(rows_before, n, cfg['fs_in'], cfg['fs_out'], cfg['window'], flush)
    out = np.full((e1 - e0, self.c), np.nan)
    win = np.zeros((e1 - e0, 2), np.int64)
    for f in range(e1 - e0):
      a, u = audio_window(e0 + f, cfg['fs_in'], cfg['fs_out'], cfg['window'])
      t1, t2 = max(0, a), min(rows_after, u)
      win[f] = t1, t2
      if t1 - base < 0:
        raise ValueError('frame %d reaches back to row %d, behind the %d carried rows' % (e0 + f, t1, self.k))
      if t2 > t1:
        span = np.array(rows[t1 - base:t2 - base], np.float64, order='C')     # (a copy: the sum sees the span alone)
        out[f] = np.add.reduce(span, axis=0) / float(t2 - t1)
    if n > 0:
      self.tail = np.ascontiguousarray(rows[-self.k:])
    with np.errstate(invalid='ignore', divide='ignore'):
      return np.sqrt(out) ** cfg['exponent'], win


class OnlineAudioFeatures(_FrontEnd):
  """The online audio front end: a bank of S sessions that take audio rows in pushes of any length and give the
  intensity envelopes OnlineDecoder.push takes as env1 / env2 -- one td_audio_online_push launch per push, the last
  K rows' squares on the device, and any cut of a recording gives the bytes of one push: the frames of
  AudioFeatures(...).compute_intensity(whole) on a fresh object, with the same windows and the same count (the
  batch call restarts its window centres on every call: DESIGN.md section 13).

  features: one preprocess.AudioFeatures (num_sessions sessions share it, default 1) or a list of S of them that
  share fs_in, fs_out, window and exponent.  The objects are read, never written, and never run.  A push is always
  [n, c] (or [S, n, c]): nothing is transposed.  Column k of the output is speaker k.  Refused by name: the
  pass-through case (fs_out >= fs_in and window <= 1), more than 8 channels, a window that carries more than 8192
  rows.  The auditory spectrogram has no online form: it is scaled by the maximum over the whole recording.

  Without a GPU the same object runs a NumPy float64 session of the same semantics."""

  NAME, OBJECTS, ROWS, WIDTH = 'OnlineAudioFeatures', 'AudioFeatures', 'audio', 'c'
  SHARE = 'The sessions of a bank share fs_in, fs_out, window and exponent: %s is %s and %s.'
  FLUSHED = 'The audio front end was flushed: reset() starts the next recording.'
  DTYPES = ('int16', 'float32', 'float64')
  HOST_CAST, COLUMN, CAST_ERRSTATE = np.float32, True, dict(over='ignore')
  _parameters = staticmethod(audio_parameters)

  def __init__(self, features, num_sessions=None):
    _FrontEnd.__init__(self, features, num_sessions)
    self.window, self.exponent = self._cfg['window'], self._cfg['exponent']
    self.tail_rows = audio_tail_rows(self.fs_in, self.fs_out, self.window)
    if self.tail_rows > device.AUDIO_ONLINE_MAX_TAIL:
      raise ValueError('OnlineAudioFeatures: %g -> %g Hz with window=%g carries %d rows (at most %d).' %
                       (self.fs_in, self.fs_out, self.window, self.tail_rows, device.AUDIO_ONLINE_MAX_TAIL))
    self._live = 0

  @staticmethod
  def _settings(features, cfg):
    return cfg

  def _setup(self, c):
    if not 1 <= c <= device.AUDIO_ONLINE_MAX_CHANNELS:
      raise ValueError('OnlineAudioFeatures takes rows of 1 to %d channels, not %d (a push is [n, c]: nothing is '
                       'transposed).' % (device.AUDIO_ONLINE_MAX_CHANNELS, c))
    self.channels = c
    if not self._on_device:
      self._host = [_HostAudioSession(self._cfg, c) for _ in range(self.sessions)]
      return
    h = device.default_handle()
    self._dev = dict(h=h, state=self._zero_state(h, device.audio_online_state_bytes(c, self.tail_rows)))

  def reset(self):
    """A fresh recording: zero state, no row pushed."""
    self._live = 0
    _FrontEnd.reset(self)

  @property
  def state(self):
    """The live tail copy of every session, [S, K, c] float32: the squares of the last K rows pushed, slot j holding
    row rows_pushed - K + j (zero before row 0) -- a device tensor (a view) or a host array; None before the first
    push."""
    if self._dev is not None:
      blocks = self._dev['state'].view(device._torch().float32)
      return blocks.reshape(self.sessions, 2, self.tail_rows, self.channels)[:, self._live]
    if self._host is not None:
      return np.stack([sess.tail for sess in self._host])
    return None

  def push(self, audio, want64=False):
    """The next n rows of every session: audio [n, c] (one session; [n] is one channel) or [S, n, c], int16,
    float32 or float64 (anything else goes through float32, as compute_intensity's astype does), a host array or a
    device tensor; n may be 0.  Returns the frames this push emits, [S, m, c] float32 (m may be 0): a device tensor
    for a device tensor, else a host array.  want64: (the float32 frames, the float64 frames they were rounded
    from -- the reference's dtype)."""
    self._refuse_flushed()
    return self._advance(audio, False, want64)

  def flush(self, want64=False):
    """The end of the recording: emits every frame of int(round(rows_pushed / fs_in * fs_out)) that no push has
    emitted yet, its window clamped at the last row, as compute_intensity(whole) does.  After it the front end
    refuses pushes until reset()."""
    return self._flush(want64)

  def _host_push(self, x, flush):
    if x is None:
      x = self._no_rows(self.channels)
    return np.stack([sess.push(x[i], self.rows_pushed, flush)[0] for i, sess in enumerate(self._host)])

  @staticmethod
  def _to_device(audio, h):
    # (a copy: the caller's may be read-only)
    return device._torch().from_numpy(np.array(audio, order='C')).to(h.device)

  def _device_push(self, x, flush, want64):
    cfg, d = self._cfg, self._dev
    out = device.audio_online_push(x, cfg['fs_in'], cfg['fs_out'], cfg['window'], cfg['exponent'], d['state'],
                                   self._live, self.rows_pushed, c=self.channels, flush=flush, want64=want64,
                                   handle=d['h'])
    self._live = out.live
    return out


# ------------------------------------------------------------------------------------------------ joining the streams
FrameJoinFlush = collections.namedtuple('FrameJoinFlush', ['blocks', 'beyond'])


class FrameJoin(object):
  """Lines up the frames of several online streams that emit at their own pace -- the EEG front end and the audio
  front end, whose envelope frame i needs half a window of audio behind frame i and so arrives later than EEG frame
  i:

      eeg = front.push(raw)
      env = audio.push(pcm)
      result = decoder.push(*join.push(eeg, env[..., 0], env[..., 1]))

  push(*blocks) takes every stream's newly emitted frames (any count, possibly none) and returns, per stream, the
  frames no earlier call has returned, up to the smallest count any stream has delivered so far; the rest waits
  inside the object.  Frames lie along `axis` (1: the banks' [S, m, ...] layout, the default; 0 for one session's
  [m, ...]).  Host arrays stay host arrays and device tensors stay on the device: nothing is copied to the host."""

  def __init__(self, num_streams, axis=1):
    if int(num_streams) < 1:
      raise ValueError('FrameJoin needs at least one stream.')
    self.num_streams, self.axis = int(num_streams), int(axis)
    self.reset()

  def reset(self):
    self._wait = [None] * self.num_streams       # what each stream delivered beyond the frames returned
    self.frames_returned = 0
    self.frames_delivered = [0] * self.num_streams

  def _count(self, block):
    return 0 if block is None else int(block.shape[self.axis])

  def _cut(self, block, lo, hi):
    if hasattr(block, 'narrow'):
      return block.narrow(self.axis, lo, hi - lo)
    index = [slice(None)] * len(block.shape)
    index[self.axis] = slice(lo, hi)
    return block[tuple(index)]

  def _append(self, waiting, block):
    if self._count(waiting) == 0:
      return block
    if self._count(block) == 0:
      return waiting
    if hasattr(waiting, 'narrow') and hasattr(block, 'narrow'):
      return device._torch().cat([waiting, block], dim=self.axis)
    return np.concatenate([np.asarray(waiting), np.asarray(block)], axis=self.axis)

  def push(self, *blocks):
    """The frames every stream has now, not returned before: a tuple of num_streams blocks of one frame count."""
    if len(blocks) != self.num_streams:
      raise ValueError('FrameJoin.push takes %d blocks, one per stream, not %d.' % (self.num_streams, len(blocks)))
    for i, block in enumerate(blocks):
      if len(block.shape) <= self.axis:
        raise ValueError('Stream %d: a block of shape %s has no axis %d.' % (i, tuple(block.shape), self.axis))
      self._wait[i] = self._append(self._wait[i], block)
      self.frames_delivered[i] += self._count(block)
    m = min(self._count(w) for w in self._wait)
    out = tuple(self._cut(w, 0, m) for w in self._wait)
    self._wait = [self._cut(w, m, self._count(w)) for w in self._wait]
    self.frames_returned += m
    return out

  def flush(self, *blocks):
    """The end: push(*blocks) when the streams' last blocks are given (their flush() outputs), then
    FrameJoinFlush(blocks: the common rest, beyond: how many frames each stream had beyond it -- they are dropped)."""
    if blocks:
      out = self.push(*blocks)
    elif any(w is None for w in self._wait):
      raise ValueError('FrameJoin.flush before any push needs the blocks.')
    else:
      out = tuple(self._cut(w, 0, 0) for w in self._wait)
    beyond = [self._count(w) for w in self._wait]
    self._wait = [self._cut(w, 0, 0) for w in self._wait]
    return FrameJoinFlush(out, beyond)


# ------------------------------------------------------------------------------------------------ the online fit
MAX_FIT_PUSH = 1048576                     # TD_ONLINE_MAX_PUSH


class _TrainingBank(_Bank):
  """What the five training banks share (OnlineRidgeFit, OnlineCCAFit, OnlineCalibration, OnlineDNNCalibration,
  OnlineCCACalibration): rows arrive in pushes of any length, the frames counted run `delay` rows behind them until a flush counts the rest, and a
  push is one device call or one call per NumPy session.  A class gives LAST_ROWS (flush's sentence for some of the
  last rows), _blocks(*rows) (the arguments of a push as [S, n, .] blocks, the EEG first), _no_blocks() (what the
  NumPy sessions take for a flush without rows), _session_push(sess, i, blocks, flush) and _device_push(blocks,
  flush) (blocks None without rows); both read rows_pushed and _pushes as they stood before the push."""
  LAST_ROWS = None

  def __init__(self, sessions, on_device, delay, handle, state_bytes, host_session):
    """handle() and state_bytes() are called on the device, host_session() S times off it."""
    _Bank.__init__(self, sessions, on_device)
    self.delay = delay
    if on_device:
      h = handle()
      self._dev = dict(h=h, state=self._zero_state(h, state_bytes()))
    else:
      self._host = [host_session() for _ in range(sessions)]
    self.reset()

  def reset(self):
    """A fresh recording: zero state (a memset), no row pushed."""
    self.rows_pushed = 0
    self._pushes = 0                             # pushes with rows: its parity is the fits' live tail copy
    _Bank.reset(self)

  @property
  def _counted(self):
    """The frames counted so far: `delay` behind the rows pushed, all of them after flush()."""
    return self.rows_pushed if self.flushed else max(0, self.rows_pushed - self.delay)

  def _float32(self, *arrays):
    """Each of `arrays` (tensors or arrays) as float32 where the bank runs: device tensors, else host arrays."""
    if not self._on_device and not any(hasattr(a, 'is_cuda') for a in arrays):
      return [np.asarray(a, np.float32) for a in arrays]
    torch = device._torch()
    where = self._dev['h'].device if self._on_device else None
    out = [(a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a, np.float32))).to(
        device=where, dtype=torch.float32) for a in arrays]
    return out if self._on_device else [a.cpu().numpy() for a in out]

  def _push(self, rows, flush):
    """push(*rows) / flush(*rows): the frames counted after it."""
    self._refuse_flushed()
    blocks = None
    if not flush or self._last_rows(self.LAST_ROWS, *rows):
      blocks = self._blocks(*rows)
      if int(blocks[0].shape[1]) > MAX_FIT_PUSH:
        raise ValueError('%s takes at most %d rows in one push, not %d.' %
                         (type(self).__name__, MAX_FIT_PUSH, blocks[0].shape[1]))
    n = 0 if blocks is None else int(blocks[0].shape[1])
    if self._on_device:
      self._device_push(blocks if n > 0 else None, flush)
    else:
      for i, sess in enumerate(self._host):
        self._session_push(sess, i, self._no_blocks() if blocks is None else blocks, flush)
    self.rows_pushed += n
    if n > 0:
      self._pushes += 1
    self.flushed = flush
    return self._counted


class _FitBank(_TrainingBank):
  """What the two fit banks share: sessions of their own with a forgetting factor, two streams of rows (the EEG and
  what is fitted to it), moments in float64 at the head of the state and two copies of the streams' tails behind
  them.  A class gives SHAPES (the sentence for a push of other shapes), and to _setup the streams' widths, the
  head's length in doubles, the tails' shapes and names in a NumPy session, and its device push, called as
  device_push(eeg, side, state, rows_pushed, pushes, flush=, forget=, handle=)."""
  FLUSHED = 'The fit was flushed: reset() starts the next recording.'
  SHAPES = None

  def _setup(self, num_sessions, forgetting, delay, widths, head_doubles, tails, state_bytes, host_session,
             device_push):
    if int(num_sessions) < 1:
      raise ValueError('%s needs at least one session.' % type(self).__name__)
    self.forgetting = forgetting
    self._widths, self._head_doubles, self._tails, self._device_call = widths, head_doubles, tails, device_push
    _TrainingBank.__init__(self, int(num_sessions), device.gpu_available(), delay, device.default_handle,
                           state_bytes, host_session)

  frames = _TrainingBank._counted                # the frames counted into the moments so far

  def _to_bank(self, eeg, side):
    """One session's [n, .] rows as [1, n, .]."""
    if len(eeg.shape) == 2 and len(side.shape) == 2 and self.sessions == 1:
      eeg, side = eeg.reshape((1,) + tuple(eeg.shape)), side.reshape((1,) + tuple(side.shape))
    return eeg, side

  def _blocks(self, eeg, side):
    """(eeg [S, n, c], side [S, n, c2]) float32: device tensors on the device, else host arrays."""
    s, (c, c2) = self.sessions, self._widths
    eeg, side = self._float32(eeg, side)
    shapes = (tuple(eeg.shape), tuple(side.shape))
    eeg, side = self._to_bank(eeg, side)
    n = int(eeg.shape[1]) if len(eeg.shape) == 3 else -1
    if len(eeg.shape) != 3 or tuple(eeg.shape) != (s, n, c) or tuple(side.shape) != (s, n, c2):
      raise ValueError(self.SHAPES % ((s, c, c, s, c2, c2) + shapes))
    return eeg, side

  def _no_blocks(self):
    return self._no_rows(self._widths[0]), self._no_rows(self._widths[1])

  def _session_push(self, sess, i, blocks, flush):
    sess.push(blocks[0][i], blocks[1][i], self.rows_pushed, flush)

  def _device_push(self, blocks, flush):
    d = self._dev
    eeg, side = blocks or (None, None)
    if blocks is not None:                       # (the device call takes unit column strides)
      eeg, side = (t.contiguous() if t.stride(2) != 1 and w > 1 else t for t, w in zip(blocks, self._widths))
    self._device_call(eeg, side, d['state'], self.rows_pushed, self._pushes, flush=flush, forget=self.forgetting,
                      handle=d['h'])

  @property
  def tails(self):
    """(EEG tail, the other stream's tail) float32, [S, rows, width] each: the live copy -- slot j of a tail of
    `rows` rows holds row rows_pushed - rows + j, zero before row 0.  The EEG's tail has pre_context + delay rows;
    the ridge fit's target tail delay rows, the CCA fit's feature tail input2_pre_context + delay.  Device tensors
    (views) or host arrays."""
    if self._dev is None:
      return tuple(np.stack([getattr(sess, name) for sess in self._host]) for name, _, _ in self._tails)
    floats = self._dev['state'].view(device._torch().float32)
    (_, r1, c1), (_, r2, c2) = self._tails
    copy = r1 * c1 + r2 * c2
    at = 2 * self._head_doubles + (self._pushes & 1) * copy
    return (floats[:, at:at + r1 * c1].reshape(self.sessions, r1, c1),
            floats[:, at + r1 * c1:at + copy].reshape(self.sessions, r2, c2))

  def _check_model(self, model, kind, pairs, session):
    """update_model's refusals: a model of another class, a (name, mine, the model's attribute) that differs, the
    session; returns the session."""
    who = '%s.update_model' % type(self).__name__
    if not isinstance(model, kind):
      raise ValueError('%s takes a %s, not a %s.' % (who, kind.__name__, type(model).__name__))
    for name, mine, attribute in pairs:
      theirs = int(getattr(model, attribute))
      if theirs != mine:
        raise ValueError('%s: the model has %s = %d, the fit %d.' % (who, name, theirs, mine))
    if not 0 <= int(session) < self.sessions:
      raise ValueError('%s: session %d of %d.' % (who, int(session), self.sessions))
    return int(session)


def _check_fit_shape(who, c, pre, post, d, g):
  """td_fit_online_push's limits, refused by name (the device call repeats them)."""
  if not 1 <= c <= device.ONLINE_FIT_MAX_CHANNELS:
    raise ValueError('%s takes 1 to %d channels, not %d.' % (who, device.ONLINE_FIT_MAX_CHANNELS, c))
  if pre < 0 or post < 0 or pre + 1 + post > device.ONLINE_FIT_MAX_LAGS:
    raise ValueError('%s takes at most %d lags, not %d + 1 + %d.' % (who, device.ONLINE_FIT_MAX_LAGS, pre, post))
  if (pre + 1 + post) * c > device.ONLINE_FIT_MAX_K:
    raise ValueError('%s takes at most %d lagged inputs, not %d lags x %d channels = %d.' %
                     (who, device.ONLINE_FIT_MAX_K, pre + 1 + post, c, (pre + 1 + post) * c))
  if not 1 <= d <= device.ONLINE_FIT_MAX_OUTPUTS:
    raise ValueError('%s takes 1 to %d outputs, not %d.' % (who, device.ONLINE_FIT_MAX_OUTPUTS, d))
  if not 0.0 < g <= 1.0:
    raise ValueError('%s takes a forgetting factor in (0, 1], not %r.' % (who, g))


class _HostRidgeFitSession(object):
  """One online fit session in NumPy: the semantics of td_fit_online_push bit for bit -- float32 rows, float64
  moments, one A * g + outer(v, v) per emitted frame in frame order -- and np.linalg.solve for the weights."""

  def __init__(self, c, pre, post, d, g):
    self.c, self.pre, self.post, self.d, self.g = c, pre, post, d, float(g)
    self.k = (pre + 1 + post) * c
    self.reset()

  def reset(self):
    n1 = self.k + 1
    self.a = np.zeros((n1, n1), np.float64)
    self.b = np.zeros((n1, self.d), np.float64)
    self.tail = np.zeros((self.pre + self.post, self.c), np.float32)
    self.target_tail = np.zeros((self.post, self.d), np.float32)

  def push(self, eeg, target, frames_before, flush):
    """eeg [n, c], target [n, d] float32 behind frames_before rows; returns the frames this push emitted."""
    lags = self.pre + 1 + self.post
    # rows[0] is EEG row frames_before - (pre + post), ys[0] target row frames_before - post
    rows, self.tail = _session_rows(self.tail, eeg, self.post, flush)
    ys, self.target_tail = _session_rows(self.target_tail, target, self.post, False)
    _, emitted, i0 = _session_frames(frames_before, eeg.shape[0], self.post, flush)
    v = np.ones((self.k + 1,), np.float64)
    for i in range(i0, i0 + emitted):
      v[:self.k] = rows[i:i + lags].reshape(-1)
      y = ys[i].astype(np.float64)
      self.a = self.a * self.g + np.outer(v, v)
      self.b = self.b * self.g + np.outer(v, y)
    return emitted

  def solve(self, lambdas):
    """(W [n_lambda, K, d], b [n_lambda, d]) float64: np.linalg.solve of the reference's cov_x and cov_xy."""
    count = self.a[self.k, self.k]
    n1 = self.k + 1
    sols = [np.linalg.solve(self.a / count + lam * np.identity(n1), self.b / count) for lam in lambdas]
    return np.stack([s[:self.k] for s in sols]), np.stack([s[self.k] for s in sols])


class OnlineRidgeFit(_FitBank):
  """The online chain's training stage: a bank of S sessions that take (eeg, target) rows in pushes of any length
  and keep the EXACT moments of the lagged ridge regression -- [x~ | 1]^T [x~ | 1] and [x~ | 1]^T y in float64, the
  lagged vector that of brain_data's context, the trailing 1 the reference's ones column -- in ONE
  td_fit_online_push launch per push, the state on the device.  Any cut of a recording gives the same bytes.
  `solve(lambdas)` turns them into ridge weights on the device (the reference's cov_x + lambda I, lambda on the
  bias entry too) and `OnlineDecoder.set_weights` takes those without a host copy:

      fit = OnlineRidgeFit(channels=64, pre_context=0, post_context=20)
      for eeg, attended in calibration_chunks:           # [n, 64] and [n] float32, any n
        fit.push(eeg, attended)
      w, b = fit.solve([0.1])                            # [1, 1, K, 1] and [1, 1, 1] device tensors
      decoder.set_weights(w[:, 0, :, 0], b[:, 0, 0])     # device to device

  A frame needs post_context rows of future EEG, so the moments run `delay` = post_context frames behind the
  input; flush() ends the recording (zero rows behind it, like the batch route's padding) and counts the rest.
  forgetting g in (0, 1]: every emitted frame first scales the moments by g, so a frame that is m frames old
  weighs g^m and A[K][K] -- what solve divides by -- is the effective frame count.  The batch route
  (`LagStats.accumulate`) treats every call's rows as whole files, padded with zeros at both ends, and so cannot be
  called per chunk; this object is that accumulate for rows that arrive in pieces.

  Refused by name: more than 128 channels, more than 64 lags, more than 2048 lagged inputs, outputs outside
  1 .. 8, a push of more than 1048576 rows, a forgetting factor outside (0, 1].  Without a GPU the same object
  runs a NumPy session of the same semantics, bit for bit (np.linalg.solve for the weights)."""
  LAST_ROWS = 'OnlineRidgeFit.flush takes the last rows as eeg AND target, or neither.'
  SHAPES = ('A push is eeg [%d, n, %d] (or [n, %d] for one session) with a target [%d, n, %d] (or [n, %d] '
            '/ [n] for one session), not eeg %s with a target %s.')

  def __init__(self, channels, pre_context, post_context, outputs=1, num_sessions=1, forgetting=1.0):
    c, pre, post, d = int(channels), int(pre_context), int(post_context), int(outputs)
    g = float(forgetting)
    _check_fit_shape('OnlineRidgeFit', c, pre, post, d, g)
    self.channels, self.pre, self.post, self.outputs = c, pre, post, d
    self.lags = pre + 1 + post
    self.inputs = self.lags * c                  # K
    n1 = self.inputs + 1
    self._setup(num_sessions, g, post, (c, d), n1 * n1 + n1 * d,
                (('tail', pre + post, c), ('target_tail', post, d)),
                lambda: device.online_fit_state_bytes(c, pre, post, d),
                lambda: _HostRidgeFitSession(c, pre, post, d, g),
                lambda *args, **kwargs: device.online_fit_push(*args, pre, post, c=c, d=d, **kwargs))

  # -- pushes ------------------------------------------------------------------------------------
  def _to_bank(self, eeg, target):
    """One session's [n, c] rows as [1, n, c]; a target [n] / [S, n] of one output as [S, n, 1]."""
    if len(eeg.shape) == 2 and self.sessions == 1:
      eeg = eeg.reshape((1,) + tuple(eeg.shape))
      if len(target.shape) <= 2:
        target = target.reshape((1,) + tuple(target.shape))       # [1, n] or [1, n, d]
    if len(target.shape) == 2 and self.outputs == 1:
      target = target.reshape(tuple(target.shape) + (1,))         # [S, n] -> [S, n, 1]
    return eeg, target

  def push(self, eeg, target):
    """The next n rows of every session: eeg [n, c] / [S, n, c] and target [n] / [n, d] / [S, n, d], float32 device
    tensors (read where they are, no host copy) or arrays; n may be 0.  Returns the frames counted so far."""
    return self._push((eeg, target), False)

  def flush(self, eeg=None, target=None):
    """The end of the recording: the last post_context frames are counted as if zero rows followed -- behind the
    recording's last rows, when they are given (one launch for both).  After it the fit refuses pushes until
    reset(); moments() and solve() stay."""
    return self._push((eeg, target), True)

  # -- what the state holds ----------------------------------------------------------------------
  def moments(self):
    """(xtx [S, K + 1, K + 1], xty [S, K + 1, d]) float64, dense and symmetric, the ones row / column last -- the
    layout of LagStats.moments.  Device tensors on the device, else host arrays."""
    if self._dev is None:
      return np.stack([sess.a for sess in self._host]), np.stack([sess.b for sess in self._host])
    return device.online_fit_moments(self._dev['state'], self.channels, self.pre, self.post, self.outputs,
                                     handle=self._dev['h'])

  def solve(self, lambdas):
    """Ridge weights from the moments so far, for every session and every lambda: (W [S, n_lambda, K, d],
    b [S, n_lambda, d]) -- the solution of (A / A[K][K] + lambda I) [W; b] = B / A[K][K], the reference's
    cov_x with lambda on the bias entry too (brain_model.py:447-455, 477).  float32 device tensors on the device
    (built and solved there: td_fit_online_solve), else host arrays (float64, as every NumPy session: not rounded
    to float32).  ValueError before any frame was counted; numpy.linalg.LinAlgError for a system that is not
    positive definite."""
    lambdas = [float(v) for v in np.atleast_1d(lambdas)]
    if not lambdas:
      raise ValueError('OnlineRidgeFit.solve needs at least one lambda.')
    if self.frames <= 0:
      raise ValueError('OnlineRidgeFit.solve: no frame counted yet (%d rows pushed, results run %d behind): the '
                       'moments are empty.' % (self.rows_pushed, self.delay))
    if self._dev is None:
      outs = [sess.solve(lambdas) for sess in self._host]
      return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return device.online_fit_solve(self._dev['state'], self.channels, self.pre, self.post, self.outputs,
                                   self.frames, lambdas, handle=self._dev['h'])

  def update_model(self, model, regularization_lambda, session=0):
    """Gives a brain_model.BrainModelLinearRegression the ridge weights of one session (model.set_weights): the
    model's channels, context and output width must be the session's.  Returns the model."""
    i = self._check_model(model, brain_model.BrainModelLinearRegression, (
        ('channels', self.channels, '_c1'), ('pre_context', self.pre, '_pre'), ('post_context', self.post, '_post'),
        ('outputs', self.outputs, '_output_width')), session)
    w, b = self.solve([regularization_lambda])
    w, b = w[i, 0], b[i, 0]
    if hasattr(w, 'cpu'):
      w, b = w.cpu().numpy(), b.cpu().numpy()
    model.set_weights([w, b])
    return model


# ------------------------------------------------------------------------------------------------ the online CCA fit
CCAFitResult = collections.namedtuple('CCAFitResult', ['rot_x', 'rot_y', 'mean_x', 'mean_y', 'e', 'corr'])

CCA_EPS_EIG = 1e-12                        # the reference's eigenvalue filter (cca.py:349-355)


def _check_ccafit_shape(who, c1, pre1, post1, c2, pre2, post2, g):
  """td_ccafit_online_push's limits, refused by name (the device call repeats them)."""
  if not 1 <= c1 <= device.ONLINE_CCAFIT_MAX_CHANNELS:
    raise ValueError('%s takes 1 to %d channels, not %d.' % (who, device.ONLINE_CCAFIT_MAX_CHANNELS, c1))
  if not 1 <= c2 <= device.ONLINE_CCAFIT_MAX_FEATURES:
    raise ValueError('%s takes 1 to %d features, not %d.' % (who, device.ONLINE_CCAFIT_MAX_FEATURES, c2))
  for pre, post in ((pre1, post1), (pre2, post2)):
    if pre < 0 or post < 0 or pre + 1 + post > device.ONLINE_CCAFIT_MAX_LAGS:
      raise ValueError('%s takes at most %d lags in a view, not %d + 1 + %d.' %
                       (who, device.ONLINE_CCAFIT_MAX_LAGS, pre, post))
  k1, k2 = (pre1 + 1 + post1) * c1, (pre2 + 1 + post2) * c2
  if k1 + k2 > device.ONLINE_CCAFIT_MAX_K:
    raise ValueError('%s takes at most %d lagged inputs in the two views, not %d + %d = %d.' %
                     (who, device.ONLINE_CCAFIT_MAX_K, k1, k2, k1 + k2))
  if not 0.0 < g <= 1.0:
    raise ValueError('%s takes a forgetting factor in (0, 1], not %r.' % (who, g))


def cca_model_from_moments(m, k1, k2, lam, dim, eps_eig=CCA_EPS_EIG):
  """The reference's CCA model (cca.py:337-362, as oracle/cca.py restates it) from the joint moments m [n, n] of
  u = [x~ | y~ | 1] in float64, for ONE minibatch that holds all counted frames: (rot_x [k1, dim], rot_y [k2, dim],
  mean_x [k1], mean_y [k2], e [dim]).  The covariances are symmetric, so the eigen-decompositions are eigh's."""
  n = k1 + k2 + 1
  count = m[n - 1, n - 1]
  mean = m[n - 1, :n - 1] / count
  mean_x, mean_y = mean[:k1], mean[k1:]
  denom = count - 1.0
  cov_xx = m[:k1, :k1] / denom - np.outer(mean_x, mean_x) + lam * np.eye(k1)
  cov_yy = m[k1:n - 1, k1:n - 1] / denom - np.outer(mean_y, mean_y) + lam * np.eye(k2)
  cov_xy = m[:k1, k1:n - 1] / denom - np.outer(mean_x, mean_y)

  def whitening(cov):
    vals, vecs = np.linalg.eigh(cov)
    keep = vals > eps_eig
    vals, vecs = vals[keep], vecs[:, keep]
    return (vecs * np.reciprocal(np.sqrt(vals))[None, :]) @ vecs.T

  k11, k22 = whitening(cov_xx), whitening(cov_yy)
  u, e, vt = np.linalg.svd((k11 @ cov_xy) @ k22, full_matrices=False)
  return k11 @ u[:, :dim], k22 @ vt.T[:, :dim], mean_x, mean_y, e[:dim]


def cca_fit_statistics(m, k1, k2, mean_x, rot_x, mean_y, rot_y):
  """corr [3, dim] = {mean_a, mean_b, power} of the projections (x~ - mean_x) rot_x and (y~ - mean_y) rot_y of the
  counted frames, in closed form from the joint moments: with mu = sums / count and C = S / count - mu mu^T,
  mean = (mu - mean_v) . R[:, d] and power[d] = sqrt((R_x[:, d]^T C_xx R_x[:, d]) (R_y[:, d]^T C_yy R_y[:, d])) --
  infer_decoder.Decoder._add_sums' {mean_x, mean_y, power}."""
  n = k1 + k2 + 1
  count = m[n - 1, n - 1]
  mu = m[n - 1, :n - 1] / count
  out = []
  quad = []
  for lo, hi, mean, rot in ((0, k1, mean_x, rot_x), (k1, n - 1, mean_y, rot_y)):
    rot = np.asarray(rot, np.float64)
    out.append((mu[lo:hi] - np.asarray(mean, np.float64).reshape(-1)) @ rot)
    mr = mu[lo:hi] @ rot
    quad.append(np.einsum('id,ij,jd->d', rot, m[lo:hi, lo:hi], rot) / count - mr * mr)
  return np.stack([out[0], out[1], np.sqrt(quad[0] * quad[1])])


class _HostCCAFitSession(object):
  """One online CCA fit session in NumPy: the semantics of td_ccafit_online_push bit for bit -- float32 rows, float64
  moments, one M * g + outer(u, u) per emitted frame in frame order -- and the reference's model in float64 NumPy
  (cca_model_from_moments)."""

  def __init__(self, c1, pre1, post1, c2, pre2, post2, g):
    self.v1, self.v2, self.g = (c1, pre1, post1), (c2, pre2, post2), float(g)
    self.post = max(post1, post2)
    self.k1, self.k2 = (pre1 + 1 + post1) * c1, (pre2 + 1 + post2) * c2
    self.reset()

  def reset(self):
    n = self.k1 + self.k2 + 1
    self.m = np.zeros((n, n), np.float64)
    self.tail = np.zeros((self.v1[1] + self.post, self.v1[0]), np.float32)
    self.feat_tail = np.zeros((self.v2[1] + self.post, self.v2[0]), np.float32)

  def push(self, eeg, feat, frames_before, flush):
    """eeg [n, c1], feat [n, c2] float32 behind frames_before rows; returns the frames this push emitted."""
    (_, pre1, post1), (_, pre2, post2) = self.v1, self.v2
    # rows[0] is EEG row frames_before - (pre1 + post), frows[0] feature row frames_before - (pre2 + post); frame f
    # reads the rows f - pre_v .. f + post_v of its view: the slots i + (post - post_v) .. of i = f - frames_before + post
    rows, self.tail = _session_rows(self.tail, eeg, self.post, flush)
    frows, self.feat_tail = _session_rows(self.feat_tail, feat, self.post, flush)
    _, emitted, i0 = _session_frames(frames_before, eeg.shape[0], self.post, flush)
    lags1, lags2 = pre1 + 1 + post1, pre2 + 1 + post2
    k1, k2 = self.k1, self.k2
    u = np.ones((k1 + k2 + 1,), np.float64)
    for i in range(i0, i0 + emitted):
      u[:k1] = rows[i:i + lags1].reshape(-1)
      u[k1:k1 + k2] = frows[i:i + lags2].reshape(-1)
      self.m = self.m * self.g + np.outer(u, u)
    return emitted

  def moments(self):
    """(xtx [k1 + 1, k1 + 1] with the ones row and column last, x2tx2, xtx2, sum2): LagStats.moments' layout."""
    k1, n = self.k1, self.k1 + self.k2 + 1
    x = np.r_[np.arange(k1), n - 1]
    return (self.m[np.ix_(x, x)], self.m[k1:n - 1, k1:n - 1].copy(), self.m[:k1, k1:n - 1].copy(),
            self.m[k1:n - 1, n - 1].copy())

  def solve(self, lambdas, dim):
    """CCAFitResult's fields for this session, float64: rot_x [n_lambda, k1, dim], ..., corr [n_lambda, 3, dim]."""
    outs = [cca_model_from_moments(self.m, self.k1, self.k2, lam, dim) for lam in lambdas]
    corr = [cca_fit_statistics(self.m, self.k1, self.k2, o[2], o[0], o[3], o[1]) for o in outs]
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), outs[0][2], outs[0][3],
            np.stack([o[4] for o in outs]), np.stack(corr))


class OnlineCCAFit(_FitBank):
  """The online CCA decoder's training stage: a bank of S sessions that take (eeg, attended features) rows in pushes
  of any length and keep the EXACT float64 moments of both lagged views -- M = sum u u^T of u = [x~ | y~ | 1], each
  half the lagged vector of brain_data's context for its view -- in ONE td_ccafit_online_push launch per push, the
  state on the device.  Any cut of a recording gives the same bytes.  `solve(lambdas, dims)` turns the moments into
  the reference's CCA model on the device, through the dense stage of the batch fit (cca.py:337-362 for one minibatch
  that holds all counted frames), with the fitted stretch's correlation statistics in closed form, and
  `OnlineDecoder.set_cca_model` takes both without a host copy:

      fit = OnlineCCAFit(64, 0, 20, features=8, input2_pre_context=0, input2_post_context=15)
      for eeg, attended in calibration_chunks:            # [n, 64] and [n, 8] float32, any n
        fit.push(eeg, attended)
      r = fit.solve([1.0], dims=5)                         # device tensors
      decoder.set_cca_model(r.mean_x, r.rot_x[:, 0], r.mean_y, r.rot_y[:, 0], corr=r.corr[:, 0])

  A frame needs max(post_context, input2_post_context) rows of the future, so the moments run `delay` frames behind
  the input; flush() ends the recording (zero rows behind it in both views, like the batch route's padding) and
  counts the rest.  forgetting g in (0, 1]: every emitted frame first scales the moments by g; M[n - 1][n - 1] --
  the count the covariances divide by -- is then the effective frame count.

  Refused by name: more than 128 channels, more than 32 features, more than 64 lags in a view, more than 2048
  lagged inputs in the two views, a push of more than 1048576 rows, a forgetting factor outside (0, 1].  Without a
  GPU the same object runs a NumPy session of the same semantics, bit for bit for the moments (float64 NumPy for the
  model, not rounded to float32)."""
  LAST_ROWS = 'OnlineCCAFit.flush takes the last rows as eeg AND feat, or neither.'
  SHAPES = ('A push is eeg [%d, n, %d] (or [n, %d] for one session) with features [%d, n, %d] (or [n, %d] for one '
            'session), not eeg %s with features %s.')

  def __init__(self, channels, pre_context, post_context, features, input2_pre_context, input2_post_context,
               num_sessions=1, forgetting=1.0):
    c1, pre1, post1 = int(channels), int(pre_context), int(post_context)
    c2, pre2, post2 = int(features), int(input2_pre_context), int(input2_post_context)
    g = float(forgetting)
    _check_ccafit_shape('OnlineCCAFit', c1, pre1, post1, c2, pre2, post2, g)
    self.channels, self.pre, self.post = c1, pre1, post1
    self.features, self.pre2, self.post2 = c2, pre2, post2
    self.inputs, self.inputs2 = (pre1 + 1 + post1) * c1, (pre2 + 1 + post2) * c2       # k1, k2
    self._views = views = (c1, pre1, post1, c2, pre2, post2)
    delay, n = max(post1, post2), self.inputs + self.inputs2 + 1
    self._setup(num_sessions, g, delay, (c1, c2), n * n,
                (('tail', pre1 + delay, c1), ('feat_tail', pre2 + delay, c2)),
                lambda: device.online_ccafit_state_bytes(*views),
                lambda: _HostCCAFitSession(*views, g),
                lambda *args, **kwargs: device.online_ccafit_push(*args, pre1, post1, pre2, post2, c1=c1, c2=c2,
                                                                  **kwargs))

  # -- pushes ------------------------------------------------------------------------------------
  def push(self, eeg, feat):
    """The next n rows of every session: eeg [n, c1] / [S, n, c1] and the attended speaker's features [n, c2] /
    [S, n, c2], float32 device tensors (read where they are, no host copy) or arrays; n may be 0.  Returns the
    frames counted so far."""
    return self._push((eeg, feat), False)

  def flush(self, eeg=None, feat=None):
    """The end of the recording: the last `delay` frames are counted as if zero rows followed in both views -- behind
    the recording's last rows, when they are given (one launch for both).  After it the fit refuses pushes until
    reset(); moments() and solve() stay."""
    return self._push((eeg, feat), True)

  # -- what the state holds ----------------------------------------------------------------------
  def moments(self):
    """(xtx [S, k1 + 1, k1 + 1], x2tx2 [S, k2, k2], xtx2 [S, k1, k2], sum2 [S, k2]) float64, dense and symmetric, the
    ones row / column of xtx last -- the layout of LagStats.moments; xtx[:, k1, k1] is the (effective) frame count.
    Device tensors on the device, else host arrays."""
    if self._dev is None:
      per = [sess.moments() for sess in self._host]
      return tuple(np.stack([p[i] for p in per]) for i in range(4))
    return device.online_ccafit_moments(self._dev['state'], *self._views, handle=self._dev['h'])

  def _check_solve(self, who, lambdas, dims):
    lambdas = [float(v) for v in np.atleast_1d(lambdas)]
    dims = int(dims)
    if not lambdas:
      raise ValueError('%s needs at least one lambda.' % who)
    if any(not lam >= 0.0 or not np.isfinite(lam) for lam in lambdas):
      raise ValueError('%s: regularization lambda must be >= 0, not %s.' % (who, lambdas))
    most = min(device.ONLINE_CCAFIT_MAX_DIMS, self.inputs, self.inputs2)
    if not 1 <= dims <= most:
      raise ValueError('%s: dims must be in [1, %d], not %d.' % (who, most, dims))
    if self.frames < 2:
      raise ValueError('%s: %d frames counted yet (%d rows pushed, results run %d behind): the covariance needs at '
                       'least 2.' % (who, self.frames, self.rows_pushed, self.delay))
    return lambdas, dims

  def solve(self, lambdas, dims, want_info=False):
    """The CCA model from the moments so far, for every session and every lambda: CCAFitResult(rot_x [S, n_lambda,
    k1, dims], rot_y [S, n_lambda, k2, dims], mean_x [S, k1], mean_y [S, k2], e [S, n_lambda, dims] -- the canonical
    correlations --, corr [S, n_lambda, 3, dims] float64 {mean_a, mean_b, power} of the counted frames' projections,
    what OnlineDecoder.set_cca_model takes).  float32 device tensors on the device (td_ccafit_online_solve: one
    dense stage per (session, lambda), synchronous), else host arrays (float64, as every NumPy session: not rounded
    to float32).  want_info: (result, info [S, n_lambda, 4]) -- td_cca_solve's sweeps and route bits (zeros on the
    host).  ValueError before 2 frames were counted."""
    lambdas, dims = self._check_solve('OnlineCCAFit.solve', lambdas, dims)
    if self._dev is None:
      outs = [sess.solve(lambdas, dims) for sess in self._host]
      result = CCAFitResult(*(np.stack([o[i] for o in outs]) for i in range(6)))
      info = np.zeros((self.sessions, len(lambdas), 4), np.int32)
    else:
      out = device.online_ccafit_solve(self._dev['state'], *self._views, self.frames, lambdas, dims,
                                       eps_eig=CCA_EPS_EIG, handle=self._dev['h'])
      result, info = CCAFitResult(*out[:6]), out.info
    return (result, info) if want_info else result

  def update_model(self, model, regularization, dims, session=0):
    """Gives a cca.BrainModelCCA of matching widths the rotations and means of one session (model.set_weights, and
    model.eigenvalues): the model's two input widths must be k1 and k2, its output_dims `dims`.  Returns the model."""
    from telluride_decoding_amd import cca
    i = self._check_model(model, cca.BrainModelCCA, (
        ('input_1 width', self.inputs, '_input1_width'), ('input_2 width', self.inputs2, '_input2_width'),
        ('output dims', int(dims), 'output_dims')), session)
    r = self.solve([regularization], dims)
    host = lambda a: (a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)).astype(np.float32)
    model.set_weights([host(r.mean_x[i]).reshape(1, -1), host(r.mean_y[i]).reshape(1, -1), host(r.rot_x[i, 0]),
                       host(r.rot_y[i, 0])])
    model.eigenvalues = host(r.e[i, 0])
    return model


# ------------------------------------------------------------------------------------------------ the online calibration
CalibrationResult =collections.namedtuple('CalibrationResult', ['corr', 'lda', 'dprime'])

CALIB_SUMS = device.ONLINE_CALIB_SUMS      # TD_CALIB_ONLINE_SUMS
_CALIB_REASONS = {
    device.CALIB_NO_WINDOW: 'No data for class 0: no window of %(width)d frames is complete after %(frames)d frames',
    device.CALIB_NO_POWER: 'the correlation power is not finite or not above zero (a constant prediction or constant '
                           'envelopes)',
    device.CALIB_SAME_MEANS: 'X0 and X1 in Scaled LDA are identical: the attended and the unattended window means '
                             'are equal',
}


def calibration_walk(sums, pred, attended, unattended, first_frame, width):
  """Advances one session's CALIB_SUMS float64 sums (td_calib_online_push's layout) in place by the emitted frames
  first_frame, first_frame + 1, ...: every sum in frame order, acc += x * y in float64; when a frame completes a
  window the classes' sum z take plain adds, their Grams G + z_i * z_j, and the open window returns to zero."""
  for i in range(len(pred)):
    p, a, u = float(pred[i]), float(attended[i]), float(unattended[i])
    for at, term in ((0, p), (1, p * p), (2, a), (3, a * a), (4, u), (5, u * u),
                     (24, p), (25, a), (26, a * p), (27, u), (28, u * p)):
      sums[at] = sums[at] + term
    if (first_frame + i + 1) % width == 0:
      for base, z in ((6, (sums[28], sums[27], sums[24])), (15, (sums[26], sums[25], sums[24]))):
        at = base + 3
        for j in range(3):
          sums[base + j] = sums[base + j] + z[j]
          for k in range(j, 3):
            sums[at] = sums[at] + z[j] * z[k]
            at += 1
      sums[24:29] = 0.0


def calibration_closed_form(sums, frames, width):
  """td_calib_online_finish for one session in NumPy float64: dict(status, count, sum_x, sum_y, sum_x2, sum_y2,
  mean_x, mean_y, power, class_means (mbar_0, mbar_1), class_variances, slope, intercept, dprime) from the
  CALIB_SUMS sums after `frames` emitted frames."""
  q = np.asarray(sums, np.float64)
  out = dict(status=device.CALIB_OK, slope=np.nan, intercept=np.nan, dprime=np.nan, class_means=(np.nan, np.nan),
             class_variances=(np.nan, np.nan))
  with np.errstate(all='ignore'):
    count = np.float64(2.0 * frames)
    sum_x, sum_x2, sum_y, sum_y2 = q[4] + q[2], q[5] + q[3], q[0] + q[0], q[1] + q[1]
    mean_x, mean_y = sum_x / count, sum_y / count
    power = np.sqrt((sum_x2 - sum_x * sum_x / count) * (sum_y2 - sum_y * sum_y / count)) / count
    out.update(count=int(2 * frames), sum_x=sum_x, sum_y=sum_y, sum_x2=sum_x2, sum_y2=sum_y2, mean_x=mean_x,
               mean_y=mean_y, power=power)
    n_win = float(int(frames) // int(width))
    if n_win < 1.0:
      out.update(status=device.CALIB_NO_WINDOW, mean_x=np.nan, mean_y=np.nan, power=np.nan)
      return out
    if not power > 0.0 or np.isinf(power):
      out.update(status=device.CALIB_NO_POWER, mean_x=np.nan, mean_y=np.nan, power=np.nan)
      return out
    scale = 1.0 / (float(width) * power)
    cv = np.array([scale, -mean_y * scale, -mean_x * scale])
    c0 = mean_x * mean_y / power
    means, variances = [], []
    for base in (6, 15):
      z, g = q[base:base + 3], q[base + 3:base + 9]
      cz = (cv[0] * z[0] + cv[1] * z[1]) + cv[2] * z[2]
      quad = ((g[0] * cv[0] * cv[0] + g[3] * cv[1] * cv[1]) + g[5] * cv[2] * cv[2]) + \
          2.0 * ((g[1] * cv[0] * cv[1] + g[2] * cv[0] * cv[2]) + g[4] * cv[1] * cv[2])
      sm, sm2 = cz + n_win * c0, (quad + 2.0 * c0 * cz) + n_win * c0 * c0
      means.append(sm / n_win)
      variances.append(sm2 / n_win - means[-1] * means[-1])
    out.update(class_means=tuple(means), class_variances=tuple(variances))
    if means[0] == means[1] or np.isnan(means[0]) or np.isnan(means[1]):
      out.update(status=device.CALIB_SAME_MEANS)
      return out
    slope = 1.0 / (means[1] - means[0])
    out.update(slope=slope, intercept=-slope * means[0],
               dprime=abs(means[1] - means[0]) / np.sqrt((variances[0] + variances[1]) / 2.0))
  return out


class _HostCalibSession(object):
  """One online calibration session in NumPy: the semantics of td_calib_online_push with a float64 prediction (as
  _HostSession predicts), the sums of calibration_walk."""

  def __init__(self, c, pre, post, width):
    self.c, self.pre, self.post, self.width = c, pre, post, width
    self.reset()

  def reset(self):
    self.sums = np.zeros((CALIB_SUMS,), np.float64)
    self.tail = np.zeros((self.pre + self.post, self.c), np.float64)
    self.env_tail = np.zeros((self.post, 2), np.float64)

  def push(self, eeg, env, w, b, frames_before, flush):
    """eeg [n, c], env [n, 2] float64 behind frames_before rows, predicted with w [lags c] and b."""
    c, pre, post = self.c, self.pre, self.post
    rows, self.tail = _session_rows(self.tail, eeg, post, flush)
    envs, self.env_tail = _session_rows(self.env_tail, env, post, False)
    first, emitted, i0 = _session_frames(frames_before, eeg.shape[0], post, flush)
    w = np.asarray(w, np.float32).astype(np.float64)
    pred = np.zeros((emitted,), np.float64)
    for l in range(pre + 1 + post):                 # (lag, channel) order, whatever the push's length
      for ch in range(c):
        pred += rows[i0 + l:i0 + l + emitted, ch] * w[l * c + ch]
    pred = pred + float(b)
    truth = envs[i0:i0 + emitted]
    calibration_walk(self.sums, pred, truth[:, 0], truth[:, 1], first, self.width)
    return emitted


class _CalibrationBank(_TrainingBank):
  """What the three calibration banks share: an OnlineDecoder bank of one kind whose sessions, context and current
  model they take, windows of window_size frames, sums in float64 at the head of the state, and a closed form over
  them with a status per session.  A class gives BANK (the decoder's kind, its words for it, whose the other kinds
  are), REASONS (status -> sentence), _reason_values() beyond width and frames, _closed_form(sums) and
  _host_result(outs), and _device_finish()."""
  FLUSHED = 'The calibration was flushed: reset() starts the next stretch.'
  BANK = REASONS = None

  def _take(self, decoder, window_size):
    """The constructor's refusals, and what every calibration takes from its decoder."""
    who, (kind, words, others) = type(self).__name__, self.BANK
    if not isinstance(decoder, OnlineDecoder):
      raise ValueError('%s calibrates an OnlineDecoder bank, not a %s.' % (who, type(decoder).__name__))
    if decoder.kind != kind:
      raise ValueError('%s calibrates %s, not a %s bank (%s).' % (who, words, decoder.kind, others))
    width = max(1, int(window_size))
    if width > MAX_WINDOW:
      raise ValueError('%s takes windows of 1 to %d frames, not %d.' % (who, MAX_WINDOW, width))
    self.decoder, self.window_size = decoder, width
    self.channels, self.pre, self.post = decoder.channels, decoder.pre, decoder.post

  def _allocate(self, delay, state_bytes, host_session):
    decoder = self.decoder
    _TrainingBank.__init__(self, decoder.sessions, decoder._on_device, delay, lambda: decoder._dev['h'], state_bytes,
                           host_session)

  frames_emitted = _TrainingBank._counted        # the frames counted into the sums so far

  @property
  def windows(self):
    """The completed windows per class."""
    return self.frames_emitted // self.window_size

  def _reason_values(self):
    return {}

  def _raise(self, status):
    for i, st in enumerate(status):
      if int(st) != device.CALIB_OK:
        reason = self.REASONS[int(st)] % dict(self._reason_values(), width=self.window_size,
                                              frames=self.frames_emitted)
        raise ValueError('%s.finish: session %d: %s.' % (type(self).__name__, i, reason))

  def _finish(self):
    """finish(): the closed form of every session, refused by _raise unless every status is CALIB_OK."""
    if self._dev is None:
      outs = [self._closed_form(sess.sums) for sess in self._host]
      self._raise([o['status'] for o in outs])
      return self._host_result(outs)
    out = self._device_finish()
    self._raise(out.status.cpu().numpy())
    return CalibrationResult(out.corr, out.lda, out.dprime)

  def _session_form(self, decoder, kind, session):
    """The front of update_decoder: the closed form (a dict) of one session's sums for a decoder of class `kind`."""
    who = '%s.update_decoder' % type(self).__name__
    if not isinstance(decoder, kind):
      raise ValueError('%s takes a %s, not a %s.' % (who, kind.__name__, type(decoder).__name__))
    if not 0 <= int(session) < self.sessions:
      raise ValueError('%s: session %d of %d.' % (who, int(session), self.sessions))
    sums = self.sums()[int(session)]
    if hasattr(sums, 'cpu'):
      sums = sums.cpu().numpy()
    o = self._closed_form(sums)
    if o['status'] != device.CALIB_OK:
      status = [device.CALIB_OK] * self.sessions
      status[int(session)] = o['status']
      self._raise(status)
    return o


class _EnvelopeCalibration(_CalibrationBank):
  """What OnlineCalibration and OnlineDNNCalibration share -- everything but the prediction: pushes of (eeg, attended
  envelope, unattended envelope) rows, td_calib_online_push's state block, whose 29 sums td_calib_online_sums reads
  and td_calib_online_finish closes, and the LinearRegressionDecoder that takes the result.  A class gives LAST_ROWS,
  BANK, its constructor, _session_push and _device_push."""
  REASONS = _CALIB_REASONS

  # -- pushes ------------------------------------------------------------------------------------
  def push(self, eeg, attended, unattended):
    """The next n rows of every session: eeg [n, C] / [S, n, C], the attended and the unattended envelope [n] /
    [S, n], float32 device tensors (read where they are) or arrays; n may be 0.  Returns the frames counted so
    far."""
    return self._push((eeg, attended, unattended), False)

  def flush(self, eeg=None, attended=None, unattended=None):
    """The end of the stretch: the last post_context frames are counted as if zero rows followed -- behind the
    stretch's last rows, when they are given (one launch for both).  After it the calibration refuses pushes until
    reset(); sums() and finish() stay."""
    return self._push((eeg, attended, unattended), True)

  def _blocks(self, eeg, attended, unattended):
    return self.decoder._as_bank(eeg, attended, unattended)

  def _no_blocks(self):
    return self._no_rows(self.channels), self._no_rows(2)

  def _device_rows(self, blocks):
    """(eeg, env) of a device push as device tensors; (None, None) without rows."""
    eeg, env = blocks or (None, None)
    if blocks is not None and not hasattr(eeg, 'is_cuda'):
      eeg, env = self._upload(self._dev['h'], eeg), self._upload(self._dev['h'], env)
    return eeg, env

  # -- what the state holds ----------------------------------------------------------------------
  def sums(self):
    """[S, 29] float64, td_calib_online_sums' order: sum p, p^2, a, a^2, u, u^2 over every counted frame (p the
    prediction, a / u the attended / unattended envelope) | class 0 (unattended): sum_w z [3] and the upper triangle
    of sum_w z z^T [6], z = a window's (sum x p, sum x, sum p) | class 1 (attended) | the open window's sum p, a,
    a p, u, u p.  A device tensor on the device, else a host array."""
    if self._dev is None:
      return np.stack([sess.sums for sess in self._host])
    return device.online_calib_sums(self._dev['state'], handle=self._dev['h'])

  def _closed_form(self, sums):
    return calibration_closed_form(sums, self.frames_emitted, self.window_size)

  def _host_result(self, outs):
    stats = [[o['mean_x'], o['mean_y'], o['power']] for o in outs]
    return CalibrationResult(np.array([[st, st] for st in stats], np.float64),
                             np.array([[1.0, o['slope'], o['intercept']] for o in outs], np.float64),
                             np.array([o['dprime'] for o in outs], np.float64))

  def _device_finish(self):
    return device.online_calib_finish(self._dev['state'], self.frames_emitted, self.window_size,
                                      handle=self._dev['h'])

  def finish(self):
    """CalibrationResult(corr [S, 2, 3] {mean_truth, mean_pred, power} for both speakers, lda [S, 3] {1, slope,
    intercept}, dprime [S]) float64 from the sums so far -- what OnlineDecoder.set_statistics takes; device tensors
    on the device (one launch; the statuses come back in one small copy), else host arrays.  The state is not
    modified.  ValueError naming the session and the reason: no completed window (train's 'No data for class'), a
    power that is not finite or not above zero, equal class means (scaled LDA's 'X0 and X1 ... identical')."""
    return self._finish()

  def update_decoder(self, decoder, session=0):
    """Gives an infer_decoder.LinearRegressionDecoder the correlation parameters and the scaled LDA of one session
    (what Decoder.train leaves in it), so that save_parameters writes them.  Returns d'."""
    from telluride_decoding_amd import scaled_lda
    o = self._session_form(decoder, infer_decoder.LinearRegressionDecoder, session)
    vec = lambda v: np.array([v], np.float64)
    decoder.model_params = infer_decoder.ModelParamsTuple(
        infer_decoder.CorrelationParamsTuple(o['count'], vec(o['sum_x']), vec(o['sum_y']), vec(o['sum_x2']),
                                             vec(o['sum_y2']), vec(o['mean_x']), vec(o['mean_y']), vec(o['power'])),
        scaled_lda.LdaParamsTuple(np.ones((1, 1)), np.zeros((1, 1)), [1, 2],
                                  [vec(o['class_means'][0]), vec(o['class_means'][1])], float(o['slope']),
                                  float(o['intercept'])))
    return float(o['dprime'])


class OnlineCalibration(_EnvelopeCalibration):
  """The online chain's last training stage: the correlation statistics, the scaled LDA and d' that
  infer_decoder.Decoder.train(data0, data1, window_size=W) would take from a labelled stretch -- data0 the
  (unattended envelope, prediction) frames, data1 the (attended envelope, prediction) frames -- for rows that arrive
  in pushes of any length, predicted with the bank's CURRENT weights, in ONE td_calib_online_push launch per push and
  with nothing stored per row:

      fit.push(eeg, att); w, b = fit.solve([lam]); decoder.set_weights(w[:, 0, :, 0], b[:, 0, 0])
      calib = OnlineCalibration(decoder, window_size=100)
      for eeg, att, unatt in calibration_chunks:         # [n, C], [n], [n] float32, any n
        calib.push(eeg, att, unatt)
      r = calib.finish()                                 # CalibrationResult(corr, lda, dprime), on the device
      decoder.set_statistics(r.corr, r.lda)              # device to device

  decoder: a linear OnlineDecoder bank; the sessions, the channels and the context are the bank's, and every push
  reads the bank's weights where they are, so the calibrator follows set_weights.  window_size: the frames averaged
  into one training point of the LDA (decoding.train_lda_model's correlation_frames, default 100; <= 1: every
  frame).  Windows are infer_decoder.average_data's: consecutive, the tail dropped.  A frame needs post_context rows
  of future EEG, so the sums run that far behind the input; flush() ends the recording.  finish() can be called at
  any time and leaves the state alone.  Any cut of a recording gives the same state bytes (sums()).

  Without a GPU the same object runs a NumPy session of the same semantics (float64 prediction)."""
  LAST_ROWS = 'OnlineCalibration.flush takes the last rows as eeg AND both envelopes, or nothing.'
  BANK = ('linear', 'a linear bank', 'OnlineCCACalibration and OnlineDNNCalibration are the other banks\'')

  def __init__(self, decoder, window_size=100):
    self._take(decoder, window_size)
    shape = (self.channels, self.pre, self.post)
    self._allocate(self.post, lambda: device.online_calib_state_bytes(*shape),
                   lambda: _HostCalibSession(*shape, self.window_size))

  def _session_push(self, sess, i, blocks, flush):
    p = self.decoder._params[i]
    sess.push(np.asarray(blocks[0][i], np.float64), np.asarray(blocks[1][i], np.float64), p['w'], p['b'],
              self.rows_pushed, flush)

  def _device_push(self, blocks, flush):
    d, bank = self._dev, self.decoder._dev
    eeg, env = self._device_rows(blocks)
    device.online_calib_push(eeg, env, bank['w'], bank['b'], d['state'], self.rows_pushed, self.pre, self.post,
                             self.window_size, c=self.channels, flush=flush, handle=d['h'])


# ------------------------------------------------------------------------------------------ the online DNN calibration
class _HostDnnCalibSession(_HostCalibSession):
  """One online DNN calibration session in NumPy: the semantics of td_fccalib_online_push with a float64 prediction
  (_HostDnnSession._predict's), the sums of calibration_walk."""

  def push(self, eeg, env, params, frames_before, flush):
    """eeg [n, c], env [n, 2] float64 behind frames_before rows, predicted with the session parameters `params`
    (dnn_session_parameters: its weights)."""
    post = self.post
    rows, self.tail = _session_rows(self.tail, eeg, post, flush)
    envs, self.env_tail = _session_rows(self.env_tail, env, post, False)
    first, emitted, i0 = _session_frames(frames_before, eeg.shape[0], post, flush)
    self.p = params                                  # (what _predict reads: c, pre, post, weights)
    pred = _HostDnnSession._predict(self, rows, i0, emitted)
    truth = envs[i0:i0 + emitted]
    calibration_walk(self.sums, pred, truth[:, 0], truth[:, 1], first, self.width)
    return emitted


class OnlineDNNCalibration(_EnvelopeCalibration):
  """OnlineCalibration for a DNN bank: the correlation statistics, the scaled LDA and d' that
  infer_decoder.Decoder.train(data0, data1, window_size=W) would take from a labelled stretch, for rows that arrive in
  pushes of any length, predicted with the bank's network -- td_fc_online_push's prediction, bit for bit -- in ONE
  td_fccalib_online_push launch per push and with nothing stored per row.  A network trained offline on other
  sessions is so scored with the new listener's statistics, not the training set's:

      decoder = OnlineDecoder(dnn_decoder, window_size=500)   # a LinearRegressionDecoder around a BrainModelDNN
      calib = OnlineDNNCalibration(decoder, window_size=100)
      for eeg, att, unatt in calibration_chunks:         # [n, C], [n], [n] float32, any n
        calib.push(eeg, att, unatt)
      r = calib.finish()                                 # CalibrationResult(corr, lda, dprime), on the device
      decoder.set_statistics(r.corr, r.lda)              # device to device

  decoder: a DNN OnlineDecoder bank; the sessions, the channels, the context and the hidden layers are the bank's,
  and every push reads the bank's packed parameters where they are on the device.  window_size, the windows, the
  delay of post_context rows, flush(), sums(), finish() and update_decoder(): OnlineCalibration's -- the state block
  is td_calib_online_push's byte for byte, and td_calib_online_sums / td_calib_online_finish serve it.  Any cut of a
  recording gives the same state bytes.

  Without a GPU the same object runs a NumPy session of the same semantics (float64 prediction)."""
  LAST_ROWS = 'OnlineDNNCalibration.flush takes the last rows as eeg AND both envelopes, or nothing.'
  BANK = ('dnn', 'a DNN bank', 'OnlineCalibration is the linear bank\'s, OnlineCCACalibration the CCA bank\'s')

  def __init__(self, decoder, window_size=100):
    self._take(decoder, window_size)
    self.hidden = list(decoder.hidden)
    shape = (self.channels, self.pre, self.post)
    device.online_dnn_calib_lds_bytes(*shape, self.hidden, 1)   # (a shape over the LDS budget: refused by name)
    self._allocate(self.post, lambda: device.online_dnn_calib_state_bytes(*shape),
                   lambda: _HostDnnCalibSession(*shape, self.window_size))

  def _session_push(self, sess, i, blocks, flush):
    sess.push(np.asarray(blocks[0][i], np.float64), np.asarray(blocks[1][i], np.float64), self.decoder._params[i],
              self.rows_pushed, flush)

  def _device_push(self, blocks, flush):
    d, bank = self._dev, self.decoder._dev
    eeg, env = self._device_rows(blocks)
    device.online_dnn_calib_push(eeg, env, bank['params'], self.hidden, d['state'], self.rows_pushed, self.pre,
                                 self.post, self.window_size, flush=flush, handle=d['h'])


# ------------------------------------------------------------------------------------------ the online CCA calibration
_CCA_CALIB_REASONS = dict(_CALIB_REASONS)
_CCA_CALIB_REASONS[device.CALIB_NO_POWER] = ('the correlation power of a dim is not finite or not above zero (a '
                                             'constant projection)')
_CCA_CALIB_REASONS[device.CALIB_NOT_POSITIVE] = ('the pooled scatter of the window means is not positive definite '
                                                 '(%(windows)d windows per class for %(dims)d dims: at least '
                                                 'dims + 2 windows in all are needed)')
_CCA_CALIB_REASONS[device.CALIB_SAME_MEANS] = ('X0 and X1 in Scaled LDA are identical: the attended and the '
                                               'unattended window means are equal along the LDA axis')


def cca_calibration_layout(dims):
  """(entries of one class, offset of class 0, offset of the open window, T) of the float64 head of
  td_ccacalib_online_push's state for `dims` columns: [0, 6 dims) the correlator | class 0 | class 1 | the open
  window [5 dims]; a class is sum z [3 dims] then the row-major upper triangle of sum z z^T."""
  n3 = 3 * dims
  per_class = n3 + n3 * (n3 + 1) // 2
  return per_class, 6 * dims, 6 * dims + 2 * per_class, device.online_ccacalib_sums_count(dims)


def cca_calibration_walk(sums, a, b1, b0, first_frame, width):
  """Advances one session's float64 sums (td_ccacalib_online_push's layout) in place by the emitted frames
  first_frame, first_frame + 1, ... with the projections a, b1 (attended), b0 (unattended) [frames, dims]: every sum
  in frame order, acc += x * y in float64; when a frame completes a window each class's sum z takes plain adds, its
  Gram G + z_i * z_j, and the open window returns to zero."""
  a, b1, b0 = (np.asarray(v, np.float64) for v in (a, b1, b0))
  d = a.shape[1]
  per_class, class0, open0, _ = cca_calibration_layout(d)
  upper = np.triu_indices(3 * d)
  for i in range(a.shape[0]):
    x, y1, y0 = a[i], b1[i], b0[i]
    sums[:6 * d] = sums[:6 * d] + np.concatenate([x, x * x, y1, y1 * y1, y0, y0 * y0])
    sums[open0:] = sums[open0:] + np.concatenate([x, y1, x * y1, y0, x * y0])
    if (first_frame + i + 1) % width == 0:
      o = sums[open0:].reshape(5, d)
      for cls, z in ((0, np.concatenate([o[4], o[0], o[3]])), (1, np.concatenate([o[2], o[0], o[1]]))):
        base = class0 + cls * per_class
        sums[base:base + 3 * d] = sums[base:base + 3 * d] + z
        sums[base + 3 * d:base + per_class] = sums[base + 3 * d:base + per_class] + np.outer(z, z)[upper]
      sums[open0:] = 0.0


def cca_calibration_closed_form(sums, frames, width, dims):
  """td_ccacalib_online_finish for one session in NumPy float64: dict(status, count, sum_x, sum_y, sum_x2, sum_y2,
  mean_a, mean_b, power [dims each], class_means [2, dims], w [dims], slope, intercept, dprime) from the sums after
  `frames` emitted frames.  Scaled LDA on two classes without the eigenproblem: the between-class scatter has rank
  one, so the leading eigenvector of inv(Sw) Sb is Sw^-1 (mu_1 - mu_0) up to scale and sign, which slope and
  intercept remove."""
  q = np.asarray(sums, np.float64)
  d = int(dims)
  per_class, class0, _, _ = cca_calibration_layout(d)
  nans = np.full((d,), np.nan)
  out = dict(status=device.CALIB_OK, w=nans, slope=np.nan, intercept=np.nan, dprime=np.nan,
             class_means=np.full((2, d), np.nan))
  with np.errstate(all='ignore'):
    count = np.float64(2.0 * frames)
    s = q[:6 * d].reshape(6, d)
    sum_x, sum_x2, sum_y, sum_y2 = s[0] + s[0], s[1] + s[1], s[4] + s[2], s[5] + s[3]
    mean_a, mean_b = sum_x / count, sum_y / count
    power = np.sqrt((sum_x2 - sum_x * sum_x / count) * (sum_y2 - sum_y * sum_y / count)) / count
    out.update(count=int(2 * frames), sum_x=sum_x, sum_y=sum_y, sum_x2=sum_x2, sum_y2=sum_y2, mean_a=mean_a,
               mean_b=mean_b, power=power)
    n_win = float(int(frames) // int(width))
    if n_win < 1.0:
      out.update(status=device.CALIB_NO_WINDOW, mean_a=nans, mean_b=nans, power=nans)
      return out
    if not np.all(power > 0.0) or np.any(np.isinf(power)):
      out.update(status=device.CALIB_NO_POWER, mean_a=nans, mean_b=nans, power=nans)
      return out
    scale = 1.0 / (float(width) * power)
    c = np.zeros((d, 3 * d))
    at = np.arange(d)
    c[at, at], c[at, d + at], c[at, 2 * d + at] = scale, -mean_b * scale, -mean_a * scale
    c0 = mean_a * mean_b / power
    upper = np.triu_indices(3 * d)
    means, scatters = [], []
    for cls in (0, 1):
      base = class0 + cls * per_class
      g = np.zeros((3 * d, 3 * d))
      g[upper] = q[base + 3 * d:base + per_class]
      g = g + np.triu(g, 1).T
      cz = c @ q[base:base + 3 * d]
      smm = c @ g @ c.T + np.outer(cz, c0) + np.outer(c0, cz) + n_win * np.outer(c0, c0)
      mu = (cz + n_win * c0) / n_win
      means.append(mu)
      scatters.append(smm - n_win * np.outer(mu, mu))
    out.update(class_means=np.stack(means))
    within = scatters[0] + scatters[1]
    delta = means[1] - means[0]
    try:
      if 2.0 * n_win < d + 2.0 or not np.all(np.isfinite(within)):
        raise np.linalg.LinAlgError('fewer points than dims')
      factor = np.linalg.cholesky(within)
      if not np.all(np.isfinite(factor)):
        raise np.linalg.LinAlgError('not finite')
    except np.linalg.LinAlgError:
      out.update(status=device.CALIB_NOT_POSITIVE)
      return out
    v = np.linalg.solve(factor.T, np.linalg.solve(factor, delta))
    w = np.ones((1,)) if d == 1 else v / np.sqrt(np.sum(v * v))
    along = float(delta @ w)
    if along == 0.0 or np.isnan(along):
      out.update(status=device.CALIB_SAME_MEANS)
      return out
    slope = 1.0 / along
    spread = float(w @ scatters[0] @ w + w @ scatters[1] @ w)
    out.update(w=w, slope=slope, intercept=-slope * float(means[0] @ w),
               dprime=abs(along) / np.sqrt(spread / (2.0 * n_win)))
  return out


class _HostCCACalibSession(object):
  """One online CCA calibration session in NumPy: the semantics of td_ccacalib_online_push with float64 projections
  (as _HostCcaSession projects), the sums of cca_calibration_walk."""

  def __init__(self, c1, pre1, post1, c2, pre2, post2, dims, width):
    self.view1, self.view2, self.dims, self.width = (c1, pre1, post1), (c2, pre2, post2), dims, width
    self.delay = max(post1, post2)
    self.reset()

  def reset(self):
    (c1, pre1, _), (c2, pre2, _) = self.view1, self.view2
    self.sums = np.zeros((device.online_ccacalib_sums_count(self.dims),), np.float64)
    self.tail = np.zeros((pre1 + self.delay, c1), np.float64)
    self.feat_tail = np.zeros((2, pre2 + self.delay, c2), np.float64)

  def push(self, eeg, feat, model, frames_before, flush):
    """eeg [n, c1], feat [2, n, c2] (attended, unattended) float64 behind frames_before rows, projected with
    model's mean_x, rot_x, mean_y, rot_y."""
    (c1, pre1, post1), (c2, pre2, post2) = self.view1, self.view2
    rows, self.tail = _session_rows(self.tail, eeg, self.delay, flush)
    frows, self.feat_tail = _session_rows(self.feat_tail, feat, self.delay, flush, axis=1)
    first, emitted, i0 = _session_frames(frames_before, eeg.shape[0], self.delay, flush)
    f64 = lambda name: np.asarray(model[name], np.float32).astype(np.float64)
    project = _HostCcaSession._project
    a = project(rows, i0, emitted, c1, pre1 + 1 + post1, f64('mean_x'), f64('rot_x'))
    b1, b0 = (project(frows[k], i0, emitted, c2, pre2 + 1 + post2, f64('mean_y'), f64('rot_y')) for k in (0, 1))
    cca_calibration_walk(self.sums, a, b1, b0, first, self.width)
    return emitted


class OnlineCCACalibration(_CalibrationBank):
  """The CCA chain's last training stage: per dim the correlation statistics, the scaled LDA over the dims columns
  and d' that infer_decoder.Decoder.train(data0, data1, window_size=W) would take from a labelled stretch with a
  CCADecoder -- data0 the (EEG projection, unattended projection) frames, data1 the (EEG projection, attended
  projection) frames, ONE correlator fed both -- for rows that arrive in pushes of any length, projected with the
  bank's CURRENT model, in ONE td_ccacalib_online_push launch per push and with nothing stored per row:

      r = fit.solve([lam], dims); decoder.set_cca_model(r.mean_x, r.rot_x[:, 0], r.mean_y, r.rot_y[:, 0])
      calib = OnlineCCACalibration(decoder, window_size=100)
      for eeg, att, unatt in calibration_chunks:         # [n, C], [n, c2], [n, c2] float32, any n
        calib.push(eeg, att, unatt)
      c = calib.finish()                                 # CalibrationResult(corr, lda, dprime), on the device
      decoder.set_cca_statistics(c.corr, c.lda)          # device to device

  decoder: a CCA OnlineDecoder bank; the sessions, the two views and the dims are the bank's, and every push reads
  the bank's means and rotations where they are, so the calibrator follows set_cca_model.  window_size: the frames
  averaged into one training point of the LDA (default 100; <= 1: every frame).  Windows are
  infer_decoder.average_data's: consecutive, the tail dropped.  The sums run max(post_context, input2_post_context)
  rows behind the input; flush() ends the recording.  finish() can be called at any time and leaves the state alone.
  Any cut of a recording gives the same state bytes (sums()).  The LDA needs a positive definite pooled scatter: at
  least dims + 2 windows in all.

  Without a GPU the same object runs a NumPy session of the same semantics (float64 projections)."""
  LAST_ROWS = 'OnlineCCACalibration.flush takes the last rows as eeg AND both feature blocks, or nothing.'
  BANK = ('cca', 'a CCA bank', 'OnlineCalibration is the linear bank\'s, OnlineDNNCalibration the DNN bank\'s')
  REASONS = _CCA_CALIB_REASONS

  def __init__(self, decoder, window_size=100):
    self._take(decoder, window_size)
    self.features, self.pre2, self.post2, self.dims = decoder.features, decoder.pre2, decoder.post2, decoder.dims
    shape = (self.channels, self.pre, self.post, self.features, self.pre2, self.post2, self.dims)
    if self.decoder._on_device:
      device.online_ccacalib_lds_bytes(*shape, 1)      # (a shape over the LDS budget: the library says so, by name)
    self._allocate(decoder.delay, lambda: device.online_ccacalib_state_bytes(*shape),
                   lambda: _HostCCACalibSession(*shape, self.window_size))

  # -- pushes ------------------------------------------------------------------------------------
  def push(self, eeg, attended_features, unattended_features):
    """The next n rows of every session: eeg [n, C] / [S, n, C], the attended and the unattended speaker's feature
    block [n, c2] / [S, n, c2], float32 device tensors (read where they are) or arrays; n may be 0.  Returns the
    frames counted so far."""
    return self._push((eeg, attended_features, unattended_features), False)

  def flush(self, eeg=None, attended_features=None, unattended_features=None):
    """The end of the stretch: the last `delay` frames are counted as if zero rows followed -- behind the stretch's
    last rows, when they are given (one launch for both).  After it the calibration refuses pushes until reset();
    sums() and finish() stay."""
    return self._push((eeg, attended_features, unattended_features), True)

  def _blocks(self, eeg, attended, unattended):
    return self.decoder._as_cca_bank(eeg, attended, unattended)

  def _no_blocks(self):
    return self._no_rows(self.channels), (self._no_rows(self.features),) * 2

  def _session_push(self, sess, i, blocks, flush):
    sess.push(np.asarray(blocks[0][i], np.float64), np.stack([np.asarray(f[i], np.float64) for f in blocks[1]]),
              self.decoder._params[i], self.rows_pushed, flush)

  def _device_push(self, blocks, flush):
    d, bank = self._dev, self.decoder._dev
    eeg = att = unatt = None
    if blocks is not None:
      eeg, att, unatt = (a if hasattr(a, 'is_cuda') else self._upload(d['h'], a) for a in (blocks[0],) + blocks[1])
    device.online_ccacalib_push(eeg, att, unatt, bank['mean_x'], bank['rot_x'], bank['mean_y'], bank['rot_y'],
                                d['state'], self.rows_pushed, self.pre, self.post, self.pre2, self.post2,
                                self.window_size, flush=flush, handle=d['h'])

  # -- what the state holds ----------------------------------------------------------------------
  def sums(self):
    """[S, 9 dims^2 + 20 dims] float64, td_ccacalib_online_sums' order (cca_calibration_layout): sum a, a^2, b1, b1^2,
    b0, b0^2 over every counted frame, [dims] each (a the EEG view's projection, b1 / b0 the attended / unattended
    speaker's) | class 0 (unattended): sum_w z [3 dims] and the upper triangle of sum_w z z^T, z = a window's
    (sum a b | sum a | sum b) | class 1 (attended) | the open window's sum a, b1, a b1, b0, a b0.  A device tensor on
    the device, else a host array."""
    if self._dev is None:
      return np.stack([sess.sums for sess in self._host])
    return device.online_ccacalib_sums(self._dev['state'], self.dims, handle=self._dev['h'])

  def _reason_values(self):
    return dict(windows=self.windows, dims=self.dims)

  def _closed_form(self, sums):
    return cca_calibration_closed_form(sums, self.frames_emitted, self.window_size, self.dims)

  def _host_result(self, outs):
    stats = [np.stack([o['mean_a'], o['mean_b'], o['power']]) for o in outs]
    return CalibrationResult(np.stack([np.stack([st, st]) for st in stats]),
                             np.stack([np.concatenate([o['w'], [o['slope'], o['intercept']]]) for o in outs]),
                             np.array([o['dprime'] for o in outs], np.float64))

  def _device_finish(self):
    return device.online_ccacalib_finish(self._dev['state'], self.dims, self.frames_emitted, self.window_size,
                                         handle=self._dev['h'])

  def finish(self):
    """CalibrationResult(corr [S, 2, 3, dims] {mean_a, mean_b, power} for both speakers, lda [S, dims + 2] {weights,
    slope, intercept}, dprime [S]) float64 from the sums so far -- what OnlineDecoder.set_cca_statistics takes; device
    tensors on the device (one launch; the statuses come back in one small copy), else host arrays.  The state is not
    modified.  ValueError naming the session and the reason: no completed window (train's 'No data for class'), a
    dim's power that is not finite or not above zero, a pooled scatter that is not positive definite (fewer than
    dims + 2 windows in all), equal class means along the LDA axis (scaled LDA's 'X0 and X1 ... identical')."""
    return self._finish()

  def update_decoder(self, decoder, session=0):
    """Gives an infer_decoder.CCADecoder the correlator's sums and statistics and the scaled LDA of one session (what
    Decoder.train leaves in it; the LDA keeps the one axis the scaled transform reads), so that save_parameters
    writes them.  Returns d'."""
    from telluride_decoding_amd import scaled_lda
    o = self._session_form(decoder, infer_decoder.CCADecoder, session)
    w = o['w'].reshape(-1, 1)
    decoder.model_params = infer_decoder.ModelParamsTuple(
        infer_decoder.CorrelationParamsTuple(o['count'], o['sum_x'], o['sum_y'], o['sum_x2'], o['sum_y2'],
                                             o['mean_a'], o['mean_b'], o['power']),
        scaled_lda.LdaParamsTuple(w, np.zeros_like(w), [1, 2], [o['class_means'][0], o['class_means'][1]],
                                  float(o['slope']), float(o['intercept'])))
    return float(o['dprime'])
