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


def session_parameters(decoder):
  """What one listener's session needs from its decoder, checked against the online path's limits:
  dict(c, pre, post, w [lags c] float32, b float32, corr [2, 3] float64, lda [3] float64 or None,
  reduction)."""
  if not isinstance(decoder, infer_decoder.LinearRegressionDecoder):
    raise ValueError('OnlineDecoder decodes with a LinearRegressionDecoder (no CCA model online), not a %s.' %
                     type(decoder).__name__)
  model = decoder.decoding_model
  if not isinstance(model, brain_model.BrainModelLinearRegression):
    raise ValueError('OnlineDecoder needs a BrainModelLinearRegression (no DNN or CCA model online), not a %s.' %
                     type(model).__name__)
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
  return dict(c=c, pre=pre, post=post, w=w[:, 0].copy(), b=np.float32(np.reshape(model.b_estimate, -1)[0]),
              corr=np.array([stats, stats], np.float64), lda=lda, reduction=reduction)


def _frame_score(truth, pred, stats, reduction, lda):
  v = (truth - stats[0]) * (pred - stats[1]) / stats[2]
  if reduction == 'first':
    return v
  if reduction == 'mean':
    return 0.0 + v
  if reduction == 'mean-squared':
    return 0.0 + np.where(v > 0.0, v * v, np.where(v < 0.0, -v * v, 0.0))
  return lda[1] * (v * lda[0]) + lda[2]


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
    rows = np.concatenate([self.tail, eeg] + ([np.zeros((post, c))] if flush else []))
    envs = np.concatenate([self.env_tail, env])
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
    both = np.concatenate([self.tail, eeg])
    self.tail = both[both.shape[0] - (pre + post):]
    self.env_tail = envs[envs.shape[0] - post:] if post else envs[:0]
    return scores, decisions, pred, frame, pl


class OnlineDecoder(object):
  """A bank of online decoding sessions, one per listener.

  decoders: one infer_decoder.LinearRegressionDecoder around a fitted BrainModelLinearRegression, or a list
  of S of them -- one listener each, with its own weights and trained statistics (the channel count and the
  context are the bank's: every decoder has the same).  The reduction, the correlation parameters and the
  LDA come from each decoder; both speakers are scored with the decoder's one set of statistics, as
  infer.run_reduction_test does.  window_step defaults to window_size // 2.  decoder_type: 'wta',
  'stepped' or 'ssd' (two launches per push: the windows, then td_decode_ssd_stream on them, device to
  device).
  """

  def __init__(self, decoders, window_size, window_step=None, decoder_type='wta', frame_rate=100.0,
               ssd_offset=0.0):
    if isinstance(decoders, infer_decoder.Decoder) or not isinstance(decoders, (list, tuple)):
      decoders = [decoders]
    if not decoders:
      raise ValueError('OnlineDecoder needs at least one decoder.')
    self._params = [session_parameters(d) for d in decoders]
    first = self._params[0]
    for p in self._params[1:]:
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
    self.sessions = len(self._params)
    self.channels, self.pre, self.post = first['c'], first['pre'], first['post']
    self.reduction = first['reduction']
    self.window_size, self.window_step = window_size, window_step
    self.decoder_type = 'stepped' if decoder_type == 'step' else decoder_type
    self._ssd = None
    if self.decoder_type == 'ssd':
      self._ssd = attention_decoder.create_attention_decoder('ssd', window_step=window_step,
                                                             frame_rate=frame_rate, ssd_offset=ssd_offset)
    self._on_device = device.gpu_available()
    if self._ssd is not None and not self._on_device:
      raise _lib.HotPathUnavailable('The state-space decoder has no host form: \'ssd\' needs the GPU.')
    self._dev = None
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
    torch = device._torch()
    ps = self._params
    # (sessions around ONE model read one copy of it)
    shared = all(np.array_equal(p['w'], ps[0]['w']) and p['b'] == ps[0]['b'] for p in ps[1:])
    models = ps[:1] if shared else ps
    dev = dict(h=h)
    dev['w'] = h.to_device(np.stack([p['w'] for p in models]))
    dev['b'] = h.to_device(np.array([[p['b']] for p in models], np.float32)).reshape(-1)
    dev['corr'] = h.to_device(np.stack([p['corr'] for p in ps]).reshape(-1, 6), np.float64).reshape(-1, 2, 3)
    dev['lda'] = (h.to_device(np.stack([p['lda'] for p in ps]), np.float64)
                  if self.reduction == 'lda' else None)
    nbytes = device.online_state_bytes(self.channels, self.pre, self.post, self.window_size)
    dev['state'] = torch.zeros((self.sessions, nbytes), dtype=torch.uint8, device=h.device)
    dev['ssd_state'] = device.ssd_state(self.sessions, handle=h) if self._ssd is not None else None
    return dev

  def reset(self):
    """A fresh recording: zero state, no frame pushed."""
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
      self._host = [_HostSession(p, self.window_size, self.window_step, kind) for p in self._params]

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

  # -- pushes ------------------------------------------------------------------------------------
  def _as_bank(self, eeg, env1, env2):
    """(eeg [S, n, C], env [S, n, 2]) as float32 host arrays or device tensors."""
    s, c = self.sessions, self.channels
    tensors = [hasattr(a, 'is_cuda') for a in (eeg, env1, env2)]
    if any(tensors):
      torch = device._torch()
      h = self._dev['h'] if self._on_device else None
      conv = lambda a: (a if hasattr(a, 'is_cuda') else torch.as_tensor(np.asarray(a))).to(
          device=h.device if h else None, dtype=torch.float32)
      eeg, env1, env2 = conv(eeg), conv(env1), conv(env2)
      if eeg.dim() == 2:
        eeg, env1, env2 = eeg.unsqueeze(0), env1.reshape(1, -1), env2.reshape(1, -1)
      env = torch.stack([env1.reshape(eeg.shape[0], -1), env2.reshape(eeg.shape[0], -1)], dim=2)
      eeg = eeg.contiguous()
      if not self._on_device:
        eeg, env = eeg.cpu().numpy(), env.cpu().numpy()
    else:
      eeg = np.asarray(eeg, np.float32)
      if eeg.ndim == 2:
        eeg = eeg[None]
      env = np.stack([np.asarray(env1, np.float32).reshape(eeg.shape[0], -1),
                      np.asarray(env2, np.float32).reshape(eeg.shape[0], -1)], axis=2)
    if eeg.ndim != 3 or tuple(eeg.shape[0:3:2]) != (s, c) or tuple(env.shape) != (s, eeg.shape[1], 2):
      raise ValueError('A push is eeg [%d, n, %d] (or [n, %d] for one session) with two envelopes of n frames '
                       'each, not eeg %s with envelopes %s.' % (s, c, c, tuple(eeg.shape), tuple(env.shape[:2])))
    return eeg, env

  def push(self, eeg, env1, env2):
    """The next n frames of every session: eeg [n, C] / [S, n, C], env1 and env2 [n] / [S, n] (speaker 1,
    speaker 2), host arrays or device tensors.  Returns OnlineResult(scores [S, new, 2] float64, decisions
    [S, new] uint8 -- [S, new, 3] float64 (p, lower, upper) for 'ssd' --, first_window) for the windows this
    push completes (host arrays)."""
    if self.flushed:
      raise ValueError('The session was flushed: reset() starts the next recording.')
    eeg, env = self._as_bank(eeg, env1, env2)
    return self._advance(eeg, env, False)

  def flush(self):
    """The end of the recording: the last post_context frames are emitted as if zero rows followed.  After
    it the session refuses pushes until reset()."""
    if self.flushed:
      raise ValueError('The session was flushed: reset() starts the next recording.')
    result = self._advance(None, None, True)
    self.flushed = True
    return result

  def _advance(self, eeg, env, flush):
    n = 0 if eeg is None else int(eeg.shape[1])
    kind = 'none' if self.decoder_type == 'ssd' else self.decoder_type
    if not self._on_device:
      if eeg is None:
        eeg = np.zeros((self.sessions, 0, self.channels), np.float32)
        env = np.zeros((self.sessions, 0, 2), np.float32)
      outs = [sess.push(np.asarray(eeg[i], np.float64), np.asarray(env[i], np.float64), self.frames_pushed,
                        flush) for i, sess in enumerate(self._host)]
      self.frames_pushed += n
      return OnlineResult(np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
                          outs[0][4].first_window)
    d = self._dev
    h = d['h']
    if eeg is not None and not hasattr(eeg, 'is_cuda'):
      eeg, env = h.to_device(eeg.reshape(-1, self.channels)).reshape(eeg.shape), \
          h.to_device(env.reshape(-1, 2)).reshape(env.shape)
    if n == 0:
      eeg = env = None
    out = device.online_push(eeg, env, d['w'], d['b'], d['corr'], d['state'], self.frames_pushed, self.pre,
                             self.post, self.window_size, self.window_step, self.reduction, d['lda'], kind,
                             flush=flush, handle=h)
    self.frames_pushed += n
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
