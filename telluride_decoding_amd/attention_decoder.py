"""Attended-speaker decision on the HIP hot path.

Same classes and call signatures as reference attention_decoder.py:
`AttentionDecoder` (winner take all, :116-138), `StepAttentionDecoder`
(:141-173), `StateSpaceAttentionDecoder` (:176-451) and
`create_attention_decoder` (:455-485).  `plot_aad_results` (:27-113) is out of
scope (matplotlib reporting).

Two ways in:
  * `attention(r1, r2)` -- the reference's streaming call, one window at a time,
    stateful.  For the winner-take-all and step decoders that is ONE float64
    compare (and a clipped +-0.1): it is done where the two scalars are, on the
    host, in the same IEEE float64 operations as the kernels of the batched path
    (decide_wta_kernel / decide_step_kernel, windows.hip) -- uploading two scalars
    and launching a kernel cost a streaming caller ~30 us per window for a `>`.
    The state-space decoder's call is real work (EM + Kalman + Newton) and runs
    the same HIP kernel as the batched path on a one-trial problem.
  * `attention_batch(r1, r2, window_offsets)` -- every window of every trial in
    one launch (trials are independent; the step and state-space decoders are
    sequential in time within a trial, one GPU lane per trial).
"""
import numpy as np

from telluride_decoding_amd import device


def _dev_f64(h, values):
  return h.to_device(np.asarray(values, np.float64).reshape(-1, 1), np.float64).reshape(-1)


class AttentionDecoder(object):
  """Winner takes all: speaker 1 iff mean(r1) > mean(r2) (strict; ties go to 2)."""

  def attention(self, r1, r2):
    # np.mean over a vector argument, as the reference does (:134); strict >
    return bool(np.mean(r1) > np.mean(r2)), 0, 0

  def attention_batch(self, r1, r2, window_offsets=None):
    """r1, r2: per-window scores (host arrays or float64 device tensors)."""
    del window_offsets
    h = device.default_handle()
    s1 = r1 if hasattr(r1, 'is_cuda') else _dev_f64(h, r1)
    s2 = r2 if hasattr(r2, 'is_cuda') else _dev_f64(h, r2)
    out = device.decide_wta(s1, s2, handle=h).cpu().numpy().astype(bool)
    zeros = np.zeros(out.shape[0])
    return out, zeros, zeros

  def tune(self, r1, r2):
    """An optional training step for tuning parameters."""
    del r1, r2


class StepAttentionDecoder(AttentionDecoder):
  """Hysteresis: a state starting at 0.5 moves +-0.1 per window inside
  [0.1, 0.9]; the decision is state > 0.5."""

  def __init__(self):
    self.state = 0.5

  def attention(self, r1, r2):
    # the float64 operations of decide_step_kernel (reference :169-173)
    if np.mean(r1) > np.mean(r2):
      self.state = min(0.9, self.state + 0.1)
    else:
      self.state = max(0.1, self.state - 0.1)
    return self.state > 0.5, 0, 0

  def attention_batch(self, r1, r2, window_offsets=None):
    h = device.default_handle()
    s1 = r1 if hasattr(r1, 'is_cuda') else _dev_f64(h, r1)
    s2 = r2 if hasattr(r2, 'is_cuda') else _dev_f64(h, r2)
    if window_offsets is None:
      window_offsets = [0, int(s1.shape[0])]
    out, _ = device.decide_step(s1, s2, window_offsets, handle=h)
    out = out.cpu().numpy().astype(bool)
    zeros = np.zeros(out.shape[0])
    return out, zeros, zeros


class StateSpaceAttentionDecoder(AttentionDecoder):
  """Fixed-lag state-space decoder (Miran/Akram et al.), reference :176-451."""

  def __init__(self, outer_iter, inner_iter, newton_iter, fs_corr, forward_lag=0,
               backward_lag=13, offset=0.0):
    self._offset = offset
    self.outer_iter, self.inner_iter, self.newton_iter = outer_iter, inner_iter, newton_iter
    self.fs_corr = fs_corr
    self.forward_lag, self.backward_lag = forward_lag, backward_lag
    self.k_f, self.k_b = forward_lag, backward_lag
    self.k_w = self.k_f + self.k_b + 1
    self.calls = 0
    self.r1, self.r2 = [], []
    self._prior = None
    # defaults of the reference (:266-271); replaced by tune()
    self.alpha_0 = [6.4113e+02, 4.0434e+03]
    self.beta_0 = [3.7581e+02, 6.2791e+03]
    self.mu_0 = [-0.3994, -1.5103]
    self.rho_d = [1.7060, 0.64395]
    self.mu_d = [-0.3994, -1.5103]

  def tune(self, r1, r2):
    return self.tune_log_normal_priors(r1, r2)

  def tune_log_normal_priors(self, r1, r2):
    """Moment-matched log-normal priors from an initial attended/unattended
    stretch (reference :277-327).  A handful of scalar reductions: host."""
    a1 = np.absolute(np.asarray(r1, np.float64) + self._offset)
    a2 = np.absolute(np.asarray(r2, np.float64) + self._offset)
    n = a1.shape[0]

    def fit(a):
      u = np.sum(a) / n
      v = np.sum((a - u) ** 2) / n
      rho = 1 / np.log(v / u ** 2 + 1)
      return rho, np.log(u) - 0.5 / rho

    rho_a, mu_a = fit(a1)
    rho_u, mu_u = fit(a2)
    self.rho_d, self.mu_d = [rho_a, rho_u], [mu_a, mu_u]
    self.mu_0 = [mu_a, mu_u]
    self._prior = ([rho_a, rho_u], [mu_a, mu_u])
    if getattr(self, '_state', None) is not None:
      # a streaming decoder tuned after it has seen windows: the reference overwrites its running
      # rho_d / mu_d (attention_decoder.py:277-327); theirs sit behind the 8 arrays of the state
      import torch
      base = int(self._state.shape[1]) - 8
      self._state[0, base + 1:base + 5] = torch.tensor([rho_a, rho_u, mu_a, mu_u], dtype=torch.float64,
                                                        device=self._state.device)

  def _run(self, s1, s2, window_offsets, h, state=None):
    return device.decode_ssd(s1, s2, window_offsets, self.outer_iter, self.inner_iter,
                             self.newton_iter, self.k_f, self.k_b, self._offset, self._prior,
                             handle=h, state=state)

  def attention(self, r1, r2):
    """Streaming call: the decoder's state lives on the device (td_decode_ssd_stream) and one
    window is decoded per call -- constant cost per window, like the reference's stateful object
    (replaying the whole history, as the first version did, made the n-th call cost n windows).
    Returns the newest window's (p, lower, upper)."""
    self.calls += 1
    self.r1.append(float(np.mean(r1)))
    self.r2.append(float(np.mean(r2)))
    h = device.default_handle()
    if getattr(self, '_state', None) is None:
      self._state = device.ssd_state(1, handle=h)
    out = self._run(_dev_f64(h, self.r1[-1:]), _dev_f64(h, self.r2[-1:]), [0, 1], h, state=self._state)
    if self.calls < self.k_w:
      return (0.5, 0.5, 0.5)
    return tuple(float(v) for v in out[0].cpu().numpy())

  def attention_batch(self, r1, r2, window_offsets=None):
    h = device.default_handle()
    s1 = r1 if hasattr(r1, 'is_cuda') else _dev_f64(h, r1)
    s2 = r2 if hasattr(r2, 'is_cuda') else _dev_f64(h, r2)
    if window_offsets is None:
      window_offsets = [0, int(s1.shape[0])]
    out = self._run(s1, s2, window_offsets, h).cpu().numpy()
    return out[:, 0], out[:, 1], out[:, 2]


def create_attention_decoder(type_name, window_step=100, frame_rate=100.0, ssd_offset=0.0):
  """'wta', 'stepped'/'step' or 'ssd' (reference :455-485)."""
  if type_name == 'wta':
    return AttentionDecoder()
  elif type_name == 'stepped' or type_name == 'step':
    return StepAttentionDecoder()
  elif type_name == 'ssd':
    fs_corr = window_step * float(frame_rate) / 2.0
    return StateSpaceAttentionDecoder(20, 1, 10, fs_corr, offset=ssd_offset)
  raise ValueError('Unknown type (%s) requested from create_attention_decoder' % type_name)
