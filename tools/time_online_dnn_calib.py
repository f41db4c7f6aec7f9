"""Time per push of the online DNN calibration (td_fccalib_online_push) and of its finish (td_calib_online_finish on
its state) against the route open before it: per push, td_fc_online_push with want_frames keeps the float32 prediction
of every emitted frame, and the envelopes of every row are kept beside it; at the end of the calibration stretch, per
session, device.window_sums twice (the correlator's sums of the two classes), device.window_class_moments twice and
scaled_lda.fit_class_moments give the statistics, the LDA and d'.

  python tools/time_online_dnn_calib.py [--pushes 50] [--warmup 10]

64 channels, 21 lags (post context 20) into hidden layers [64, 64], windows of 100 frames; S in {1, 64} sessions and n
in {10, 100} rows per push.  Every push is timed on its own between device synchronisations, both routes in one run;
finish and the baseline's end of calibration are timed the same way on the state the pushes left, `pushes` times after
`warmup`.  Reported: the median and the range, in microseconds, whether the two ranges overlap, and the bytes each
route keeps per session."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import device, infer_decoder, scaled_lda

C, PRE, POST, WIDTH = 64, 0, 20, 100
HIDDEN = [64, 64]


def _spread(values):
  return [float(np.median(values)), float(np.min(values)), float(np.max(values))]


def _overlap(a, b):
  """Whether the ranges of two _spread results share a point."""
  return a[1] <= b[2] and b[1] <= a[2]


def _batch_end(h, preds, envs, sessions):
  """The baseline's end of calibration: (corr, lda, dprime) per session from the kept predictions and envelopes."""
  out = []
  for s in range(sessions):
    pred = torch.cat([p[s] for p in preds]).reshape(-1, 1)
    rows = int(pred.shape[0])
    env = torch.cat([e[s] for e in envs])[:rows]
    streams = [(env[:, 1:2], pred), (env[:, 0:1], pred)]        # class 0 = unattended, class 1 = attended
    dec = infer_decoder.Decoder()
    queued = [device.window_sums(x, y, [0, rows], rows, rows, handle=h) for x, y in streams]
    for q in queued:
      dec._add_sums(rows, q.cpu().numpy()[0])
    mx, my, pw = dec._stat_vectors(1)
    moments = [device.window_class_moments(x, y, WIDTH, mx, my, pw, handle=h) for x, y in streams]
    lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    lda.fit_class_moments([m.cpu().numpy() for m in moments])
    (m1, v1), (m2, v2) = lda.projected_class_stats()
    out.append(((mx[0], my[0], pw[0]), (1.0, lda.slope, lda.intercept), (m2 - m1) / np.sqrt((v1 + v2) / 2.0)))
  return out


def _model(rng, k):
  """Packed [W1, b1, W2, b2, W3, b3] of a Glorot-uniform network on k inputs, small biases."""
  widths = [k] + HIDDEN + [1]
  parts = []
  for i in range(len(widths) - 1):
    limit = np.sqrt(6.0 / (widths[i] + widths[i + 1]))
    parts.append(rng.uniform(-limit, limit, (widths[i] * widths[i + 1],)))
    parts.append(0.01 * rng.standard_normal((widths[i + 1],)))
  return np.concatenate(parts).astype(np.float32)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=50)
  ap.add_argument('--warmup', type=int, default=10)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  k = (PRE + 1 + POST) * C
  total = args.warmup + args.pushes
  params = h.to_device(_model(rng, k)[None])
  assert int(params.shape[1]) == device.dnn_param_count(k, HIDDEN)
  mix = h.to_device((rng.standard_normal((1, C)) / np.sqrt(C)).astype(np.float32))
  rows = []
  for sessions in (1, 64):
    for n in (10, 100):
      eeg = h.to_device(rng.standard_normal((sessions * total * n, C)).astype(np.float32)).reshape(sessions, total * n, C)
      env = h.to_device(rng.standard_normal((sessions * total * n, 2)).astype(np.float32)).reshape(sessions, total * n, 2)
      env[:, :, 0] += eeg @ mix[0]                            # the attended envelope follows the EEG
      state = torch.zeros((sessions, device.online_dnn_calib_state_bytes(C, PRE, POST)), dtype=torch.uint8,
                          device=h.device)
      old_state = torch.zeros((sessions, device.online_state_bytes(C, PRE, POST, WIDTH)), dtype=torch.uint8,
                              device=h.device)
      corr = torch.tensor([[[0.0, 0.0, 1.0]] * 2] * sessions, dtype=torch.float64, device=h.device)
      preds, envs = [], []
      t_new, t_old = [], []
      for i in range(total):
        lo, hi = i * n, (i + 1) * n
        h.synchronize()
        t0 = time.perf_counter()
        device.online_dnn_calib_push(eeg[:, lo:hi], env[:, lo:hi], params, HIDDEN, state, lo, PRE, POST, WIDTH,
                                     handle=h)
        h.synchronize()
        t1 = time.perf_counter()
        out = device.dnn_online_push(eeg[:, lo:hi], env[:, lo:hi], params, HIDDEN, corr, old_state, lo, PRE, POST,
                                     WIDTH, WIDTH, want_frames=True, handle=h)
        preds.append(out.pred)
        envs.append(env[:, lo:hi])
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      frames = total * n - POST
      kept_new = int(state.shape[1])
      kept_old = int(old_state.shape[1]) + 4 * frames + 8 * total * n
      row = dict(what='push', sessions=sessions, n=n, pushes=len(t_new), online_us=_spread(t_new),
                 baseline_us=_spread(t_old), online_bytes_per_session=kept_new, baseline_bytes_per_session=kept_old)
      row['ranges_overlap'] = _overlap(row['online_us'], row['baseline_us'])
      rows.append(row)
      print('push    S = %2d  n = %3d   online %9.1f us (%.1f - %.1f)   baseline %10.1f us (%.1f - %.1f)   ranges %s   '
            'kept %d / %d bytes per session' %
            ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us']) +
             ('overlap' if row['ranges_overlap'] else 'apart', kept_new, kept_old)))
      t_new, t_old = [], []
      for i in range(total):
        h.synchronize()
        t0 = time.perf_counter()
        fin = device.online_calib_finish(state, frames, WIDTH, handle=h)
        status = fin.status.cpu().numpy()
        h.synchronize()
        t1 = time.perf_counter()
        want = _batch_end(h, preds, envs, sessions)
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      assert not status.any()
      got_d, want_d = fin.dprime.cpu().numpy(), np.array([o[2] for o in want])
      assert np.allclose(got_d, want_d, rtol=1e-9), (got_d, want_d)
      row = dict(what='finish', sessions=sessions, n=n, frames=frames, calls=len(t_new), online_us=_spread(t_new),
                 baseline_us=_spread(t_old))
      row['ranges_overlap'] = _overlap(row['online_us'], row['baseline_us'])
      rows.append(row)
      print('finish  S = %2d  N = %4d   online %9.1f us (%.1f - %.1f)   baseline %10.1f us (%.1f - %.1f)   ranges %s' %
            ((sessions, frames) + tuple(row['online_us']) + tuple(row['baseline_us']) +
             ('overlap' if row['ranges_overlap'] else 'apart',)))
      del state, old_state, eeg, env, preds, envs
  print(json.dumps({'tool': 'time_online_dnn_calib', 'channels': C, 'lags': PRE + 1 + POST, 'hidden': HIDDEN,
                    'width': WIDTH, 'rows': rows}))


if __name__ == '__main__':
  main()
