"""Time per push of the online CCA calibration (td_ccacalib_online_push) and of its finish
(td_ccacalib_online_finish) against the route the library had before it: per push, td_cca_online_push with want_frames
keeps the float32 projections (a | b1 | b0) of every emitted frame; at the end of the calibration stretch, per session,
device.window_sums twice (the correlator's sums of the two classes), device.window_class_moments twice and
scaled_lda.fit_class_moments give the statistics, the LDA and d'.

  python tools/time_online_cca_calib.py [--pushes 50] [--warmup 10]

64 channels x 21 lags (post context 20) against 8 features x 16 lags (post context 15) in 5 dims, windows of 100
frames; S in {1, 64} sessions and n in {10, 100} rows per push.  Every push is timed on its own between device
synchronisations, both routes in one run; finish and the baseline's end of calibration are timed the same way on the
state the pushes left, `pushes` times after `warmup`.  Reported: the median and the range, in microseconds, and the
bytes each route keeps per session."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import device, infer_decoder, scaled_lda

C1, PRE1, POST1, C2, PRE2, POST2, DIMS, WIDTH = 64, 0, 20, 8, 0, 15, 5, 100
VIEWS = (PRE1, POST1, PRE2, POST2)


def _spread(values):
  return [float(np.median(values)), float(np.min(values)), float(np.max(values))]


def _batch_end(h, projs, sessions):
  """The baseline's end of calibration: (statistics, slope w, intercept, d') per session from the kept projections."""
  out = []
  for s in range(sessions):
    proj = torch.cat([p[s] for p in projs])
    rows = int(proj.shape[0])
    a, b1, b0 = (proj[:, i * DIMS:(i + 1) * DIMS] for i in range(3))
    streams = [(a, b0), (a, b1)]                                # class 0 = unattended, class 1 = attended
    dec = infer_decoder.Decoder()
    queued = [device.window_sums(x, y, [0, rows], rows, rows, handle=h) for x, y in streams]
    for q in queued:
      dec._add_sums(rows, q.cpu().numpy()[0])
    mx, my, pw = dec._stat_vectors(DIMS)
    moments = [device.window_class_moments(x, y, WIDTH, mx, my, pw, handle=h) for x, y in streams]
    lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    lda.fit_class_moments([m.cpu().numpy() for m in moments])
    (m1, v1), (m2, v2) = lda.projected_class_stats()
    out.append((np.stack([mx, my, pw]), np.real(lda.slope * np.asarray(lda.coef_array)[:, 0]), lda.intercept,
                (m2 - m1) / np.sqrt((v1 + v2) / 2.0)))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=50)
  ap.add_argument('--warmup', type=int, default=10)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  k1, k2 = (PRE1 + 1 + POST1) * C1, (PRE2 + 1 + POST2) * C2
  total = args.warmup + args.pushes
  up = lambda a: h.to_device(a.reshape(-1, a.shape[-1])).reshape(a.shape)
  rot_x = (rng.standard_normal((1, k1, DIMS)) / np.sqrt(k1)).astype(np.float32)
  rot_y = (rng.standard_normal((1, k2, DIMS)) / np.sqrt(k2)).astype(np.float32)
  model = [up(np.zeros((1, k1), np.float32)), up(rot_x), up(np.zeros((1, k2), np.float32)), up(rot_y)]
  carry = torch.linalg.pinv(model[3][0, :C2].double()).float()   # [DIMS, C2]: a into the attended block's lag 0
  rows = []
  for sessions in (1, 64):
    for n in (10, 100):
      eeg = up(rng.standard_normal((sessions, total * n, C1)).astype(np.float32))
      att = up(rng.standard_normal((sessions, total * n, C2)).astype(np.float32))
      unatt = up(rng.standard_normal((sessions, total * n, C2)).astype(np.float32))
      att += (eeg @ model[1][0, :C1]) @ carry                   # the attended block follows the EEG (the lag-0 terms)
      state = torch.zeros((sessions, device.online_ccacalib_state_bytes(C1, PRE1, POST1, C2, PRE2, POST2, DIMS)),
                          dtype=torch.uint8, device=h.device)
      old_state = torch.zeros((sessions, device.cca_online_state_bytes(C1, PRE1, POST1, C2, PRE2, POST2, WIDTH)),
                              dtype=torch.uint8, device=h.device)
      corr = torch.ones((sessions, 2, 3, DIMS), dtype=torch.float64, device=h.device)
      projs = []
      t_new, t_old = [], []
      for i in range(total):
        lo, hi = i * n, (i + 1) * n
        h.synchronize()
        t0 = time.perf_counter()
        device.online_ccacalib_push(eeg[:, lo:hi], att[:, lo:hi], unatt[:, lo:hi], *model, state, lo, *VIEWS, WIDTH,
                                    handle=h)
        h.synchronize()
        t1 = time.perf_counter()
        out = device.cca_online_push(eeg[:, lo:hi], att[:, lo:hi], unatt[:, lo:hi], *model, corr, old_state, lo,
                                     *VIEWS, WIDTH, WIDTH, want_frames=True, handle=h)
        projs.append(out.proj)
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      frames = total * n - max(POST1, POST2)
      kept_new = int(state.shape[1])
      kept_old = int(old_state.shape[1]) + 4 * 3 * DIMS * frames
      row = dict(what='push', sessions=sessions, n=n, pushes=len(t_new), online_us=_spread(t_new),
                 baseline_us=_spread(t_old), online_bytes_per_session=kept_new, baseline_bytes_per_session=kept_old)
      rows.append(row)
      print('push    S = %2d  n = %3d   online %9.1f us (%.1f - %.1f)   baseline %10.1f us (%.1f - %.1f)   kept %d / '
            '%d bytes per session' % ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us']) +
                                   (kept_new, kept_old)))
      t_new, t_old = [], []
      for i in range(total):
        h.synchronize()
        t0 = time.perf_counter()
        fin = device.online_ccacalib_finish(state, DIMS, frames, WIDTH, handle=h)
        status = fin.status.cpu().numpy()
        h.synchronize()
        t1 = time.perf_counter()
        want = _batch_end(h, projs, sessions)
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      assert not status.any(), status
      got_d, want_d = fin.dprime.cpu().numpy(), np.array([o[3] for o in want])
      assert np.allclose(got_d, want_d, rtol=1e-9), (got_d, want_d)
      row = dict(what='finish', sessions=sessions, n=n, frames=frames, calls=len(t_new), online_us=_spread(t_new),
                 baseline_us=_spread(t_old))
      rows.append(row)
      print('finish  S = %2d  N = %4d   online %9.1f us (%.1f - %.1f)   baseline %10.1f us (%.1f - %.1f)' %
            ((sessions, frames) + tuple(row['online_us']) + tuple(row['baseline_us'])))
      del state, old_state, eeg, att, unatt, projs
  print(json.dumps({'tool': 'time_online_cca_calib', 'views': [C1, PRE1 + 1 + POST1, C2, PRE2 + 1 + POST2],
                    'dims': DIMS, 'width': WIDTH, 'rows': rows}))


if __name__ == '__main__':
  main()
