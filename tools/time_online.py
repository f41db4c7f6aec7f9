"""Time per push of the online decoder (td_online_push) against the same push built from the calls the
library had before it: per session, concatenate the kept tail and the chunk on the device, predict_fir,
frame_scores twice, append to a score buffer, window_means + decide_wta when a window completes.

  python tools/time_online.py [--pushes 200] [--warmup 20]

64 channels, 32 lags (post context 31), windows of 100 frames every 50, winner-take-all; S in {1, 64} sessions
and n in {1, 10, 100} frames per push.  Every push is timed on its own between device synchronisations;
reported: the median and the range over the pushes after the warm-up, in microseconds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import device

C, PRE, POST, WIDTH, HOP = 64, 0, 31, 100, 50


class Baseline(object):
  """One session out of the existing calls; the state a caller has to keep by hand."""

  def __init__(self, h, w, b, corr):
    self.h, self.w, self.b, self.corr = h, w.reshape(-1, 1).contiguous(), b.reshape(1), corr
    self.tail = h.zeros((PRE + POST, C))
    self.env_tail = h.zeros((POST, 2))
    self.buf = [h.zeros((0,), 'float64'), h.zeros((0,), 'float64')]
    self.buf_start, self.pushed, self.windows = 0, 0, 0

  def push(self, eeg, env):
    h, n = self.h, int(eeg.shape[0])
    rows = torch.cat([self.tail, eeg])
    envs = torch.cat([self.env_tail, env])
    pred = device.predict_fir(rows, [0, int(rows.shape[0])], self.w, self.b, PRE, POST, handle=h)
    first = max(0, self.pushed - POST)                  # frames [first, last) come out of this push
    last = max(0, self.pushed + n - POST)
    lo = first - (self.pushed - POST)                   # (frames before the recording are dropped)
    pred, truth = pred[PRE + lo:PRE + n], envs[lo:n]
    out = None
    if last > first:
      for k in (0, 1):
        cr = self.corr[k]
        frame = device.frame_scores(truth[:, k:k + 1], pred, 'first', cr[0], cr[1], cr[2], handle=h)
        self.buf[k] = torch.cat([self.buf[k], frame])
      total = (last - WIDTH) // HOP + 1 if last >= WIDTH else 0
      if total > self.windows:
        at = self.windows * HOP - self.buf_start
        means = [device.window_means(self.buf[k][at:], [0, int(self.buf[k].shape[0]) - at], WIDTH, HOP, handle=h)
                 for k in (0, 1)]
        out = (means, device.decide_wta(means[0], means[1], handle=h))
        self.windows = total
        keep = self.windows * HOP - self.buf_start
        self.buf = [v[keep:] for v in self.buf]
        self.buf_start += keep
    self.tail = rows[int(rows.shape[0]) - (PRE + POST):]
    self.env_tail = envs[int(envs.shape[0]) - POST:]
    self.pushed += n
    return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  k = C * (PRE + 1 + POST)
  w = h.to_device((rng.standard_normal((1, k)) / np.sqrt(k)).astype(np.float32))
  b = h.to_device(np.zeros((1, 1), np.float32)).reshape(-1)
  stats = [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]
  rows = []
  for sessions in (1, 64):
    corr = h.to_device(np.array([stats] * sessions).reshape(-1, 6), np.float64).reshape(sessions, 2, 3)
    for n in (1, 10, 100):
      total = args.warmup + args.pushes
      eeg = h.to_device(rng.standard_normal((sessions * total * n, C)).astype(np.float32)).reshape(sessions, total * n, C)
      env = h.to_device(rng.standard_normal((sessions * total * n, 2)).astype(np.float32)).reshape(sessions, total * n, 2)
      nbytes = device.online_state_bytes(C, PRE, POST, WIDTH)
      state = torch.zeros((sessions, nbytes), dtype=torch.uint8, device=h.device)
      base = [Baseline(h, w, b, stats) for _ in range(sessions)]
      t_new, t_old = [], []
      for i in range(total):
        lo, hi = i * n, (i + 1) * n
        h.synchronize()
        t0 = time.perf_counter()
        device.online_push(eeg[:, lo:hi], env[:, lo:hi], w, b, corr, state, lo, PRE, POST, WIDTH, HOP, 'first',
                           None, 'wta', handle=h)
        h.synchronize()
        t1 = time.perf_counter()
        for s in range(sessions):
          base[s].push(eeg[s, lo:hi], env[s, lo:hi])
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      row = dict(sessions=sessions, n=n, pushes=len(t_new),
                 online_us=[float(np.median(t_new)), float(np.min(t_new)), float(np.max(t_new))],
                 baseline_us=[float(np.median(t_old)), float(np.min(t_old)), float(np.max(t_old))])
      rows.append(row)
      print('S = %2d  n = %3d   online %8.1f us (%.1f - %.1f)   baseline %9.1f us (%.1f - %.1f)' %
            ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us'])))
  print(json.dumps({'tool': 'time_online', 'channels': C, 'lags': PRE + 1 + POST, 'window': [WIDTH, HOP],
                    'rows': rows}))


if __name__ == '__main__':
  main()
