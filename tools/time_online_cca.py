"""Time per push of the online CCA decoder (td_cca_online_push) against the same push built from the calls the
library offers without it: per session, concatenate the kept tails and the chunk on the device, cca_transform
once per speaker (each projects the EEG view again), frame_scores twice, append to a score buffer,
window_means + decide_wta when a window completes.

  python tools/time_online_cca.py [--pushes 200] [--warmup 20]

64 channels x 21 lags against 8 feature bands x 16 lags, 5 dims, reduction 'lda', windows of 100 frames every 50,
winner-take-all; S in {1, 64} sessions and n in {1, 10, 100} frames per push.  Every push is timed on its own
between device synchronisations; reported: the median and the range over the pushes after the warm-up, in
microseconds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import device

C1, PRE1, POST1 = 64, 0, 20
C2, PRE2, POST2 = 8, 0, 15
DIMS, WIDTH, HOP = 5, 100, 50
POST = max(POST1, POST2)
assert PRE1 == 0 and PRE2 == 0          # (the baseline below cuts its views for views without pre-context)


class Baseline(object):
  """One session out of the existing calls; the state a caller has to keep by hand."""

  def __init__(self, h, model, stats, lda):
    self.h, self.model, self.stats = h, model, stats
    self.lda = dict(lda_w=lda[:-2], lda_slope=lda[-2], lda_intercept=lda[-1])
    self.tail = h.zeros((PRE1 + POST, C1))
    self.feat_tail = [h.zeros((PRE2 + POST, C2)) for _ in (0, 1)]
    self.buf = [h.zeros((0,), 'float64'), h.zeros((0,), 'float64')]
    self.buf_start, self.pushed, self.windows = 0, 0, 0

  def push(self, eeg, feats):
    h, n = self.h, int(eeg.shape[0])
    m1, r1, m2, r2 = self.model
    rows = torch.cat([self.tail, eeg])                  # rows[0] is the EEG row pushed - PRE1 - POST
    frows = [torch.cat([self.feat_tail[k], feats[k]]) for k in (0, 1)]
    first = max(0, self.pushed - POST)                  # frames [first, last) come out of this push
    last = max(0, self.pushed + n - POST)
    out = None
    if last > first:
      # (no pre-context here: frame t sits at rows[t - (pushed - POST)] in both views; the `POST` rows behind the
      # last emitted frame go in as well so that neither view is padded with zeros, and their outputs are dropped)
      a1, a2 = first - (self.pushed - POST), last - (self.pushed - POST)
      x = rows[a1:a2 + POST]
      for k in (0, 1):
        y = frows[k][a1:a2 + POST]
        z = device.cca_transform(x, y, [0, int(x.shape[0])], m1, r1, m2, r2, PRE1, POST1, PRE2, POST2, handle=h)
        frame = device.frame_scores(z[:last - first, :DIMS], z[:last - first, DIMS:], 'lda', self.stats[0],
                                    self.stats[1], self.stats[2], handle=h, **self.lda)
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
    self.tail = rows[int(rows.shape[0]) - (PRE1 + POST):]
    self.feat_tail = [f[int(f.shape[0]) - (PRE2 + POST):] for f in frows]
    self.pushed += n
    return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  k1, k2 = C1 * (PRE1 + 1 + POST1), C2 * (PRE2 + 1 + POST2)
  up = lambda a: h.to_device(a.astype(np.float32))
  mean_x, mean_y = up(rng.standard_normal((1, k1))), up(rng.standard_normal((1, k2)))
  rot_x, rot_y = up(rng.standard_normal((k1, DIMS)) / np.sqrt(k1)), up(rng.standard_normal((k2, DIMS)) / np.sqrt(k2))
  stats = np.stack([np.zeros(DIMS), np.zeros(DIMS), np.ones(DIMS)])
  lda = np.concatenate([rng.standard_normal(DIMS), [1.5, 0.1]])
  rows = []
  for sessions in (1, 64):
    corr = h.to_device(np.tile(stats.reshape(1, -1), (2 * sessions, 1)).reshape(-1, DIMS),
                       np.float64).reshape(sessions, 2, 3, DIMS)
    lda_dev = h.to_device(np.tile(lda, (sessions, 1)), np.float64)
    for n in (1, 10, 100):
      total = args.warmup + args.pushes
      block = lambda c: h.to_device(rng.standard_normal((sessions * total * n, c)).astype(np.float32)).reshape(
          sessions, total * n, c)
      eeg, feat = block(C1), [block(C2), block(C2)]
      nbytes = device.cca_online_state_bytes(C1, PRE1, POST1, C2, PRE2, POST2, WIDTH)
      state = torch.zeros((sessions, nbytes), dtype=torch.uint8, device=h.device)
      base = [Baseline(h, (mean_x, rot_x, mean_y, rot_y), stats, lda) for _ in range(sessions)]
      t_new, t_old = [], []
      for i in range(total):
        lo, hi = i * n, (i + 1) * n
        h.synchronize()
        t0 = time.perf_counter()
        device.cca_online_push(eeg[:, lo:hi], feat[0][:, lo:hi], feat[1][:, lo:hi], mean_x, rot_x.unsqueeze(0),
                               mean_y, rot_y.unsqueeze(0), corr, state, lo, PRE1, POST1, PRE2, POST2, WIDTH, HOP,
                               'lda', lda_dev, 'wta', handle=h)
        h.synchronize()
        t1 = time.perf_counter()
        for s in range(sessions):
          base[s].push(eeg[s, lo:hi], [feat[0][s, lo:hi], feat[1][s, lo:hi]])
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
            ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us'])), flush=True)
  print(json.dumps({'tool': 'time_online_cca', 'view1': [C1, PRE1, POST1], 'view2': [C2, PRE2, POST2], 'dims': DIMS,
                    'reduction': 'lda', 'window': [WIDTH, HOP], 'rows': rows}))


if __name__ == '__main__':
  main()
