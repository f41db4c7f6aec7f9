"""Time per push of the online DNN decoder (td_fc_online_push) against the same push built from the calls the
library offers without it: per session, concatenate the kept tails and the chunk on the device, mlp_forward on them
(three launches), frame_scores twice, append to a score buffer, window_means + decide_wta when a window completes.

  python tools/time_online_dnn.py [--pushes 200] [--warmup 20]

Two models: 64 channels x 21 lags into hidden [64, 64] (W1 344 KB), and 128 channels x 64 lags into hidden [64]
(W1 2 MB, the largest the kernels take).  Reduction 'first', windows of 100 frames every 50, winner-take-all; S in
{1, 64} sessions (one shared model) and n in {1, 10, 100} frames per push.  Every push is timed on its own between
device synchronisations; reported: the median and the range over the pushes after the warm-up, in microseconds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import device

MODELS = [((64, 0, 20), [64, 64]), ((128, 31, 32), [64])]
WIDTH, HOP = 100, 50


class Baseline(object):
  """One session out of the existing calls; the state a caller has to keep by hand."""

  def __init__(self, h, shape, hidden, params, stats):
    self.h, (self.c, self.pre, self.post), self.hidden, self.params, self.stats = h, shape, hidden, params, stats
    self.tail = h.zeros((self.pre + self.post, self.c))
    self.env_tail = h.zeros((self.post, 2))
    self.buf = [h.zeros((0,), 'float64'), h.zeros((0,), 'float64')]
    self.buf_start, self.pushed, self.windows = 0, 0, 0

  def push(self, eeg, env):
    h, n, pre, post = self.h, int(eeg.shape[0]), self.pre, self.post
    rows = torch.cat([self.tail, eeg])                  # rows[0] is the EEG row pushed - pre - post
    envs = torch.cat([self.env_tail, env])              # envs[0] is the envelope row pushed - post
    first = max(0, self.pushed - post)                  # frames [first, last) come out of this push
    last = max(0, self.pushed + n - post)
    out = None
    if last > first:
      # frame t reads rows t - pre .. t + post = rows[a + (t - first) ...]: the block below holds exactly the rows
      # the emitted frames read, so neither end is padded with zeros; its outputs pre .. pre + count are the frames
      a, count = first - (self.pushed - post), last - first
      x = rows[a:a + count + pre + post]
      pred = device.mlp_forward(x, [0, int(x.shape[0])], pre, post, self.hidden, 1, self.params, handle=h)
      pred = pred[pre:pre + count]
      truth = envs[a:a + count]
      for k in (0, 1):
        frame = device.frame_scores(truth[:, k:k + 1], pred, 'first', self.stats[0], self.stats[1], self.stats[2],
                                    handle=h)
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
    self.tail = rows[int(rows.shape[0]) - (pre + post):]
    self.env_tail = envs[int(envs.shape[0]) - post:]
    self.pushed += n
    return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  gen = torch.Generator(device=h.device)
  gen.manual_seed(0)
  stats = [0.0, 0.0, 1.0]
  results = []
  for (c, pre, post), hidden in MODELS:
    widths = [c * (pre + 1 + post)] + hidden + [1]
    flat = []
    for fi, fo in zip(widths[:-1], widths[1:]):
      lim = np.sqrt(6.0 / (fi + fo))
      flat += [rng.uniform(-lim, lim, (fi * fo,)), 0.01 * rng.standard_normal(fo)]
    params = h.to_device(np.concatenate(flat).astype(np.float32).reshape(1, -1))
    pass_, lds = device.dnn_online_lds_bytes(c, pre, post, hidden, 100)
    print('%d channels x %d lags, hidden %s: W1 %d KB, %d frames a pass, %d bytes of LDS' %
          (c, pre + 1 + post, hidden, widths[0] * widths[1] * 4 // 1024, pass_, lds), flush=True)
    rows = []
    for sessions in (1, 64):
      corr = h.to_device(np.tile(np.array(stats), (2 * sessions, 1)), np.float64).reshape(sessions, 2, 3)
      for n in (1, 10, 100):
        total = args.warmup + args.pushes
        eeg = torch.randn((sessions, total * n, c), generator=gen, device=h.device, dtype=torch.float32)
        env = torch.randn((sessions, total * n, 2), generator=gen, device=h.device, dtype=torch.float32)
        nbytes = device.online_state_bytes(c, pre, post, WIDTH)
        state = torch.zeros((sessions, nbytes), dtype=torch.uint8, device=h.device)
        base = [Baseline(h, (c, pre, post), hidden, params[0], stats) for _ in range(sessions)]
        t_new, t_old = [], []
        for i in range(total):
          lo, hi = i * n, (i + 1) * n
          h.synchronize()
          t0 = time.perf_counter()
          device.dnn_online_push(eeg[:, lo:hi], env[:, lo:hi], params, hidden, corr, state, lo, pre, post, WIDTH, HOP,
                                 'first', None, 'wta', handle=h)
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
              ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us'])), flush=True)
        del eeg, env
    results.append(dict(shape=[c, pre, post], hidden=hidden, pass_frames=pass_, lds_bytes=lds, rows=rows))
  print(json.dumps({'tool': 'time_online_dnn', 'reduction': 'first', 'window': [WIDTH, HOP], 'models': results}))


if __name__ == '__main__':
  main()
