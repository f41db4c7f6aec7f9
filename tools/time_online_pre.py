"""Time per push of the online front end (td_frontend_push) against what the library offered before it, per
session: Preprocessor.process on the same device-tensor chunk, the filters carrying their state.

  python tools/time_online_pre.py [--pushes 200] [--warmup 20]

64 channels, 1000 -> 100 Hz, a 0.5 Hz order-4 high-pass plus the automatic low-pass (7 sections), a global
re-reference, normalisation; S in {1, 64} sessions and n in {10, 100, 1000} raw rows per push (multiples of the
resampling period: the baseline raises on any other chunk).  Every push is timed on its own between device
synchronisations; reported: the median and the range over the pushes after the warm-up, in microseconds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from telluride_decoding_amd import device, online, preprocess

C = 64
KW = dict(highpass_cutoff=0.5, highpass_order=4, channels_to_ref=[list(range(C))], data_mean=0.25, data_std=1.5)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  rows = []
  for sessions in (1, 64):
    for n in (10, 100, 1000):
      total = args.warmup + args.pushes
      # the same `total` chunks over again for every session: only the time matters
      raw = h.to_device((2.0 + rng.standard_normal((total * n, C))).astype(np.float32))
      x = raw.unsqueeze(0).expand(sessions, total * n, C).contiguous() if sessions * total * n * C <= (1 << 28) \
          else None
      front = online.OnlinePreprocessor(preprocess.Preprocessor('eeg', 1000, 100, **KW), num_sessions=sessions)
      base = [preprocess.Preprocessor('eeg', 1000, 100, **KW) for _ in range(sessions)]
      assert front.sections == 7
      t_new, t_old = [], []
      for i in range(total):
        lo, hi = i * n, (i + 1) * n
        chunk = x[:, lo:hi] if x is not None else raw[lo:hi].unsqueeze(0).expand(sessions, n, C).contiguous()
        h.synchronize()
        t0 = time.perf_counter()
        front.push(chunk)
        h.synchronize()
        t1 = time.perf_counter()
        for s in range(sessions):
          base[s].process(chunk[s], reset=i == 0)
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      row = dict(sessions=sessions, n=n, pushes=len(t_new),
                 frontend_us=[float(np.median(t_new)), float(np.min(t_new)), float(np.max(t_new))],
                 baseline_us=[float(np.median(t_old)), float(np.min(t_old)), float(np.max(t_old))])
      rows.append(row)
      print('S = %2d  n = %4d   front end %8.1f us (%.1f - %.1f)   Preprocessor.process x S %10.1f us (%.1f - %.1f)' %
            ((sessions, n) + tuple(row['frontend_us']) + tuple(row['baseline_us'])), flush=True)
  print(json.dumps({'tool': 'time_online_pre', 'channels': C, 'sections': 7, 'rates': [1000, 100], 'rows': rows}))


if __name__ == '__main__':
  main()
