"""Time per push of the online CCA fit (td_ccafit_online_push) against the route the library had before it: keep every
row so far and, per push and session, LagStats.reset + LagStats.accumulate over all of them (the batch accumulate
treats a call's rows as whole files, so a chunk cannot be added on its own); and td_ccafit_online_solve against
reset + accumulate + LagStats.cca_solve on those rows, for 1 and 3 lambdas at 5 dims.

  python tools/time_online_cca_fit.py [--pushes 50] [--warmup 10] [--solves 20] [--solve-warmup 3]

64 channels x 21 lags (post context 20) against 8 features x 16 lags (post context 15): n = 1473; S in {1, 64}
sessions and n in {10, 100} rows per push.  Every push is timed on its own between device synchronisations, both
routes in the same run; the baseline's history grows with every push, so its range is wide by construction (its first
timed push covers (warmup + 1) n rows, its last (warmup + pushes) n).  Reported: the median and the range over the
pushes after the warm-up, in microseconds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import device

VIEWS = (64, 0, 20, 8, 0, 15)               # c1, pre1, post1, c2, pre2, post2
DIMS = 5


def _spread(values):
  return [float(np.median(values)), float(np.min(values)), float(np.max(values))]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=50)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--solves', type=int, default=20)
  ap.add_argument('--solve-warmup', type=int, default=3)
  args = ap.parse_args()
  h = device.default_handle()
  rng = np.random.default_rng(0)
  c1, pre1, post1, c2, pre2, post2 = VIEWS
  delay = max(post1, post2)
  nbytes = device.online_ccafit_state_bytes(*VIEWS)
  total = args.warmup + args.pushes
  rows = []
  for sessions in (1, 64):
    for n in (10, 100):
      # (one shared source per session, so that the two views correlate and the dense stage has something to find)
      src = rng.standard_normal((sessions * total * n, 4))
      eeg = (src @ rng.standard_normal((4, c1)) + rng.standard_normal((sessions * total * n, c1))).astype(np.float32)
      feat = (src @ rng.standard_normal((4, c2)) + 0.5 * rng.standard_normal((sessions * total * n, c2))).astype(
          np.float32)
      eeg = h.to_device(eeg).reshape(sessions, total * n, c1)
      feat = h.to_device(feat).reshape(sessions, total * n, c2)
      state = torch.zeros((sessions, nbytes), dtype=torch.uint8, device=h.device)
      stats = [device.LagStats(*VIEWS, handle=h) for _ in range(sessions)]
      t_new, t_old = [], []
      for i in range(total):
        lo, hi = i * n, (i + 1) * n
        h.synchronize()
        t0 = time.perf_counter()
        device.online_ccafit_push(eeg[:, lo:hi], feat[:, lo:hi], state, lo, i, pre1, post1, pre2, post2, handle=h)
        h.synchronize()
        t1 = time.perf_counter()
        for s in range(sessions):
          stats[s].reset()
          stats[s].accumulate(eeg[s, :hi], feat[s, :hi], None, [0, hi])
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      row = dict(what='push', sessions=sessions, n=n, pushes=len(t_new), online_us=_spread(t_new),
                 baseline_us=_spread(t_old))
      rows.append(row)
      print('push   S = %2d  n = %3d   online %9.1f us (%.1f - %.1f)   baseline %10.1f us (%.1f - %.1f)' %
            ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us'])), flush=True)
      if sessions == 1 and n == 100:
        rows_all = total * n
        frames = rows_all - delay
        for lambdas in ([1.0], [0.1, 1.0, 10.0]):
          t_new, t_old = [], []
          for i in range(args.solve_warmup + args.solves):
            h.synchronize()
            t0 = time.perf_counter()
            device.online_ccafit_solve(state, *VIEWS, frames, lambdas, DIMS, handle=h)
            h.synchronize()
            t1 = time.perf_counter()
            stats[0].reset()
            stats[0].accumulate(eeg[0, :rows_all], feat[0, :rows_all], None, [0, rows_all])
            for lam in lambdas:
              stats[0].cca_solve(rows_all - 1, lam, DIMS)
            h.synchronize()
            t2 = time.perf_counter()
            if i >= args.solve_warmup:
              t_new.append(1e6 * (t1 - t0))
              t_old.append(1e6 * (t2 - t1))
          row = dict(what='solve', sessions=1, lambdas=len(lambdas), dims=DIMS, solves=len(t_new),
                     online_us=_spread(t_new), baseline_us=_spread(t_old))
          rows.append(row)
          print('solve  S =  1  lambdas = %d   online %9.1f us (%.1f - %.1f)   baseline %10.1f us (%.1f - %.1f)' %
                ((len(lambdas),) + tuple(row['online_us']) + tuple(row['baseline_us'])), flush=True)
      del stats, state, eeg, feat
  print(json.dumps({'tool': 'time_online_cca_fit', 'views': VIEWS, 'dims': DIMS, 'rows': rows}))


if __name__ == '__main__':
  main()
