"""The CCA leave-one-file-out x lambda sweep at the RegressionCCA preset shape (64 channels x 22 lags of EEG against
31 lags of one intensity channel, batch 100, 5 dimensions, 32 files x 20 000 frames, lambda = 1e-1 .. 1e7): the
batched sweep against the forced per-fold route (existing calls only: what the code could do without the sweep), in
ONE process, wall clock around regression.jackknife_over_regularizations (the call ends with the scores on the host).

  python tools/time_cca_sweep.py [--sweeps 11] [--per-fold-sweeps 11] [--files 32] [--frames 20000] [--json PATH]

Prints the first sweep of each route apart from the median of the following ones, the spread of those (min, max),
what regression.LAST_SWEEP reports, and the largest distance between the two routes' results.  The kernels alone: run
the tool under rocprofv3 --kernel-trace --stats (no counters in that run) with --per-fold-sweeps 0."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from telluride_decoding_amd import brain_data, device, regression, synth


def timed(fn, h):
  h.synchronize()
  t0 = time.perf_counter()
  out = fn()
  h.synchronize()
  return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
  rest = ms[1:]
  return {'first_ms': ms[0], 'median_ms': float(np.median(rest)) if rest else None,
          'min_ms': float(np.min(rest)) if rest else None, 'max_ms': float(np.max(rest)) if rest else None,
          'sweeps_after_first': len(rest)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--sweeps', type=int, default=11)
  ap.add_argument('--per-fold-sweeps', type=int, default=11)
  ap.add_argument('--files', type=int, default=32)
  ap.add_argument('--frames', type=int, default=20000)
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  trials = synth.make_trials(11, args.files, args.frames, 64)
  files = [(eeg, env[:, :1].copy(), env[:, :1].copy(), att) for eeg, env, att in trials]
  ds = brain_data.Dataset(files, 100, 0, 21, 15, 15)
  lambdas = [10.0 ** k for k in range(-1, 8)]
  h = device.default_handle()
  ds.device_arrays(h)                                  # (the upload is not the sweep's)
  result = {'shape': {'files': args.files, 'frames': args.frames, 'k1': 64 * 22, 'k2': 31, 'lambdas': len(lambdas),
                      'dim': 5, 'batch': 100}}
  runs = {}
  for name, route, n in (('batched', None, args.sweeps), ('per_fold', 'per_fold', args.per_fold_sweeps)):
    ms = []
    for _ in range(n):
      t, res = timed(lambda: regression.jackknife_over_regularizations(ds, lambdas, model='cca', cca_dims=5,
                                                                       _route=route), h)
      ms.append(t)
      runs[name] = res['all_runs']
    if n:
      result[name] = summary(ms)
      result[name]['last_sweep'] = {k: regression.LAST_SWEEP.get(k) for k in ('cca_route', 'cca_pairs')}
  if len(runs) == 2:
    result['max_distance_between_routes'] = float(np.nanmax(np.abs(runs['batched'] - runs['per_fold'])))
  if 'batched' in runs:
    result['mean_r_per_lambda'] = [float(v) for v in np.nanmean(runs['batched'], axis=1)]
  line = json.dumps(result)
  print(line)
  if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
