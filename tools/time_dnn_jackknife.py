"""Times the training of a BrainModelDNN jackknife: all folds in one brain_model.fit_many call (td_dnn_train_many)
against one BrainModelDNN.fit after another on a Dataset of each fold's recordings (what regression.jackknife_dnn's
'per_fold' route does; the only way before fit_many).

Shape: the codelab shape -- 64 channels, pre 15 / post 21 (37 lags, K = 2368), [20, 20], D = 1,
B = 512 -- on 8 recordings of about 30 000 frames, so 8 folds of about 410 steps an epoch, 2 epochs.  Everything is
resident on the device before the clock starts: the full dataset and the eight fold datasets are uploaded, and both
routes have run once (code objects, scratch).  A synchronised host clock around whole calls; the two routes alternate
within every repetition.  Models are rebuilt (same seed) outside the timed region, so every repetition trains from
the same weights.

Then a scan: fit_many of 1, 2, 4, 8 and 16 models on the full dataset (no fold held out), to show where the chip
saturates; ms per call and per model.

Prints one JSON line per measurement.  Needs an MI355X: without one the first device call raises."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, PRE, POST, HIDDEN, BATCH = 64, 15, 21, [20, 20], 512


def _files(lengths):
  rng = np.random.default_rng(0)
  out = []
  for n in lengths:
    x = rng.standard_normal((n, C)).astype(np.float32)
    y = np.sin(x[:, :1] * 2 * np.pi).astype(np.float32)
    z = np.zeros((n, 1), np.float32)
    out.append((x, z, y, z))
  return out


def _models(ds, n, loss, lr=1e-3):
  from telluride_decoding_amd import brain_model
  models = []
  for _ in range(n):
    m = brain_model.BrainModelDNN(ds, HIDDEN, seed=0)
    m.compile(optimizer=brain_model.RMSprop(learning_rate=lr), loss=loss)
    models.append(m)
  return models


def _timed(fn):
  import torch
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0)


def _summary(ms):
  return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)),
          'spread_ms': float(np.max(ms) - np.min(ms)), 'all_ms': [float(v) for v in ms]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--epochs', type=int, default=2)
  ap.add_argument('--loss', choices=('mse', 'pearson'), default='mse')
  ap.add_argument('--shuffle-seed', type=int, default=None)
  ap.add_argument('--scan', default='1,2,4,8,16')
  args = ap.parse_args()
  if args.reps < 5:
    ap.error('at least 5 repetitions')
  from telluride_decoding_amd import brain_data, brain_model, device
  h = device.default_handle()                      # (raises without a GPU: there is no fallback)
  lengths = [30000 + 250 * (i - 4) for i in range(8)]
  files = _files(lengths)
  ds = brain_data.Dataset(files, BATCH, PRE, POST)
  ds.device_arrays(h)
  folds = list(range(len(files)))
  held = [[f] for f in folds]
  fold_ds = [brain_data.Dataset([files[g] for g in folds if g != f], BATCH, PRE, POST) for f in folds]
  for fd in fold_ds:
    fd.device_arrays(h)
  steps = [sum(brain_model.fold_rows_used(ds, hf)) // BATCH for hf in held]

  def batched(models):
    brain_model.fit_many(models, ds, held_out=held, epochs=args.epochs, shuffle_seeds=args.shuffle_seed)

  def per_fold(models):
    for m, fd in zip(models, fold_ds):
      m.fit(fd, epochs=args.epochs, shuffle_seed=args.shuffle_seed)

  # warm-up of both routes, which must also agree bit for bit
  a, b = _models(ds, len(folds), args.loss), _models(ds, len(folds), args.loss)
  batched(a)
  per_fold(b)
  same = all(np.array_equal(u, v) for ma, mb in zip(a, b) for u, v in zip(ma.get_weights(), mb.get_weights()))
  if not same:
    raise SystemExit('the two routes do not agree bit for bit')
  times = {'batched': [], 'per_fold': []}
  for _ in range(args.reps):
    for name, fn in (('batched', batched), ('per_fold', per_fold)):
      models = _models(ds, len(folds), args.loss)
      for m in models:
        m._device_params(h)
      times[name].append(_timed(lambda: fn(models)))
  base = {'shape': 'codelab x 8 recordings', 'loss': args.loss, 'epochs': args.epochs, 'folds': len(folds),
          'steps_per_epoch': steps, 'shuffle_seed': args.shuffle_seed, 'routes_agree_bitwise': same}
  for name in ('batched', 'per_fold'):
    print(json.dumps(dict(base, route=name, **_summary(times[name]))), flush=True)
  tb, tp = np.median(times['batched']), np.median(times['per_fold'])
  spread = float(np.max(times['per_fold']) - np.min(times['per_fold']))
  print(json.dumps({'per_fold_over_batched': float(tp / tb), 'difference_ms': float(tp - tb),
                    'per_fold_spread_ms': spread,
                    'faster_by_more_than_the_spread': 'batched' if tp - tb > spread else
                    'per_fold' if tb - tp > spread else 'neither'}), flush=True)
  # the scan: n models on the full dataset
  full_steps = ds.num_batches()
  for n in [int(v) for v in args.scan.split(',') if v]:
    _models_n = lambda: _models(ds, n, args.loss)
    brain_model.fit_many(_models_n(), ds, epochs=1)
    ms = []
    for _ in range(args.reps):
      models = _models_n()
      for m in models:
        m._device_params(h)
      ms.append(_timed(lambda: brain_model.fit_many(models, ds, epochs=args.epochs,
                                                    shuffle_seeds=args.shuffle_seed)))
    s = _summary(ms)
    print(json.dumps(dict({'scan_models': n, 'steps_per_epoch': full_steps, 'epochs': args.epochs,
                           'ms_per_model': s['median_ms'] / n,
                           'us_per_round': 1e3 * s['median_ms'] / (args.epochs * full_steps)}, **s)), flush=True)


if __name__ == '__main__':
  main()
