"""Times a leave-one-file-out jackknife of BrainModelClassifier: every (learning rate, fold) trained by one
brain_model.fit_many and scored by one brain_model.evaluate_many (td_clf_train_many) against one
BrainModelClassifier.fit and one evaluate after another on Datasets of each fold's recordings (what
regression.jackknife_classifier's 'per_fold' route does; the only way before fit_many took classifiers).

hipEvents around whole sweeps (training and scoring of all models) on device-resident data -- the full dataset, every
fold's training Dataset and every held-out Dataset are uploaded first -- after a warm-up sweep of each route, median
of --reps.  Models are rebuilt (same seed) outside the timed region.  Shapes, 10 recordings x 2 learning rates each:
  mm   DESIGN section 15's shape (a) cut to a jackknife: 64 channels x 37 lags plus a 1-channel envelope x 37 lags
       (K = 2405), [20, 20], D = 1, B = 512, 10 x 6000 frames (105 steps an epoch and fold), 2 epochs;
  ref  its shape (b): 3 + 2 context-free inputs, [20], D = 1, B = 128, 10 x 1000 frames (70 steps), 5 epochs.
--route per_fold uses nothing but the public fit / evaluate, so the same file times a checkout from before
fit_many took classifiers (the baseline of "one fit after another" is that commit: the single fit's code was touched
since).  Prints one JSON line per measurement.  Needs an MI355X: without one the first device call raises."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATES = [1e-3, 3e-3]
SHAPES = {'mm': dict(files=[6000] * 10, c=64, pre=15, post=21, c2=1, pre2=15, post2=21, batch=512, hidden=[20, 20],
                     epochs=2),
          'ref': dict(files=[1000] * 10, c=3, pre=0, post=0, c2=2, pre2=0, post2=0, batch=128, hidden=[20], epochs=5)}


def _files(shape):
  rng = np.random.default_rng(0)
  out = []
  for n in shape['files']:
    x = rng.standard_normal((n, shape['c'])).astype(np.float32)
    y = (rng.standard_normal((n, 1)) > 0.5).astype(np.float32)
    x2 = (y * 2 * x[:, :shape['c2']] + (1 - y) * rng.standard_normal((n, shape['c2']))).astype(np.float32)
    out.append((x, x2, y, np.zeros((n, 1), np.float32)))
  return out


def _dataset(files, shape):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(files, shape['batch'], shape['pre'], shape['post'], shape['pre2'], shape['post2'])


def _models(ds, shape, n_folds, h):
  """[learning rate][fold], compiled, parameters on the device."""
  from telluride_decoding_amd import brain_model
  grid = []
  for lr in RATES:
    row = [brain_model.BrainModelClassifier(ds, shape['hidden'], seed=0) for _ in range(n_folds)]
    for m in row:
      m.compile(optimizer=brain_model.Adam(learning_rate=lr))
      m._device_params(h)
    grid.append(row)
  return grid


def _timed(fn):
  import torch
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  out = fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b), out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--route', choices=('both', 'per_fold', 'batched'), default='both')
  ap.add_argument('--shapes', default='mm,ref')
  args = ap.parse_args()
  from telluride_decoding_amd import brain_model, device
  h = device.default_handle()                      # (raises without a GPU: there is no fallback)
  routes = ['per_fold', 'batched'] if args.route == 'both' else [args.route]
  for name in [s for s in args.shapes.split(',') if s]:
    shape = SHAPES[name]
    files = _files(shape)
    folds = list(range(len(files)))
    ds = _dataset(files, shape)
    train = [_dataset([files[g] for g in folds if g != f], shape) for f in folds]
    held = [_dataset([files[f]], shape) for f in folds]
    for d in [ds] + train + held:
      d.device_arrays(h)
    epochs = shape['epochs']

    def per_fold(grid):
      scores = []
      for row in grid:
        for m, tr, he in zip(row, train, held):
          m.fit(tr, epochs=epochs)
          scores.append(m.evaluate(he)['accuracy'])
      return scores

    def batched(grid):
      flat = [m for row in grid for m in row]
      brain_model.fit_many(flat, ds, held_out=[[f] for _ in RATES for f in folds], epochs=epochs)
      return [s['accuracy'] for s in brain_model.evaluate_many(flat, ds, files=[[f] for _ in RATES for f in folds])]

    run = {'per_fold': per_fold, 'batched': batched}
    warm = {r: run[r](_models(ds, shape, len(folds), h)) for r in routes}        # code objects, scratch
    if len(routes) == 2 and warm['per_fold'] != warm['batched']:
      raise SystemExit('the two routes do not score alike')
    times = {r: [] for r in routes}
    for _ in range(args.reps):
      for r in routes:                                                             # the routes alternate
        grid = _models(ds, shape, len(folds), h)
        times[r].append(_timed(lambda: run[r](grid))[0])
    steps = train[0].num_batches()
    for r in routes:
      ms = times[r]
      print(json.dumps({'shape': name, 'route': r, 'models': len(RATES) * len(folds), 'epochs': epochs,
                        'steps_per_epoch': steps, 'sweep_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)),
                        'max_ms': float(np.max(ms)), 'all_ms': [float(v) for v in ms],
                        'us_per_model_step': 1e3 * float(np.median(ms)) / (len(RATES) * len(folds) * epochs * steps)}),
            flush=True)


if __name__ == '__main__':
  main()
