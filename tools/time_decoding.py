"""Times the correlation + LDA stage of a decoding experiment at the driver's default window:
Decoder.train(mixed, matched, window_size=100) for a LinearRegressionDecoder around a fitted
BrainModelLinearRegression (decoding.train_lda_model, correlation_frames = 100).

1e6 frames per class (10 recordings of 1e5 frames, 8 channels, no context), 1, 5 and 8 output columns, on
device-resident Datasets (the recordings are uploaded, and the mixed-up dataset resolved, by the warm-up
call).  Wall-clock time around a device synchronise, the median of --reps calls after one warm-up call; a
fresh decoder per call, so every call accumulates its statistics from zero.  Only calls that every version
of the package since the decoder's device fast path has, so the same file times an older checkout too.
Prints one JSON line per shape.  Needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _files(num_files, frames, channels, outputs):
  rng = np.random.default_rng(0)
  w = rng.standard_normal((channels, outputs)).astype(np.float32)
  out = []
  for _ in range(num_files):
    x = rng.standard_normal((frames, channels)).astype(np.float32)
    y = (x @ w + rng.standard_normal((frames, outputs))).astype(np.float32)
    z = np.zeros((frames, 1), np.float32)
    out.append((x, z, y, z))
  return out


def time_train(outputs, window, reps, num_files=10, frames=100000, channels=8, batch=1000):
  import torch
  from telluride_decoding_amd import brain_data, brain_model, device, infer_decoder
  files = _files(num_files, frames, channels, outputs)
  matched = brain_data.Dataset(files, batch)
  mixed = brain_data.Dataset(files, batch, mixup_batch=True)
  model = brain_model.BrainModelLinearRegression(matched, regularization_lambda=0.1)
  model.fit(matched)
  device.default_handle()

  def one():
    dec = infer_decoder.LinearRegressionDecoder(model, reduction='lda')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dprime = dec.train(mixed, matched, window_size=window)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), float(dprime)
  one()                                    # warm-up: uploads, the resolved mixed-up dataset, code objects
  runs = [one() for _ in range(reps)]
  ms = [r[0] for r in runs]
  return {'outputs': outputs, 'window': window, 'frames_per_class': num_files * frames,
          'train_ms': float(np.median(ms)), 'train_ms_all': ms, 'dprime': runs[-1][1]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--window', type=int, default=100)
  ap.add_argument('--outputs', type=int, nargs='*', default=[1, 5, 8])
  ap.add_argument('--frames', type=int, default=100000, help='frames per recording (10 recordings per class)')
  args = ap.parse_args()
  for outputs in args.outputs:
    print(json.dumps(time_train(outputs, args.window, args.reps, frames=args.frames)), flush=True)


if __name__ == '__main__':
  main()
