"""Times BrainModelClassifier.fit (td_mlpc_train) against the same training in torch eager on the same GPU.

hipEvents around whole fit calls on device-resident data, after a warm-up fit of the same shape, median of
--reps; the torch baseline is autograd + torch.optim.Adam(eps=1e-7) + BCEWithLogitsLoss on the concatenated lag
matrix, materialised outside the timed region.  Shapes:
  mm   64 channels x 37 lags (pre 15 / post 21) plus a 1-channel envelope x 37 lags (K = 2405), [20, 20], D = 1,
       B = 512, 40 x 6000 frames (468 steps);
  ref  the reference test's: 3 + 2 context-free inputs, [20], D = 1, B = 128, 1000 frames (7 steps).
Prints one JSON line per measurement.  Needs an MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dataset(files, c, pre, post, c2, pre2, post2, batch):
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(0)
  out = []
  for n in files:
    x = rng.standard_normal((n, c)).astype(np.float32)
    y = (rng.standard_normal((n, 1)) > 0.5).astype(np.float32)
    x2 = (y * 2 * x[:, :c2] + (1 - y) * rng.standard_normal((n, c2))).astype(np.float32)
    out.append((x, x2, y, np.zeros((n, 1), np.float32)))
  return brain_data.Dataset(out, batch, pre, post, pre2, post2)


def _events():
  import torch
  return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def time_hip(ds, hidden, epochs, reps):
  import torch
  from telluride_decoding_amd import brain_model, device
  h = device.default_handle()
  ds.device_arrays(h)
  m = brain_model.BrainModelClassifier(ds, hidden)
  m.compile()
  m.fit(ds, epochs=1)                     # warm-up: code objects, scratch, device copies
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    a, b = _events()
    a.record()
    m.fit(ds, epochs=epochs)
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return float(np.median(times)), float(min(times)), float(max(times))


def time_torch(ds, hidden, epochs, reps):
  import torch
  from telluride_decoding_amd import brain_model
  dev = torch.device('cuda')
  x = torch.from_numpy(np.concatenate([np.concatenate([f['input_1'], f['input_2']], axis=1) for f, _ in ds])).to(dev)
  y = torch.from_numpy(np.concatenate([t for _, t in ds])).to(dev)
  widths = [x.shape[1]] + hidden + [y.shape[1]]
  w0 = brain_model.BrainModelClassifier(ds, hidden).get_weights()
  b = ds.batch_size
  steps = x.shape[0] // b
  loss_fn = torch.nn.BCEWithLogitsLoss()

  def run(n_epochs):
    params = [torch.tensor(w, device=dev, requires_grad=True) for w in w0]
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-7)
    for _ in range(n_epochs):
      for s in range(steps):
        a = x[s * b:(s + 1) * b]
        for l in range(len(widths) - 1):
          a = a @ params[2 * l] + params[2 * l + 1]
          if l < len(widths) - 2:
            a = torch.relu(a)
        loss = loss_fn(a, y[s * b:(s + 1) * b])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
  run(1)
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    e0, e1 = _events()
    e0.record()
    run(epochs)
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1))
  return float(np.median(times)), steps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--torch-epochs', type=int, default=2)
  args = ap.parse_args()
  mm = _dataset([6000] * 40, 64, 15, 21, 1, 15, 21, 512)
  ref = _dataset([1000], 3, 0, 0, 2, 0, 0, 128)
  for name, ds, hidden, epochs in (('mm', mm, [20, 20], 10), ('ref', ref, [20], 100)):
    steps = ds.num_batches()
    ms, lo, hi = time_hip(ds, hidden, epochs, args.reps)
    print(json.dumps({'shape': name, 'path': 'hip', 'epochs': epochs, 'steps_per_epoch': steps, 'fit_ms': ms,
                      'fit_ms_min': lo, 'fit_ms_max': hi, 'us_per_step': 1e3 * ms / (epochs * steps),
                      'ms_per_epoch': ms / epochs}), flush=True)
    t_epochs = args.torch_epochs if name == 'mm' else 10 * args.torch_epochs
    ms, steps = time_torch(ds, hidden, t_epochs, args.reps)
    print(json.dumps({'shape': name, 'path': 'torch_eager', 'epochs': t_epochs, 'steps_per_epoch': steps,
                      'fit_ms': ms, 'us_per_step': 1e3 * ms / (t_epochs * steps), 'ms_per_epoch': ms / t_epochs}),
          flush=True)


if __name__ == '__main__':
  main()
