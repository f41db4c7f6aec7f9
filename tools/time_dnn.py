"""Times BrainModelDNN.fit (td_mlp_train, td_mlp_train_loss) against the same training in torch eager on the
same GPU.

hipEvents around whole fit calls on device-resident data, after a warm-up fit of the same shape; the torch
baseline is autograd + torch.optim.RMSprop(alpha=0.9, eps=1e-7) on the lagged input, materialised outside the
timed region.  Shapes:
  codelab  64 channels, pre 15 / post 21 (K = 2368), [20, 20], D = 1, B = 512, 40 x 6000 frames (468 steps);
  ref      2 channels, no context, [40, 20, 10], D = 1, B = 1000, 10000 frames (10 steps).
--loss mse (default), pearson, or both: with both, every repetition times an mse fit and then a Pearson fit,
so the two alternate within the call; torch eager is timed on the mse only.
Prints one JSON line per measurement.  Needs an MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dataset(files, c, pre, post, batch):
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(0)
  out = []
  for n in files:
    x = rng.standard_normal((n, c)).astype(np.float32)
    y = np.sin(x[:, :1] * 2 * np.pi).astype(np.float32)
    z = np.zeros((n, 1), np.float32)
    out.append((x, z, y, z))
  return brain_data.Dataset(out, batch, pre, post)


def _events():
  import torch
  return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def time_hip(ds, hidden, epochs, reps, losses=('mse',)):
  """{loss: (median ms, [ms of every repetition])}; the losses alternate within each repetition."""
  import torch
  from telluride_decoding_amd import brain_model, device
  h = device.default_handle()
  ds.device_arrays(h)
  models = {}
  for loss in losses:
    m = brain_model.BrainModelDNN(ds, hidden)
    m.compile(loss=loss)
    m.fit(ds, epochs=1)                   # warm-up: code objects, scratch, device copies
    models[loss] = m
  torch.cuda.synchronize()
  times = {loss: [] for loss in losses}
  for _ in range(reps):
    for loss in losses:
      a, b = _events()
      a.record()
      models[loss].fit(ds, epochs=epochs)
      b.record()
      b.synchronize()
      times[loss].append(a.elapsed_time(b))
  return {loss: (float(np.median(t)), t) for loss, t in times.items()}


def time_torch(ds, hidden, epochs, reps):
  import torch
  from telluride_decoding_amd import brain_model
  dev = torch.device('cuda')
  x = torch.from_numpy(np.concatenate([f['input_1'] for f, _ in ds])).to(dev)
  y = torch.from_numpy(np.concatenate([t for _, t in ds])).to(dev)
  widths = [x.shape[1]] + hidden + [y.shape[1]]
  w0 = brain_model.BrainModelDNN(ds, hidden).get_weights()
  b = ds.batch_size
  steps = x.shape[0] // b

  def run(n_epochs):
    params = [torch.tensor(w, device=dev, requires_grad=True) for w in w0]
    opt = torch.optim.RMSprop(params, lr=1e-3, alpha=0.9, eps=1e-7)
    for _ in range(n_epochs):
      for s in range(steps):
        a = x[s * b:(s + 1) * b]
        for l in range(len(widths) - 1):
          a = a @ params[2 * l] + params[2 * l + 1]
          if l < len(widths) - 2:
            a = torch.relu(a)
        loss = torch.mean((a - y[s * b:(s + 1) * b]) ** 2)
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
  ap.add_argument('--torch-epochs', type=int, default=2, help='0: skip the torch eager baseline')
  ap.add_argument('--loss', choices=('mse', 'pearson', 'both'), default='mse')
  args = ap.parse_args()
  losses = ('mse', 'pearson') if args.loss == 'both' else (args.loss,)
  codelab = _dataset([6000] * 40, 64, 15, 21, 512)
  ref = _dataset([10000], 2, 0, 0, 1000)
  for name, ds, hidden, epoch_list in (('codelab', codelab, [20, 20], (10, 100)), ('ref', ref, [40, 20, 10], (100,))):
    steps = ds.num_batches()
    for epochs in epoch_list:
      for loss, (ms, every) in time_hip(ds, hidden, epochs, args.reps, losses).items():
        print(json.dumps({'shape': name, 'path': 'hip', 'loss': loss, 'epochs': epochs, 'steps_per_epoch': steps,
                          'fit_ms': ms, 'us_per_step': 1e3 * ms / (epochs * steps), 'ms_per_epoch': ms / epochs,
                          'fit_ms_all': every}), flush=True)
    if args.torch_epochs <= 0:
      continue
    ms, steps = time_torch(ds, hidden, args.torch_epochs, args.reps)
    print(json.dumps({'shape': name, 'path': 'torch_eager', 'epochs': args.torch_epochs, 'steps_per_epoch': steps,
                      'fit_ms': ms, 'us_per_step': 1e3 * ms / (args.torch_epochs * steps),
                      'ms_per_epoch': ms / args.torch_epochs}), flush=True)


if __name__ == '__main__':
  main()
