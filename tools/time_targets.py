"""The targets pass of the C2 fit, float32 kernel against float16 kernel against a yardstick that is
neither: td_chan_max, a kernel that only reads x and takes the channel maxima.  ONE process,
interleaved rounds, hipEvents on the launching stream; on a stream that carries the pipeline's
accumulate mask (the last 192 CUs of 256) and on the whole chip.  Median and minimum of each.

  python tools/time_targets.py [--rounds 12] [--reps 10] [--arm both|mask|whole] [--json PATH]

What an event pair brackets: `reps` calls of LagStats.accumulate(parts = TARGETS | TARGETS_FIRST)
-- the targets launch AND the finalize launch that reduces its slabs (the same launch in both arms:
the difference of the two arms is the difference of the targets kernels; their ratio to td_chan_max
is not the kernels' ratio) -- or `reps` calls of td_chan_max.  The kernels alone: run this tool under
rocprofv3 --kernel-trace --stats with --arm mask or --arm whole and read the three kernels' lines
(lagcov_targets_mfma_kernel, lagcov_targets_split_kernel, chan_max_kernel*)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from telluride_decoding_amd import _lib, device

CHAN_MAX = '_Z11td_chan_maxP9td_handlePKflixxPj'     # td_chan_max (td_common.h): internal, C++ linkage


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=12)
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--arm', default='both', choices=('both', 'mask', 'whole'))
  ap.add_argument('--json', default=None)
  args = ap.parse_args()
  lib = _lib.load()
  chan_max = getattr(lib, CHAN_MAX)
  chan_max.restype = ctypes.c_int
  chan_max.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_longlong,
                       ctypes.c_longlong, ctypes.c_void_p]
  dev = torch.cuda.current_device()
  n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
  torch.manual_seed(0)
  n, c = 1000000, 64
  x = torch.randn(n, c, device='cuda')
  y = torch.randn(n, 1, device='cuda')
  offs = np.arange(11, dtype=np.int64) * 100000
  out = {'what': 'C2 targets pass (1e6 x 64 float32 + 1e6 targets, 32 lags): us per call, hipEvents, %d rounds x %d '
                 'reps interleaved in one process; f32 / f16 = accumulate(parts = targets first): the targets '
                 'launch + its finalize launch; chan_max = td_chan_max over the same x' % (args.rounds, args.reps)}
  keep = []
  for arm in ('mask', 'whole'):
    if args.arm not in ('both', arm):
      continue
    if arm == 'mask':
      p = ctypes.c_void_p()
      _lib.check(None, lib.td_stream_create_masked(dev, n_cu // 4, n_cu - n_cu // 4, ctypes.byref(p)))
      keep.append(p)
      stream = torch.cuda.ExternalStream(p.value)
    else:
      stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
      h = device.Handle()
      if arm == 'mask':
        h.check(lib.td_set_cu_count(h.ptr, n_cu - n_cu // 4))
      st = device.LagStats(c, 0, 31, d=1, handle=h)
      tab = torch.zeros(17 * 128, dtype=torch.int32, device='cuda')

      def run(kind):
        if kind == 'chan_max':
          tab.zero_()
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record(stream)
          for _ in range(args.reps):
            h.check(chan_max(h.ptr, x.data_ptr(), c, c, 0, n, tab.data_ptr()))
          e1.record(stream)
        else:
          h.set_option('targets_f16', 1 if kind == 'f16' else 0)
          st.reset()
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record(stream)
          for _ in range(args.reps):
            st.accumulate(x, None, y, offs, parts=2 | 4)
          e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.reps

      kinds = ('f32', 'f16', 'chan_max')
      for k in kinds:
        run(k)
      times = {k: [] for k in kinds}
      for _ in range(args.rounds):
        for k in kinds:
          times[k].append(run(k))
      h.set_option('targets_f16', 1)
      res = {k: {'median_us': float(np.median(v)), 'min_us': float(np.min(v)), 'max_us': float(np.max(v))}
             for k, v in times.items()}
      res['f16_over_f32_median'] = res['f16']['median_us'] / res['f32']['median_us']
      res['f32_minus_f16_median_us'] = res['f32']['median_us'] - res['f16']['median_us']
      res['cus'] = n_cu - n_cu // 4 if arm == 'mask' else n_cu
      out[arm] = res
      print('%-5s (%3d CUs): f32 %.1f (min %.1f)  f16 %.1f (min %.1f)  chan_max %.1f (min %.1f) us' % (
          arm, res['cus'], res['f32']['median_us'], res['f32']['min_us'], res['f16']['median_us'],
          res['f16']['min_us'], res['chan_max']['median_us'], res['chan_max']['min_us']))
      del st, h          # (before the stream they queue on goes away)
    torch.cuda.synchronize()
  for p in keep:
    lib.td_stream_destroy(p)
  if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, 'w') as f:
      json.dump(out, f, indent=1)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
