"""P1 through the Preprocessor drop-in, hipEvents around whole process() calls: 64 ch x 1e6 frames at
1000 Hz (float32 on the device), high-pass 0.1 Hz order 4 + the automatic order-10 low-pass (7 sections),
resampled to 100 Hz, global re-reference, normalisation.  Prints the time per call against the HBM and
FP64 floors (estimates from the data sizes and the spec rates) and, where scipy
exists, against scipy's sosfilt + the reference's resample loop on 16 host threads.
   python tools/time_preprocess.py [--reps 20] [--no-host]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from telluride_decoding_amd import device  # noqa: E402
from telluride_decoding_amd import preprocess as pp  # noqa: E402
from tests import host_preprocess as hp  # noqa: E402

HBM_TBS = 6.3          # achievable stream rate (MI355X_MICROARCH: 6.29 TB/s measured copy)
FP64_TFLOPS = 78.6     # FP64 vector peak (spec)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--no-host', action='store_true')
  args = ap.parse_args()
  h = device.default_handle()
  x = hp.p1_input()
  n, c = x.shape
  t = torch.from_numpy(x).to(h.device)
  p = pp.Preprocessor('p1', hp.P1['fs_in'], hp.P1['fs_out'],
                      **{k: v for k, v in hp.P1.items() if k not in ('fs_in', 'fs_out')})
  for _ in range(3):
    y = p.process(t, reset=True)
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(args.reps):
    y = p.process(t, reset=True)
  e1.record()
  torch.cuda.synchronize()
  ms = e0.elapsed_time(e1) / args.reps
  s = p.sos.shape[0]
  m = int(y.shape[0])
  # floors: read x once, write the float32 output once; every (frame, channel, section) 5 multiply-adds
  bytes_min = n * c * 4 + m * c * 4
  flop_min = n * c * s * 10
  hbm_ms, fp64_ms = bytes_min / (HBM_TBS * 1e12) * 1e3, flop_min / (FP64_TFLOPS * 1e12) * 1e3
  # this design: x twice (chunk ends, outputs), y written + read, z written + read, output written
  bytes_design = 2 * n * c * 4 + 4 * m * c * 8 + m * c * 4
  res = {'case': 'P1', 'frames': n, 'channels': c, 'sections': s, 'out_rows': m, 'ms_per_call': round(ms, 4),
         'hbm_floor_ms_est': round(hbm_ms, 4), 'fp64_floor_ms_est': round(fp64_ms, 4),
         'design_bytes_floor_ms_est': round(bytes_design / (HBM_TBS * 1e12) * 1e3, 4),
         'fp64_two_pass_floor_ms_est': round(2 * fp64_ms, 4),
         'fraction_of_hbm_floor': round(hbm_ms / ms, 3), 'fraction_of_fp64_floor': round(fp64_ms / ms, 3)}
  if not args.no_host:
    try:
      import scipy.signal as ss
    except ImportError:
      ss = None
    if ss is not None:
      sos = p.sos
      zi = ss.sosfilt_zi(sos)
      cols = np.array_split(np.arange(c), 16)

      def run(cs):
        xs = x[:, cs].astype(np.float64)
        ys, _ = ss.sosfilt(sos, xs, zi=xs[0] * zi[:, :, None], axis=0)
        return ys

      t0 = time.perf_counter()
      with ThreadPoolExecutor(16) as ex:
        ys = np.concatenate(list(ex.map(run, cols)), axis=1)
      idx, _ = pp.resample_indices(n, hp.P1['fs_in'], hp.P1['fs_out'])
      out = np.zeros((len(idx), c))
      for i in range(len(idx)):             # the reference's per-row loop (preprocess.py:387-390)
        out[i, :] = ys[int(idx[i]), :]
      res['host_scipy_16_threads_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
  print(json.dumps(res))


if __name__ == '__main__':
  main()
