"""Times the ingest stage on the GPU against the host path.

Workload (the defaults): 40 trials x (64 EEG channels + 2 envelopes) x 1e5 frames, float32, as device tensors.
   python tools/time_ingest.py [--trials 40] [--frames 100000] [--host-frames 2000] [--repeats 5]

Prints one JSON object:
  device_wall_s      BrainExperiment.z_score_all_data + write_all_data through the device path (host clock; the
                     write ends in a copy to the host and a file write, so the device is idle when it stops)
  kernels            per entry point, device events (Handle.timer_start / timer_stop) around one call, the median
                     of --repeats after a warm-up: ms, the bytes the call has to read and write, GB/s, and
                     `of_copy` = its time over the time of a device-to-device copy that moves the same number of
                     bytes (a copy of n bytes reads n and writes n), timed the same way in this run
  host_wall_s        the host path -- tfrecord.write_file plus NumPy two-pass moments and normalisation, the only
                     route before the device path existed -- timed on --host-frames frames of one trial and scaled
                     to the workload (the Python writer is linear in the records: ~190 us each)
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--trials', type=int, default=40)
  ap.add_argument('--frames', type=int, default=100000)
  ap.add_argument('--channels', type=int, default=64)
  ap.add_argument('--envelopes', type=int, default=2)
  ap.add_argument('--host-frames', type=int, default=2000)
  ap.add_argument('--repeats', type=int, default=5)
  args = ap.parse_args()

  import torch
  from telluride_decoding_amd import device, ingest, tfrecord
  if not device.gpu_available():
    raise SystemExit('time_ingest needs a GPU: there is nothing to time without one')
  h = device.default_handle()
  gen = torch.Generator(device='cuda').manual_seed(1)

  def make(rows, width, offset):
    return offset + torch.randn((rows, width), generator=gen, device='cuda', dtype=torch.float32)

  trials = {}
  for t in range(args.trials):
    trials['trial_%02d' % t] = [{'eeg': make(args.frames, args.channels, 1e4),
                                 'envelope': make(args.frames, args.envelopes, 5.0)}]
  out_dir = tempfile.mkdtemp(prefix='time_ingest_')
  result = {'trials': args.trials, 'frames': args.frames, 'channels': args.channels, 'envelopes': args.envelopes}
  try:
    # ---- per kernel, against a copy of the same bytes
    def timed(fn):
      fn()
      h.synchronize()
      times = []
      for _ in range(args.repeats):
        h.timer_start()
        fn()
        times.append(h.timer_stop())
      return statistics.median(times)

    def copy_ms(nbytes):
      n = max(1, nbytes // 2)
      src = torch.empty(n, dtype=torch.uint8, device='cuda')
      dst = torch.empty_like(src)
      return timed(lambda: dst.copy_(src))

    eeg = [v[0]['eeg'] for v in trials.values()]
    one = eeg[0]
    template, layout = ingest.device_record_plan({k: v for k, v in trials['trial_00'][0].items()})
    stride = len(template)
    feats = [(trials['trial_00'][0][k], off, False) for k, off, _ in layout]
    in_bytes = one.numel() * 4 + trials['trial_00'][0]['envelope'].numel() * 4
    kernels = {}
    for name, fn, nbytes in (
        ('moments (all trials, eeg)', lambda: device.ingest_moments(eeg), 2 * sum(e.numel() * 4 for e in eeg)),
        ('normalize (one trial, eeg)', lambda: device.ingest_normalize(one, 1e4, 1.0, False, False),
         2 * one.numel() * 4),
        ('encode (one trial)', lambda: device.tfrecord_encode(template, feats, args.frames),
         in_bytes + args.frames * stride)):
      ms, cms = timed(fn), copy_ms(nbytes)
      kernels[name] = {'ms': round(ms, 4), 'bytes': nbytes, 'GB_per_s': round(nbytes / ms / 1e6, 1),
                       'copy_ms': round(cms, 4), 'of_copy': round(ms / cms, 2)}
    result['kernels'] = kernels
    result['record_stride'] = stride
    result['route'] = device.tfrecord_route(stride)

    # ---- the host path, on a slice of one trial, scaled
    m = min(args.host_frames, args.frames)
    host = {k: v[:m].cpu().numpy() for k, v in trials['trial_00'][0].items()}
    t0 = time.perf_counter()
    for k, v in host.items():
      mean = np.sum(v, dtype=np.float64) / v.size
      std = np.sqrt(np.sum((v.astype(np.float64) - mean) ** 2) / v.size)
      host[k] = ((v - mean) / std).astype(np.float32)
    t1 = time.perf_counter()
    tfrecord.write_file(os.path.join(out_dir, 'host.tfrecords'), host)
    t2 = time.perf_counter()
    scale = args.trials * args.frames / float(m)
    result['host_frames_timed'] = m
    result['host_us_per_record'] = round((t2 - t1) / m * 1e6, 1)
    result['host_wall_s'] = round((t2 - t0) * scale, 1)

    # ---- the device path, whole workload, wall time
    exp = ingest.BrainExperiment(trials, out_dir, out_dir)
    exp.load_all_data()
    h.synchronize()
    t0 = time.perf_counter()
    exp.z_score_all_data()
    h.synchronize()
    t1 = time.perf_counter()
    files = exp.write_all_data(out_dir)
    t2 = time.perf_counter()
    result['device_zscore_s'] = round(t1 - t0, 3)
    result['device_write_s'] = round(t2 - t1, 3)
    result['device_wall_s'] = round(t2 - t0, 3)
    result['file_bytes'] = sum(os.path.getsize(f) for f in files)
    result['speedup'] = round(result['host_wall_s'] / result['device_wall_s'], 1)
    count, bad = ingest.count_tfrecords(files[0]) if args.frames <= 5000 else (args.frames, False)
    assert count == args.frames and not bad
  finally:
    shutil.rmtree(out_dir, ignore_errors=True)
  print(json.dumps(result))


if __name__ == '__main__':
  main()
