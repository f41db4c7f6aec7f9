"""Time per push of the online audio front end (td_audio_online_push) against what the library offered before it,
per session: AudioFeatures.compute_intensity on the same device-tensor chunk, its buffer carried.  A cost comparison
only: the baseline restarts its window centres on every call, so it computes a different, cut-dependent envelope.

  python tools/time_online_audio.py [--pushes 200] [--warmup 20]

16 kHz stereo int16 -> 64 Hz, window 1; S in {1, 64} sessions and n in {160, 1600, 16000} rows per push.  Every push
is timed on its own between device synchronisations; reported: the median and the range over the pushes after the
warm-up, in microseconds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from telluride_decoding_amd import device, online, preprocess

FS_IN, FS_OUT, WINDOW, C = 16000, 64, 1, 2


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--pushes', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=20)
  args = ap.parse_args()
  import torch
  h = device.default_handle()
  rng = np.random.default_rng(0)
  rows = []
  for sessions in (1, 64):
    for n in (160, 1600, 16000):
      total = args.warmup + args.pushes
      # the same `total` chunks over again for every session: only the time matters
      pcm = torch.from_numpy(rng.integers(-20000, 20001, size=(total * n, C)).astype(np.int16)).to(h.device)
      front = online.OnlineAudioFeatures(preprocess.AudioFeatures('audio', FS_IN, FS_OUT, WINDOW),
                                         num_sessions=sessions)
      base = [preprocess.AudioFeatures('audio', FS_IN, FS_OUT, WINDOW) for _ in range(sessions)]
      t_new, t_old = [], []
      for i in range(total):
        chunk = pcm[i * n:(i + 1) * n].unsqueeze(0).expand(sessions, n, C).contiguous()
        h.synchronize()
        t0 = time.perf_counter()
        front.push(chunk)
        h.synchronize()
        t1 = time.perf_counter()
        for s in range(sessions):
          base[s].compute_intensity(chunk[s])
        h.synchronize()
        t2 = time.perf_counter()
        if i >= args.warmup:
          t_new.append(1e6 * (t1 - t0))
          t_old.append(1e6 * (t2 - t1))
      row = dict(sessions=sessions, n=n, pushes=len(t_new),
                 online_us=[float(np.median(t_new)), float(np.min(t_new)), float(np.max(t_new))],
                 baseline_us=[float(np.median(t_old)), float(np.min(t_old)), float(np.max(t_old))])
      rows.append(row)
      print('S = %2d  n = %5d   online %8.1f us (%.1f - %.1f)   compute_intensity x S %10.1f us (%.1f - %.1f)' %
            ((sessions, n) + tuple(row['online_us']) + tuple(row['baseline_us'])), flush=True)
  print(json.dumps({'tool': 'time_online_audio', 'channels': C, 'rates': [FS_IN, FS_OUT], 'window': WINDOW,
                    'rows': rows}))


if __name__ == '__main__':
  main()
