"""AudioFeatures on the device, hipEvents around whole calls on device tensors, against the reference's host
path restated (its per-frame np.mean loop; scipy's lfilter + stft where scipy imports):
  - compute_intensity, 60 s and 20 min of 44.1 kHz stereo float32 to 100 Hz (window 1, exponent log10(2));
  - compute_spectrogram of 60 s at 16 kHz with the reference's defaults.
Floors are estimates from the data sizes and the spec rates.
   python tools/time_audio.py [--reps 20] [--no-host]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from telluride_decoding_amd import device  # noqa: E402
from telluride_decoding_amd import preprocess as pp  # noqa: E402
from tests import host_audio as ha  # noqa: E402

HBM_TBS = 6.3          # achievable stream rate (MI355X_MICROARCH: 6.29 TB/s measured copy)
FP64_MFMA_TFLOPS = 78.6


def timed(fn, reps):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / reps


def host_intensity(x, fs_in, fs_out):
  """The reference's loop (preprocess.py:652-663, 706), window 1, no buffer."""
  data = x.astype(np.float32) ** 2
  hw = 0.5 / fs_out
  rows = int(round(data.shape[0] / fs_in * fs_out))
  out = np.zeros((rows, data.shape[1]))
  for i in range(rows):
    t = float(i) / fs_out
    t1 = int(max(0, round(fs_in * (t - hw))))
    t2 = int(min(data.shape[0], round(fs_in * (t + hw))))
    out[i, :] = np.mean(data[t1:t2, :], axis=0)
  return (out ** 0.5) ** np.log10(2)


def intensity(seconds, reps, no_host):
  h = device.default_handle()
  n = int(seconds * 44100)
  rng = np.random.default_rng(1)
  x = rng.standard_normal((n, 2), dtype=np.float32)
  t = torch.from_numpy(x).to(h.device)
  ms = timed(lambda: pp.AudioFeatures('a', 44100, 100, exponent=np.log10(2)).compute_intensity(t), reps)
  rows = int(round(n / 44100 * 100))
  kern = timed(lambda: device.audio_intensity(t, None, rows, 44100, 100, 0.005, True, True, np.log10(2)), reps)
  bytes_min = n * 2 * 4 + rows * 2 * 8
  res = {'case': 'intensity_%gs_44k1_stereo' % seconds, 'frames': n, 'out_rows': rows, 'input_mb': round(n * 8 / 1e6, 1),
         'ms_per_call': round(ms, 4), 'kernel_ms': round(kern, 4),
         'hbm_floor_ms_est': round(bytes_min / (HBM_TBS * 1e12) * 1e3, 4),
         'kernel_fraction_of_hbm_floor': round(bytes_min / (HBM_TBS * 1e9) / kern, 3)}
  if not no_host:
    t0 = time.perf_counter()
    host_intensity(x, 44100, 100)
    res['host_reference_loop_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
  return res


def spectrogram(seconds, reps, no_host):
  h = device.default_handle()
  n = int(seconds * 16000)
  wave = ha.spectrogram_input('time', n).astype(np.float32)
  t = torch.from_numpy(wave).to(h.device)
  p = pp.AudioFeatures('s', 16000, 100)
  ms = timed(lambda: p.compute_spectrogram(t), reps)
  seg, hop, nfft, frames = ha.spectrogram_shape(n)
  k = nfft // 2 + 1
  kp = -(-k // 16) * 16
  flop = 2.0 * frames * (-(-seg // 64) * 64) * 2 * kp
  bytes_min = n * 4 + k * frames * 8
  res = {'case': 'spectrogram_%gs_16k' % seconds, 'samples': n, 'bins': k, 'frames': frames,
         'ms_per_call': round(ms, 4), 'fp64_mfma_floor_ms_est': round(flop / (FP64_MFMA_TFLOPS * 1e12) * 1e3, 4),
         'hbm_floor_ms_est': round(bytes_min / (HBM_TBS * 1e12) * 1e3, 4),
         'design_bytes_floor_ms_est': round(5 * k * frames * 8 / (HBM_TBS * 1e12) * 1e3, 4)}
  if not no_host:
    try:
      import scipy.signal as ss
    except ImportError:
      ss = None
    if ss is not None:
      t0 = time.perf_counter()
      w = wave.astype(np.float32)
      pe = ss.lfilter([1, -0.95], [1], w)
      _, _, spec = ss.stft(pe, fs=1.0, window='hamming', nperseg=128, noverlap=112, nfft=512,
                           return_onesided=True)
      spec = np.real(spec * np.conj(spec))
      spec = ss.lfilter((.2, 1, .2), [1], spec, axis=0)
      spec = ss.lfilter((.2, 1, .2), [1], spec, axis=1)
      off = 0.0001 * np.max(spec)
      spec = (off + spec) ** 0.25 - off ** 0.25
      spec = 255 / np.max(spec) * spec
      res['host_reference_scipy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--no-host', action='store_true')
  args = ap.parse_args()
  print(json.dumps(intensity(60, args.reps, args.no_host)))
  print(json.dumps(intensity(20 * 60, args.reps, args.no_host)))
  print(json.dumps(spectrogram(60, args.reps, args.no_host)))


if __name__ == '__main__':
  main()
