"""Times the way in from a raw recording: a BrainVision or EDF file -> the feature 'eeg' resident on the GPU, host
route against device route.

Workload (the defaults, DESIGN section 23's): 64 channels x 1.8e6 frames, an hour at 500 Hz, as a BrainVision
float32 multiplexed file and as an EDF file with 500 samples per record, generated from a seed into a temporary
directory.  --formats also takes `bdf`: a BioSemi BDF file of --channels signals plus a 'Status'
signal, --bdf_samples (2048) 24-bit samples per record.
   python tools/time_raw_ingest.py [--channels 64] [--frames 1800000] [--repeats 5] [--formats brainvision,edf]

Prints one JSON object, per format:
  host_wall_s / device_wall_s   BrainExperiment.load_all_data + assemble_brain_data of every channel, the result on
                                the device (the host route's NumPy 'eeg' is uploaded): the host clock around a device
                                synchronise, host and device route alternated, the median of --repeats after a
                                warm-up of each, with the fastest and slowest run
  device_split_s                the device route taken apart with the same clock, every part waited for before the
                                next starts: the file into pinned memory, the upload, the decode launch, the
                                assemble launch
  decode / assemble / loop      device events around the decode launch, the one-launch assemble and the retained
                                strided-copy loop on the same rows: ms (median, fastest, slowest), the bytes read
                                plus written, GB/s, and the time over that of `copy`, a device-to-device copy that
                                moves the same number of bytes, timed the same way in this run
  status_events (bdf)           BrainTrial.find_status_trigger_times on the device signal (the launches, the 8-byte
                                count and the events copied back) and the host form that copies the channel back
                                first: the host clock, seconds (median, fastest, slowest), and the number of events
Exits with an error when there is no GPU.
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--channels', type=int, default=64)
  ap.add_argument('--frames', type=int, default=1800000)
  ap.add_argument('--edf_samples', type=int, default=500)
  ap.add_argument('--bdf_samples', type=int, default=2048)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--formats', default='brainvision,edf')
  args = ap.parse_args()

  import numpy as np
  import torch
  from telluride_decoding_amd import device, ingest, ingest_bdf, ingest_brainvision, ingest_edf
  from tests import host_bdf as hb
  from tests import host_raw as hr
  if not device.gpu_available():
    raise SystemExit('time_raw_ingest needs a GPU: there is nothing to time without one')
  h = device.default_handle()
  really_available = device.gpu_available
  out_dir = tempfile.mkdtemp(prefix='time_raw_ingest_')
  result = {'channels': args.channels, 'frames': args.frames}
  rng = np.random.default_rng(1)
  names = hr.channel_names(args.channels)

  def spread(times, digits=4):
    return {'median': round(statistics.median(times), digits), 'min': round(min(times), digits),
            'max': round(max(times), digits)}

  def timed(fn):
    fn()
    h.synchronize()
    times = []
    for _ in range(args.repeats):
      h.timer_start()
      fn()
      times.append(h.timer_stop())
    return times

  def against_copy(times, nbytes, copy_ms):
    out = spread(times)
    out.update(bytes=nbytes, GB_per_s=round(nbytes / out['median'] / 1e6, 1), of_copy=round(out['median'] / copy_ms, 2))
    return out

  def copy_ms(nbytes):
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=h.device)
    dst = torch.empty_like(src)
    return spread(timed(lambda: dst.copy_(src)))

  def status_events(make):
    """find_status_trigger_times on the device signal (the launches, the 8-byte count and the events copied back)
    against the host form, which copies the whole channel back first: the host clock, the median of --repeats."""
    trial = ingest.BrainTrial('trial')
    trial.load_brain_data(out_dir, make())
    signal = trial.brain_data[hb.STATUS].signal
    assert ingest._is_device_tensor(signal)

    def clocked(fn):
      fn()
      times = []
      for _ in range(args.repeats):
        h.synchronize()
        t0 = time.perf_counter()
        found = fn()
        times.append(time.perf_counter() - t0)
      return found, spread(times, 6)

    def on_host():
      code = ingest._host_array(signal)[:, 0].astype(np.int64) & 0xffff
      at = np.flatnonzero((code != np.concatenate(([0], code[:-1]))) & (code != 0))
      return at / trial.brain_data[hb.STATUS].sr, code[at]

    (times, codes), device_s = clocked(trial.find_status_trigger_times)
    (host_times, host_codes), host_s = clocked(on_host)
    assert np.array_equal(times, host_times) and np.array_equal(codes, host_codes)
    return {'samples': int(signal.shape[0]), 'events': int(len(times)), 'device_s': device_s,
            'host_copy_back_s': host_s}

  try:
    for fmt in args.formats.split(','):
      if fmt == 'brainvision':
        samples = rng.standard_normal((args.frames, args.channels), dtype=np.float32).view(np.uint32)
        hr.write_brainvision(out_dir, 'rec', samples, hr.resolutions(args.channels), names=names)
        data_path, make = os.path.join(out_dir, 'rec.eeg'), lambda: ingest_brainvision.BvBrainDataFile('rec')
        del samples
      elif fmt == 'bdf':
        n = args.bdf_samples
        records = args.frames // n
        signals = [{'label': names[c], 'digital': rng.integers(-(1 << 23), 1 << 23, size=(records, n), dtype=np.int32),
                    'physical_min': -262144, 'physical_max': 262143, 'digital_min': -8388608, 'digital_max': 8388607}
                   for c in range(args.channels)]
        signals.append(dict(signals[0], label=hb.STATUS, digital=hb.status_codes(rng, records * n, every=n // 2 + 1)
                            .reshape(records, n)))
        hb.write_bdf(os.path.join(out_dir, 'rec.bdf'), signals)
        data_path, make = os.path.join(out_dir, 'rec.bdf'), lambda: ingest_bdf.BdfBrainDataFile('rec')
        del signals
      else:
        n = args.edf_samples
        records = args.frames // n
        hr.write_edf(os.path.join(out_dir, 'rec.edf'),
                     [{'label': names[c], 'digital': rng.integers(-32768, 32768, size=(records, n)).astype(np.int16),
                       'physical_min': -3276.8, 'physical_max': 3276.7, 'digital_min': -32768, 'digital_max': 32767}
                      for c in range(args.channels)])
        data_path, make = os.path.join(out_dir, 'rec.edf'), lambda: ingest_edf.EdfBrainDataFile('rec')
      out = {'file_bytes': os.path.getsize(data_path)}

      def wall(on_device):
        device.gpu_available = really_available if on_device else (lambda: False)
        try:
          h.synchronize()
          t0 = time.perf_counter()
          sound = {'audio_data': np.zeros((16, 1), np.float32), 'audio_sr': 16000}
          experiment = ingest.BrainExperiment({'trial': [sound, make()]}, out_dir, out_dir)
          experiment.load_all_data()
          trial = experiment.trial_data('trial')
          trial.assemble_brain_data(list(names))
          eeg = trial.model_features['eeg']
          if not ingest._is_device_tensor(eeg):
            eeg = torch.from_numpy(eeg).to(h.device)
          h.synchronize()
          t1 = time.perf_counter()
        finally:
          device.gpu_available = really_available
        per = {'brainvision': 1, 'edf': args.edf_samples, 'bdf': args.bdf_samples}[fmt]
        assert tuple(eeg.shape) == (args.frames // per * per, args.channels)
        return t1 - t0

      wall(False), wall(True)
      host_times, device_times = [], []
      for _ in range(args.repeats):
        host_times.append(wall(False))
        device_times.append(wall(True))
      out['host_wall_s'], out['device_wall_s'] = spread(host_times), spread(device_times)

      # ---- the device route taken apart (one run, every part waited for)
      size = out['file_bytes']
      pinned = torch.empty(size, dtype=torch.uint8, pin_memory=True)
      image = h.empty((size,), 'uint8')
      if fmt == 'brainvision':
        layout = dict(data_offset=0, records=args.frames, record_bytes=4 * args.channels, samples_per_record=1,
                      sample_kind=device.RAW_FLOAT32, signal_offsets=[4 * c for c in range(args.channels)],
                      scales=hr.resolutions(args.channels))
        rows, elem = args.frames, 4
      elif fmt == 'bdf':
        n = args.bdf_samples
        layout = dict(data_offset=256 * (args.channels + 2), records=args.frames // n,
                      record_bytes=3 * n * (args.channels + 1), samples_per_record=n,
                      signal_offsets=[3 * n * c for c in range(args.channels)], scales=[0.1] * args.channels,
                      offsets=[0.5] * args.channels)
        rows, elem = args.frames // n * n, 8
      else:
        n = args.edf_samples
        layout = dict(data_offset=256 * (args.channels + 1), records=args.frames // n,
                      record_bytes=2 * n * args.channels, samples_per_record=n, sample_kind=device.RAW_INT16,
                      signal_offsets=[2 * n * c for c in range(args.channels)], scales=[0.1] * args.channels,
                      offsets=[0.5] * args.channels)
        rows, elem = args.frames // n * n, 8
      matrix = h.empty((args.channels, rows), 'float64' if elem == 8 else 'float32')
      eeg = h.empty((rows, args.channels), 'float32')
      h.synchronize()
      t0 = time.perf_counter()
      with open(data_path, 'rb') as f:
        f.readinto(memoryview(pinned.numpy()))
      t1 = time.perf_counter()
      image.copy_(pinned, non_blocking=True)
      h.synchronize()
      t2 = time.perf_counter()
      decoder = device.raw24_decode if fmt == 'bdf' else device.raw_decode
      decode = lambda: decoder(image, out=matrix, handle=h, **layout)
      decode()
      h.synchronize()
      t3 = time.perf_counter()
      sources = [matrix[c].reshape(-1, 1) for c in range(args.channels)]
      assemble = lambda: device.columns_assemble(sources, rows, out=eeg, handle=h)
      assemble()
      h.synchronize()
      t4 = time.perf_counter()
      out['device_split_s'] = {'file_read': round(t1 - t0, 4), 'upload': round(t2 - t1, 4),
                               'decode': round(t3 - t2, 4), 'assemble': round(t4 - t3, 4)}
      out['route'] = {'decode_transposed': fmt != 'bdf' and device.raw_route(
          layout['samples_per_record'], 4 if elem == 4 else 2, layout['record_bytes'])[0],
                      'assemble_transposed': device.columns_route(args.channels, 1)}

      # ---- each launch against a copy of the same bytes
      # (what the launch reads of the image -- the listed signals' bytes -- plus what it writes)
      sample_bytes = {'brainvision': 4, 'edf': 2, 'bdf': 3}[fmt]
      decode_bytes = args.channels * rows * (sample_bytes + elem)
      assemble_bytes = args.channels * rows * (elem + 4)
      copy_decode, copy_assemble = copy_ms(decode_bytes), copy_ms(assemble_bytes)
      out['decode'] = against_copy(timed(decode), decode_bytes, copy_decode['median'])
      out['assemble'] = against_copy(timed(assemble), assemble_bytes, copy_assemble['median'])
      out['loop'] = against_copy(timed(lambda: ingest._assemble_columns_loop(sources, rows, args.channels)),
                                 assemble_bytes, copy_assemble['median'])
      out['copy'] = {'decode_bytes_ms': copy_decode, 'assemble_bytes_ms': copy_assemble}
      if fmt == 'bdf':
        out['status_events'] = status_events(make)
      result[fmt] = out
      del pinned, image, matrix, eeg, sources
  finally:
    shutil.rmtree(out_dir, ignore_errors=True)
  print(json.dumps(result))


if __name__ == '__main__':
  main()
