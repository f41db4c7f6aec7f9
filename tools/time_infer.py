"""The window-size sweep of infer.run_reduction_test, timed two ways on the same per-frame scores in
one process: the per-size route (per size: window means of both speakers' scores and
of the labels, each behind an upload and in front of a copy back, then one decision launch) against the
one-call sweep (td_attention_sweep: two launches, one copy back).  One decoded recording of 60 000
frames, the six default window sizes, the winner-take-all and the stepped decoder.  Then the directory
form end to end: a saved model and TFRecord files in, accuracies out.

Warm-up first, then the median of repeated runs, each run timed on its own with the device idle before
and after.  Prints one JSON line.
    python tools/time_infer.py [--reps 30]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def _median_ms(fn, reps, warmup=5):
  import torch
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
  return statistics.median(times), min(times), max(times)


def main(argv=None):
  parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  parser.add_argument('--reps', type=int, default=30)
  parser.add_argument('--frames', type=int, default=60000)
  args = parser.parse_args(argv)
  from telluride_decoding_amd import brain_data, brain_model, decoding, device, infer, infer_decoder, synth, tfrecord
  device.default_handle()
  trial = 6000
  trials = synth.make_trials(9, args.frames // trial, trial, 64, switch_half=True)

  def speaker(k, mix=False):
    files = [(t[0], t[1][:, 1 - k:2 - k], t[1][:, k:k + 1], t[2]) for t in trials]
    return brain_data.Dataset(files, 1000, 0, 31, mixup_batch=mix, mixup_seed=3)

  bd1, bd2 = speaker(0), speaker(1)
  model = brain_model.BrainModelLinearRegression(bd1, regularization_lambda=0.1)
  model.fit(bd1)
  dec = infer_decoder.LinearRegressionDecoder(model, reduction='lda')
  dec.train(speaker(0, True), bd1)
  on_device = [dec.test_all_device(bd1), dec.test_all_device(bd2)]
  on_host = [(scores.cpu().numpy(), labels) for scores, labels in on_device]
  sizes = list(infer.WINDOW_LIST)
  out = {'frames': int(on_device[0][0].shape[0]), 'window_sizes': sizes, 'reps': args.reps}
  for decoder_type in ('wta', 'stepped'):
    per_size = lambda: infer._sweep_per_size(on_host[0], on_host[1], decoder_type, 100.0, sizes, 0.0, None)
    fused = lambda: infer._sweep_fused(on_device[0], on_device[1], decoder_type, 100.0, sizes, 0.0, None)
    assert per_size() == fused()
    for name, fn in (('per_size', per_size), ('sweep', fused)):
      median, low, high = _median_ms(fn, args.reps)
      out['%s_%s_ms' % (decoder_type, name)] = round(median, 4)
      out['%s_%s_range_ms' % (decoder_type, name)] = [round(low, 4), round(high, 4)]
    out['%s_accuracy' % decoder_type] = {str(k): float(v) for k, v in fused().items()}

  # the directory form, end to end: files -> saved model -> accuracies
  root = tempfile.mkdtemp(prefix='time_infer_')
  try:
    for i, (eeg, env, att) in enumerate(trials):
      tfrecord.write_file(os.path.join(root, 'trial_%02d.tfrecords' % i),
                          {'eeg': eeg, 'intensity': env[:, 0:1], 'intensity2': env[:, 1:2], 'attend': att})
    saved = os.path.join(root, 'linear_saved')
    flags = decoding.DecodingOptions().set_from_dict(dict(
        tfexample_dir=root, input_field='eeg', output_field='intensity', dnn_regressor='linear', post_context=31,
        train_file_pattern='trial_0[0-7]', test_file_pattern='trial_0[89]', validate_file_pattern='',
        batch_size=1000, summary_dir=os.path.join(root, 'summary'), saved_model_dir=saved))
    decoding.run_decoding_experiment(flags)
    directory = lambda: infer.run_reduction_test(saved, root, 'trial_0[0-7]', 'trial_', 'lda', 'wta', 'intensity',
                                                 'intensity2')
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')        # (the reference's progress prints)
    try:
      median, low, high = _median_ms(directory, max(args.reps // 6, 3), warmup=2)
    finally:
      sys.stdout.close()
      sys.stdout = stdout
    out['directory_form_wta_ms'] = round(median, 3)
    out['directory_form_wta_range_ms'] = [round(low, 3), round(high, 3)]
  finally:
    shutil.rmtree(root, ignore_errors=True)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
