"""The decode harness: load a saved model, score two speakers window by window, decide, count.

The reference's infer.py, entry point for entry point: `create_brain_data` (:109-170),
`calculate_time_axis` (:173-199), `get_data_for_model` (:202-244), `regress_and_correlate`
(:247-266), `load_model` (:269-298), `find_first_segment` (:301-324), `run_reduction_test`
(:327-464), `run_comparison_test` (:467-525) and `main` (:528-548) with the reference's flags
(`make_parser`; `python -m telluride_decoding_amd.infer`).

A model directory is what decoding.run_decoding_experiment writes with `saved_model_dir` set --
decoder_model.json with the fitted model inside it -- or a directory holding `model.save`'s
brain_model.json next to a decoder_model.json.  It is this package's own format:
a TensorFlow SavedModel is neither written nor read.  Plots are not drawn (`plot_dir` is accepted and
one line is logged).

`run_reduction_test` and `run_comparison_test` take two forms, chosen by whether the first argument
is a string: the reference's (model directory, TFRecord directory, file patterns, ...) and the
in-memory form (a Decoder -- or, for the comparison, a factory of Decoders -- and the two speakers'
test datasets, the rest by keyword).

Everything per frame and per window runs in HIP kernels.  The model's forward pass and the per-frame
scores come from `Decoder.test_all_device` (one launch set per dataset, the scores stay on the
device).  The sweep over the window sizes is ONE call, `td_attention_sweep`: the window means of both
speakers' scores and of the labels for every size, the end of the first same-label stretch, the
decisions of the winner-take-all / stepped decoders and the counts of correct windows, in two
launches and one copy back.  The state-space decoder takes the means from that call and runs the
existing `td_decode_ssd` per size.  `regress_and_correlate`, `_window_means_host` and
`decode_attention` remain as the per-size route (one `td_window_means` launch per signal and size, one
decision launch per size): the reference's own call structure, and what the sweep is tested against
bit for bit.
"""
import argparse
import collections
import logging
import os

import numpy as np

from telluride_decoding_amd import attention_decoder
from telluride_decoding_amd import brain_data
from telluride_decoding_amd import device
from telluride_decoding_amd import infer_decoder

WINDOW_LIST = (10, 100, 200, 400, 700, 1000)       # infer.py:376
ALLOWABLE_DECODER_TYPES = ('wta', 'stepped', 'ssd')  # infer.py:99


def _window_means_host(values, window_size, window_step):
  """Means of the full windows [k * step, k * step + size) of a [frames, cols] host array over all
  its entries (np.mean of a window, infer.py:264-265), float64, on the device: [n_windows]."""
  h = device.default_handle()
  values = np.asarray(values, np.float64)
  if values.ndim == 1:
    values = values.reshape(-1, 1)
  rows, cols = values.shape
  if rows < window_size:
    return np.zeros((0,), np.float64)
  acc = None
  for c in range(cols):
    col = h.to_device(np.ascontiguousarray(values[:, c:c + 1]), np.float64).reshape(-1)
    m = device.window_means(col, [0, rows], window_size, window_step, handle=h)
    acc = m if acc is None else acc + m
  return (acc / cols if cols > 1 else acc).cpu().numpy()


def regress_and_correlate(model_object, test_data, window_size):
  """Runs the decoder over `test_data` and averages scores and attention labels per window of
  `window_size` frames every window_size // 2 (infer.py:247-266; windows run across minibatch
  boundaries, only full windows count: result_store.py:253-271).

  Returns two lists of floats: the window scores and the window-averaged labels.
  """
  window_size = int(window_size)
  if window_size < 1:
    raise ValueError('Window size (%s) must be at least one frame.' % window_size)
  step = window_size // 2
  if step < 1:
    # TwoResultStore with a step of 0 never advances (result_store.py:262-271 yields the first
    # window for ever); the reference's harness never asks for it
    raise ValueError('Window size %d gives a window step of 0.' % window_size)
  return _window_results(model_object.test_all(test_data), window_size)


def _window_results(decoded, window_size):
  """(window scores, window label means) of one decoded dataset = test_all's (scores, labels)."""
  scores, labels = decoded
  step = window_size // 2
  if scores is None:
    return [], []
  if labels is None:
    raise ValueError('The dataset has no attended_speaker labels.')
  full_results = _window_means_host(scores, window_size, step)
  label_means = _window_means_host(labels, window_size, step)
  return [float(v) for v in full_results], [float(v) for v in label_means]


def calculate_time_axis(data, window_step, window_width, frame_rate):
  """Time (in minutes) of the CENTRE of every analysis window of a windowed signal (reference
  infer.py:173-199): `data` is the number of windows, or a list / array with one entry (row) per
  window."""
  import numbers
  if isinstance(data, numbers.Number):
    num_points = int(data)
  elif isinstance(data, list):
    num_points = len(data)
  elif isinstance(data, np.ndarray):
    num_points = data.shape[0]
  else:
    raise TypeError('Unknown type passed as input argument.')
  return (np.arange(num_points) * window_step + window_width / 2.0) / frame_rate / 60.0


def find_first_segment(labels):
  """Index of the first window whose label differs from the first one's -- the end of the stretch
  the state-space decoder's priors are tuned on -- or 0 when the label never changes
  (infer.py:301-324)."""
  if isinstance(labels, list):
    labels = np.asarray(labels)
  if not isinstance(labels, np.ndarray):
    raise TypeError('Labels input must be an ndarray, not %s' % type(labels))
  if labels.ndim != 1:
    raise TypeError('Labels input must be one-dimensional, not %s' % str(labels.shape))
  end_section = np.nonzero(np.logical_xor(labels, labels[0]))
  if end_section[0].shape[0]:
    return end_section[0][0]
  return 0


def decode_attention(decoder, d1_results, d2_results):
  """[n_windows, 3] array of (decision, lower, upper): `decoder.attention(c1, c2)` for every window
  in turn (infer.py:393-394), as ONE batched device call -- the decoders' state machines are
  sequential in time, so one GPU lane walks the windows (windows.hip)."""
  a, lo, hi = decoder.attention_batch(np.asarray(d1_results, np.float64),
                                      np.asarray(d2_results, np.float64))
  return np.stack([np.asarray(a, np.float64), np.asarray(lo, np.float64),
                   np.asarray(hi, np.float64)], axis=1)


def fraction_correct(attention, labels):
  """infer.py:395-402: `attention` true = attending to speaker 1 = label 0, so a window counts as
  correct when (attention >= 0.5) xor label."""
  labels = np.reshape(np.asarray(labels), (-1, 1))
  correct = np.logical_xor(attention[:, 0:1] >= 0.5, labels)
  return np.sum(correct) / float(len(correct))




# ---------------------------------------------------------------- data and models from files
def create_brain_data(tf_dir, train_files, test_files, params, audio_label):
  """The BrainData of one speaker for a saved model (reference infer.py:109-170): the TFRecord files
  of `tf_dir`, `train_files` / `test_files` (a name or pattern, or a list of them, joined with |)
  picking the two phases; input params['input_field'] with the contexts in `params`, `audio_label`
  as output and as input 2, the attention labels from params['attended_field'] ('attend' when the
  key is absent); minibatches of 200 frames at 100 Hz, never shuffled."""
  if isinstance(train_files, str):
    train_files = [train_files]
  train_file_re = '|'.join(['%s' % s for s in train_files])
  if isinstance(test_files, str):
    test_files = [test_files]
  test_file_re = '|'.join(['%s' % s for s in test_files])
  print('Training data from %s -> %s with label %s.' % (tf_dir, train_file_re, audio_label))
  print('Testing data from %s -> %s with label %s.' % (tf_dir, test_file_re, audio_label))
  attended = params['attended_field'] if 'attended_field' in params else 'attend'
  return brain_data.TFExampleData(
      params['input_field'], audio_label, 100,
      pre_context=params['pre_context'], post_context=params['post_context'],
      in2_fields=audio_label, in2_pre_context=params['input2_pre_context'],
      in2_post_context=params['input2_post_context'], attended_field=attended,
      final_batch_size=200, repeat_count=1, shuffle_buffer_size=0, data_dir=tf_dir,
      data_pattern='', train_file_pattern=train_file_re, validate_file_pattern='',
      test_file_pattern=test_file_re)


def get_data_for_model(tf_dir, train_files, test_files, model_object, audio_label_1, audio_label_2):
  """(bd1_train, bd1_test, bd2_train, bd2_test): the train and test datasets with speaker 1 and
  speaker 2 as the candidate audio, built from the loaded model's own parameters and checked
  against its input and output widths (reference infer.py:202-244)."""
  brain_data_1 = create_brain_data(tf_dir, train_files, test_files,
                                   model_object.decoding_model_params, audio_label_1)
  brain_data_2 = create_brain_data(tf_dir, train_files, test_files,
                                   model_object.decoding_model_params, audio_label_2)
  bd1_train = brain_data_1.create_dataset(mode='train')
  bd1_test = brain_data_1.create_dataset(mode='test')
  bd2_train = brain_data_2.create_dataset(mode='train')
  bd2_test = brain_data_2.create_dataset(mode='test')
  for dataset in (bd1_train, bd1_test, bd2_train, bd2_test):
    model_object.check_model_and_data(dataset)
  print('Finished the model checking.')
  return bd1_train, bd1_test, bd2_train, bd2_test


def load_model(model_dir, reducer):
  """The Decoder of a saved model directory (reference infer.py:269-298): the decoder class from
  the directory's name, the decoding model from the directory (Decoder.load_decoding_model), the
  correlation and LDA parameters from its decoder_model.json."""
  model_object = infer_decoder.create_decoder(model_dir.lower(), reduction=reducer)
  model_object.load_decoding_model(model_dir, {})
  decoder_param_filename = os.path.join(model_dir, infer_decoder.DECODER_PARAM_FILE_NAME)
  if os.path.exists(decoder_param_filename):
    model_object.restore_parameters(decoder_param_filename)
  else:
    raise IOError('Can not load decoder model parameters from %s' % decoder_param_filename)
  return model_object


# ---------------------------------------------------------------- the window-size sweep
def _checked_window_list(window_list):
  return list(WINDOW_LIST if window_list is None else window_list)


def _sweep_per_size(decoded1, decoded2, decoder_type, frame_rate, window_list, ssd_offset, details):
  """The sweep one size at a time, from the two decoded datasets (test_all's host results): three
  window-mean launches and one decision launch per size, each between an upload and a copy back --
  the call structure of the reference's loop (infer.py:376-407)."""
  window_results = []
  for window_size in window_list:
    window_step = window_size // 2
    if window_step < 1:
      raise ValueError('Window size %d gives a window step of 0.' % window_size)
    d1_results, _ = _window_results(decoded1, window_size)
    d2_results, labels = _window_results(decoded2, window_size)
    decoder = attention_decoder.create_attention_decoder(
        decoder_type, window_step=window_step, frame_rate=frame_rate, ssd_offset=ssd_offset)
    end_first_section = find_first_segment(labels)
    if end_first_section:
      decoder.tune(d1_results[:end_first_section], d2_results[:end_first_section])
    attention = decode_attention(decoder, d1_results, d2_results)
    frac_correct = fraction_correct(attention, labels)
    window_results.append(frac_correct)
    if details is not None:
      details[window_size] = dict(d1=np.asarray(d1_results), d2=np.asarray(d2_results),
                                  labels=np.asarray(labels), attention=attention,
                                  end_first_section=int(end_first_section))
  return dict(zip(window_list, window_results))


_SWEEP_CODES = {'wta': 'wta', 'stepped': 'stepped', 'step': 'stepped', 'ssd': 'none'}


def _host_decoded(decoded):
  scores, labels = decoded
  return (None if scores is None else scores.cpu().numpy()), labels


def _sweep_fused(decoded1, decoded2, decoder_type, frame_rate, window_list, ssd_offset, details):
  """The same sweep from test_all_device's results in one td_attention_sweep call per 16 sizes: the
  labels go up once, means, decisions and counts come back in one copy.  Same results, bit for bit,
  as _sweep_per_size."""
  (s1, labels1), (s2, labels2) = decoded1, decoded2
  plain = (s1 is not None and s2 is not None and labels1 is not None and labels2 is not None and
           int(s1.shape[0]) == int(s2.shape[0]) and np.size(labels2) == int(s2.shape[0]) and
           decoder_type in _SWEEP_CODES)
  if not plain:
    # An empty dataset, no labels, datasets of different lengths, labels of several columns, an
    # unknown decoder: whatever the per-size route makes of them (mostly: what it raises).
    return _sweep_per_size(_host_decoded(decoded1), _host_decoded(decoded2), decoder_type, frame_rate,
                           window_list, ssd_offset, details)
  h = device.default_handle()
  labels_dev = h.to_device(np.ascontiguousarray(labels2, np.float64).reshape(-1, 1),
                           np.float64).reshape(-1)
  # (a size whose step would be 0 raises when the loop below reaches it, as it always did)
  usable = []
  for window_size in window_list:
    if window_size // 2 < 1:
      break
    usable.append((window_size, window_size // 2))
  hosts = []
  for at in range(0, len(usable), device.SWEEP_MAX_SIZES):
    sweep = device.attention_sweep(s1, s2, labels_dev, usable[at:at + device.SWEEP_MAX_SIZES],
                                   _SWEEP_CODES[decoder_type], handle=h)
    hosts.append(device.attention_sweep_host(sweep))
  window_results = []
  for index, window_size in enumerate(window_list):
    window_step = window_size // 2
    if window_step < 1:
      raise ValueError('Window size %d gives a window step of 0.' % window_size)
    host, k = hosts[index // device.SWEEP_MAX_SIZES], index % device.SWEEP_MAX_SIZES
    first, last = int(host.window_offsets[k]), int(host.window_offsets[k + 1])
    d1_results = host.means[0, first:last].copy()
    d2_results = host.means[1, first:last].copy()
    labels = host.means[2, first:last].copy()
    if last == first:
      find_first_segment(labels)            # (no full window: raises what it always raised)
    end_first_section = int(host.summary[k, 0])
    if decoder_type == 'ssd':
      decoder = attention_decoder.create_attention_decoder(
          decoder_type, window_step=window_step, frame_rate=frame_rate, ssd_offset=ssd_offset)
      if end_first_section:
        decoder.tune([float(v) for v in d1_results[:end_first_section]],
                     [float(v) for v in d2_results[:end_first_section]])
      attention = decode_attention(decoder, d1_results, d2_results)
      frac_correct = fraction_correct(attention, labels)
    else:
      zeros = np.zeros(last - first)
      attention = np.stack([host.decisions[first:last].astype(np.float64), zeros, zeros], axis=1)
      frac_correct = host.summary[k, 1] / float(last - first)
    window_results.append(frac_correct)
    if details is not None:
      details[window_size] = dict(d1=d1_results, d2=d2_results, labels=labels, attention=attention,
                                  end_first_section=end_first_section)
  return dict(zip(window_list, window_results))


def run_reduction_test(model_dir, tf_dir, train_files, test_files=None, reduction=None,
                       decoder_type=None, audio_label_1=None, audio_label_2=None, plot_dir=None, *,
                       bd1_train=None, bd2_train=None, frame_rate=100.0, window_list=None,
                       ssd_offset=0.0, details=None, save_results_csv=None):
  """The window-size sweep of reference infer.run_reduction_test (:327-464), in two forms.

  The reference's form -- `model_dir` is a string: load_model(model_dir, reduction), the four
  datasets of get_data_for_model(tf_dir, train_files, test_files, ..., audio_label_1,
  audio_label_2), the decoder's inference parameters trained on the training datasets only if the
  saved model brought none (`decoding_model_params` empty), then the sweep.

  The in-memory form -- run_reduction_test(decoder, bd1_test, bd2_test, decoder_type='wta',
  bd1_train=None, bd2_train=None): an infer_decoder.Decoder (its reduction already chosen) and the
  test dataset with speaker 1 / speaker 2 as the candidate audio; the attention labels come with
  bd2_test (:384-386).  A decoder without trained inference parameters is trained first when the
  training datasets are given.

  Both forms, by keyword: frame_rate, window_list (default 10 ... 1000, the step is half the size),
  ssd_offset, details (a dict that receives per window size the scores, labels and decisions) and
  save_results_csv (a path for the reference's `Window size,Accuracy` file, :445-450).  plot_dir is
  accepted; plots are not drawn.

  Returns {window_size: fraction of windows decoded correctly}.
  """
  if isinstance(model_dir, str):
    for name, value in (('test_files', test_files), ('reduction', reduction),
                        ('decoder_type', decoder_type), ('audio_label_1', audio_label_1),
                        ('audio_label_2', audio_label_2)):
      if value is None:
        raise TypeError('run_reduction_test from a model directory needs %s.' % name)
    print('Running regression test with %s.' % reduction)
    model_object = load_model(model_dir, reduction)
    bd1_train, bd1_test, bd2_train, bd2_test = get_data_for_model(
        tf_dir, train_files, test_files, model_object, audio_label_1, audio_label_2)
    if model_object.decoding_model_params:
      print('Found saved model, no need to train the decoding model.')
      print(' Decoding_params are: %s' % (model_object.decoding_model_params,))
    else:
      model_object.train(bd1_train, bd2_train)
      print('Finished the inference model training.')
  else:
    model_object, bd1_test, bd2_test = model_dir, tf_dir, train_files
    if decoder_type is None:      # (the in-memory form's fourth positional argument, formerly)
      decoder_type = 'wta' if test_files is None else test_files
    if (not model_object.decoding_model_params and bd1_train is not None and
        bd2_train is not None):
      model_object.train(bd1_train, bd2_train)
  if plot_dir:
    logging.info('Plots are not drawn: nothing is written to %s.', plot_dir)
  window_list = _checked_window_list(window_list)
  # The reference decodes both datasets again for every window size (regress_and_correlate inside
  # the loop, infer.py:380-386); the per-frame scores do not depend on the window, so each dataset is
  # decoded ONCE here, and its scores stay on the device for the sweep.
  decoded1 = model_object.test_all_device(bd1_test)
  decoded2 = model_object.test_all_device(bd2_test)
  results = _sweep_fused(decoded1, decoded2, decoder_type, frame_rate, window_list, ssd_offset,
                         details)
  if isinstance(model_dir, str):
    test_name = test_files if isinstance(test_files, str) else (list(test_files) or [''])[0]
    print('Infer classification result for %s with %s and %s: %s' %
          (os.path.join(tf_dir, test_name), reduction, decoder_type,
           [results[w] for w in window_list]))
  if save_results_csv is not None:
    print('Saving results to {}'.format(save_results_csv))
    with open(save_results_csv, 'w') as f:
      f.write('Window size,Accuracy\n')
      for window_size in window_list:
        f.write('{},{}\n'.format(window_size, results[window_size]))
  return results


def run_comparison_test(model_dir, tf_dir, train_files, test_files=None, audio_label=None,
                        audio_label_2=None, plot_dir=None, reduction_list=None, decoder_list=None, *,
                        bd1_train=None, bd2_train=None, **kwargs):
  """run_reduction_test for every (reduction, decoder type) pair (reference infer.py:467-525): an
  OrderedDict keyed by (reduction, decoder) of {window size: fraction correct}.

  The reference's form -- `model_dir` is a string: every pair loads the saved model anew.  The
  in-memory form -- run_comparison_test(make_decoder, bd1_test, bd2_test, reduction_list,
  decoder_list=None, bd1_train=None, bd2_train=None): `make_decoder(reduction)` returns the
  infer_decoder.Decoder for one reduction.  Further keywords go to run_reduction_test.  The
  comparison plot is not drawn."""
  from_files = isinstance(model_dir, str)
  if not from_files and reduction_list is None:
    reduction_list = test_files       # (the in-memory form's fourth positional argument)
  if reduction_list is None:
    raise TypeError('run_comparison_test needs a reduction_list.')
  all_results = collections.OrderedDict()
  for reduction in reduction_list:
    for decoder in decoder_list or ALLOWABLE_DECODER_TYPES:
      if from_files:
        print('Running the regression test with %s and %s.' % (reduction, decoder))
        all_results[(reduction, decoder)] = run_reduction_test(
            model_dir, tf_dir, train_files, test_files, reduction, decoder, audio_label,
            audio_label_2, plot_dir, **kwargs)
      else:
        all_results[(reduction, decoder)] = run_reduction_test(
            model_dir(reduction), tf_dir, train_files, decoder_type=decoder, bd1_train=bd1_train,
            bd2_train=bd2_train, **kwargs)
  return all_results


# ---------------------------------------------------------------- command line
_REDUCTION_CHOICES = ['first', 'second', 'lda', 'mean', 'mean-squared', 'all']


def _parse_bool(text):
  if text.lower() in ('true', 't', '1', 'yes', 'y'):
    return True
  if text.lower() in ('false', 'f', '0', 'no', 'n'):
    return False
  raise argparse.ArgumentTypeError('not a boolean: %r' % text)


def make_parser():
  """The reference's flags under their names (infer.py:61-104).  --train_files and --test_files may
  be repeated; a boolean is given as --flag, --noflag or --flag=true|false.  The reference's
  defaults for the directories and the test file are paths of its authors' file system: here they
  are empty, and main asks for tf_dir and model_dir."""
  parser = argparse.ArgumentParser(prog='infer', description=__doc__.split('\n')[0])
  parser.add_argument('--tf_dir', default=None, help='Location of the TFRecord data for evaluation.')
  parser.add_argument('--model_dir', default=None, help='Location of the saved model.')
  parser.add_argument('--plot_dir', default=None, help='Accepted; plots are not drawn.')
  parser.add_argument('--save_results_csv', default=None, help='Path to results csv file')
  parser.add_argument('--train_files', action='append', default=[],
                      help='Training files for the decoder\'s inference parameters.')
  parser.add_argument('--test_files', action='append', default=[],
                      help='Testing files with which to verify performance.')
  parser.add_argument('--window_width', type=int, default=1000)
  parser.add_argument('--window_step', type=int, default=500)
  parser.add_argument('--window_overlap', type=float, default=0.5)
  parser.add_argument('--frame_rate', type=float, default=100)
  parser.add_argument('--reduction', default='lda', choices=_REDUCTION_CHOICES)
  parser.add_argument('--decoder', default='wta', choices=list(ALLOWABLE_DECODER_TYPES))
  for name in ('window_test', 'comparison_test'):
    parser.add_argument('--' + name, dest=name, nargs='?', const=True, default=False,
                        type=_parse_bool)
    parser.add_argument('--no' + name, dest=name, action='store_const', const=False)
  parser.add_argument('--audio_label', default='loudness',
                      help='TFRecord field of the audio signal; the second speaker is this label '
                      'with 2 appended.')
  return parser


def main(argv=None):
  """argv: the command line's arguments without the program name (None: sys.argv[1:]).  Returns what
  the test it ran returned."""
  parser = make_parser()
  flags = parser.parse_args(argv)
  if not flags.tf_dir or not os.path.exists(flags.tf_dir):
    parser.error('Can not find tf_dir: %s' % flags.tf_dir)
  if not flags.model_dir or not os.path.exists(flags.model_dir):
    parser.error('Can not find model_dir: %s' % flags.model_dir)
  print('FLAGS.reduction is', flags.reduction)
  common = dict(frame_rate=flags.frame_rate, save_results_csv=flags.save_results_csv)
  if flags.comparison_test:
    return run_comparison_test(flags.model_dir, flags.tf_dir, flags.train_files, flags.test_files,
                               flags.audio_label, flags.audio_label + '2', flags.plot_dir,
                               reduction_list=['first', 'lda'], **common)
  return run_reduction_test(flags.model_dir, flags.tf_dir, flags.train_files, flags.test_files,
                            flags.reduction, flags.decoder, flags.audio_label,
                            flags.audio_label + '2', flags.plot_dir, **common)


if __name__ == '__main__':
  main()
