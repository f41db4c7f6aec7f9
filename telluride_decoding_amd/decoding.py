"""Train and test a decoder from a set of options: the package's counterpart of the reference's
main program, decoding.py.

The same entry points with the same meaning -- `DecodingOptions` (:48-154), `create_brain_model`
(:259-311), `train_and_test` (:314-350), `write_experiment_summary` (:353-410), `check_files`
(:413-433), `train_lda_model` (:436-482), `run_decoding_experiment` (:485-577), `main` (:580-586) --
built from this package's own estimators: the data come from brain_data.create_brain_dataset, the
models are brain_model.BrainModelLinearRegression / BrainModelDNN / BrainModelClassifier and
cca.BrainModelCCA, the correlation + LDA stage is infer_decoder.Decoder.train, whose windowed route
(correlation_frames = 100 by default) runs on the device (device.window_class_moments).

Where this module departs from the reference:
  * the options are a plain class and the command line is argparse (no absl, no attr);
  * tensorboard_dir is accepted and ignored; saved_model_dir receives one file, decoder_model.json,
    which holds the decoder's parameters and, under 'decoding_model', the fitted model in this
    package's own format (brain_model.model_to_dict; a TensorFlow SavedModel is not written).
    infer.load_model reads the directory back;
  * 'classifier' gets the parsed hidden-unit list (the reference hands the constructor the raw string
    and fails there), and, having no decoder in infer_decoder.create_decoder, skips the LDA stage:
    d' is None;
  * for 'fullyconnected' the `loss` option ('mse' | 'pearson') reaches compile (the reference defines
    the flag and never reads it);
  * 'tf' and 'linear_with_bias', listed by the reference's flag and built by nothing there, raise the
    same TypeError as any unknown name.
"""
import argparse
import logging
import os

import numpy as np

from telluride_decoding_amd import brain_data
from telluride_decoding_amd import brain_model
from telluride_decoding_amd import cca
from telluride_decoding_amd import infer_decoder
from telluride_decoding_amd import tfrecord

# What stands in for the reference's brain_model.BrainModel base class in the type checks.
_BRAIN_MODELS = (brain_model.BrainModelLinearRegression, brain_model.BrainModelDNN,
                 brain_model.BrainModelClassifier, cca.BrainModelCCA)


class DecodingOptions(object):
  """All the parameters of one decoding experiment (names and defaults: the reference's)."""

  _DEFAULTS = (
      ('attended_field', 'attend'),
      ('batch_norm', False),
      ('batch_size', 512),
      ('cca_dimensions', 10),
      ('check_file_pattern', ''),
      ('correlation_frames', 100),
      ('correlation_reducer', 'lda'),
      ('data', 'tfrecords'),
      ('debug', False),
      ('dnn_regressor', 'fullyconnected'),
      ('dropout', 0.0),
      ('epoch_count', 100),
      ('frame_rate', 100.0),
      ('hidden_units', '20-20'),
      ('input2_field', ''),
      ('input2_post_context', 0),
      ('input2_pre_context', 0),
      ('input_offset', 0),
      ('input_field', 'mel_spectrogram'),
      ('learning_rate', 0.05),
      ('loss', 'mse'),
      ('min_context', 0),
      ('output_field', 'envelope'),
      ('post_context', 0),
      ('pre_context', 0),
      ('random_mixup_batch', False),
      ('regularization_lambda', 0.1),
      ('saved_model_dir', None),
      ('shuffle_buffer_size', 100000),
      ('summary_dir', '/tmp/tf'),
      ('tensorboard_dir', None),
      ('test_file_pattern', ''),
      ('test_metric', 'pearson_correlation_first'),
      ('tfexample_dir', None),
      ('tfexample_pattern', ''),
      ('train_file_pattern', ''),
      ('validate_file_pattern', ''),
  )

  def __init__(self):
    for name, default in self._DEFAULTS:
      setattr(self, name, default)

  @classmethod
  def field_names(cls):
    return [name for name, _ in cls._DEFAULTS]

  def as_dict(self):
    return {name: getattr(self, name) for name in self.field_names()}

  def set_flags(self, all_flags):
    """Takes every option from an object that has them as attributes (an argparse.Namespace)."""
    for name in self.field_names():
      setattr(self, name, getattr(all_flags, name))
    return self

  def experiment_parameters(self, delimiter=','):
    """'name=value' of every option, sorted by name and joined by `delimiter`; the list itself
    when the delimiter is None (or empty)."""
    values = self.as_dict()
    keys_and_values = ['%s=%s' % (k, values[k]) for k in sorted(values)]
    if delimiter:
      return delimiter.join(keys_and_values)
    return keys_and_values

  def set_from_dict(self, new_values):
    for k, v in new_values.items():
      setattr(self, k, v)
    return self

  def __repr__(self):
    return 'DecodingOptions(%s)' % self.experiment_parameters(', ')


def _hidden_units(model_flags):
  if not model_flags.hidden_units:
    return []
  return [int(x) for x in model_flags.hidden_units.split('-')]


def create_brain_model(model_flags, input_dataset):
  """The model the options name, sized from `input_dataset` and compiled."""
  if not isinstance(model_flags, DecodingOptions):
    raise TypeError('Model_flags must be a DecodingOptions, not a %s' % type(model_flags))
  if not isinstance(input_dataset, brain_data.Dataset):
    raise TypeError('input_dataset must be a tf.data.Dataset, not %s' % type(input_dataset))
  compile_args = {}
  if model_flags.dnn_regressor == 'fullyconnected':
    bm = brain_model.BrainModelDNN(input_dataset, _hidden_units(model_flags),
                                   tensorboard_dir=model_flags.tensorboard_dir)
    compile_args['loss'] = model_flags.loss
  elif model_flags.dnn_regressor == 'classifier':
    bm = brain_model.BrainModelClassifier(input_dataset, _hidden_units(model_flags),
                                          tensorboard_dir=model_flags.tensorboard_dir)
  elif model_flags.dnn_regressor == 'linear':
    bm = brain_model.BrainModelLinearRegression(input_dataset, model_flags.regularization_lambda,
                                                tensorboard_dir=model_flags.tensorboard_dir)
  elif model_flags.dnn_regressor == 'cca':
    bm = cca.BrainModelCCA(input_dataset, cca_dims=model_flags.cca_dimensions,
                           regularization_lambda=model_flags.regularization_lambda,
                           tensorboard_dir=model_flags.tensorboard_dir)
  else:
    raise TypeError('Unknown model type %s in create_brain_model.' % model_flags.dnn_regressor)
  bm.compile(learning_rate=model_flags.learning_rate, **compile_args)
  return bm


def train_and_test(my_flags, test_brain_data, test_brain_model, epochs=1):
  """Fits the model on the 'train' dataset and evaluates it on the 'test' dataset:
  (train_results -- {} for the closed-form models --, test_results)."""
  if not isinstance(test_brain_data, brain_data.BrainData):
    raise TypeError('test_brain_data must be a BrainData object, not a %s' % test_brain_data)
  if not isinstance(test_brain_model, _BRAIN_MODELS):
    raise TypeError('Model in train_and_test must be a BrainModel object, not %s' % test_brain_model)
  if not isinstance(my_flags, DecodingOptions):
    raise TypeError('Train_and_test needs a DecodingOptions object, not %s.' % type(my_flags))
  logging.info('train_and_test: %s', my_flags.experiment_parameters())
  train_dataset = test_brain_data.create_dataset('train')
  train_results = test_brain_model.fit(train_dataset, epochs=epochs)
  test_dataset = test_brain_data.create_dataset('test')
  test_results = test_brain_model.evaluate(test_dataset)
  return train_results, test_results


def write_experiment_summary(my_flags, train_results, test_results, dprime=None):
  """Writes results.txt into the options' summary_dir: the parameters, one line per test metric and
  d'.  The token PARAMS in summary_dir is replaced by the experiment's parameters, so that parallel
  runs under one flag value land in separate directories."""
  if not isinstance(my_flags, DecodingOptions):
    raise TypeError('Write_experiment_summary needs a DecodingOptions object,' +
                    ' not %s.' % type(my_flags))
  del train_results               # (the reference writes nothing of them either)
  summary_dir = my_flags.summary_dir
  if not summary_dir:
    return
  if 'PARAMS' in summary_dir:
    summary_dir = summary_dir.replace('PARAMS', my_flags.experiment_parameters(','))
  results_file = os.path.join(summary_dir, 'results.txt')
  os.makedirs(summary_dir, exist_ok=True)
  with open(results_file, 'w') as fp:
    fp.write('Parameters: %s\n' % my_flags.experiment_parameters(';'))
    for k in test_results:
      if isinstance(test_results[k], np.ndarray):
        fp.write('Final_Test/%s: %s\n' %
                 (k, ' '.join([str(f) for f in np.reshape(test_results[k], (-1))])))
      else:
        fp.write('Final_Testing/%s: %g\n' % (k, test_results[k]))
    if dprime is not None:
      fp.write('Final_Testing/dprime: %g\n' % dprime)
  logging.info('Wrote summary results to %s', results_file)


def check_files(exp_data_dir, tfexample_pattern='.tfrecords'):
  """Counts the records of every .tfrecords file under `exp_data_dir` whose name contains
  `tfexample_pattern` (logged per file) and prints how many files there are."""
  all_files = []
  for path, _, files in os.walk(exp_data_dir):
    all_files += [os.path.join(path, f) for f in sorted(files)
                  if f.endswith('.tfrecords') and tfexample_pattern in f]
  logging.info('Found %d files for TFExample data analysis.', len(all_files))
  print('Found %d files for TFExample data analysis.' % len(all_files))
  for f in all_files:
    logging.info('%s: %d', f, tfrecord.count_tfrecords(f)[0])


def train_lda_model(brain_dataset, trained_model, my_flags):
  """Trains the correlation + LDA stage on the 'test' files run through the trained model: the matched
  data against the same data mixed up within each minibatch.  Returns (d', the trained Decoder)."""
  if not isinstance(brain_dataset, brain_data.BrainData):
    raise TypeError('Train_lda_model needs BrainData, not %s.' % type(brain_dataset))
  if not callable(trained_model):
    raise TypeError('Trained_model parameter is not a callable function, but a %s.' %
                    type(trained_model))
  if isinstance(my_flags, dict):
    my_flags = DecodingOptions().set_from_dict(my_flags)
  elif not isinstance(my_flags, DecodingOptions):
    raise TypeError('Train_lda_model needs a DecodingOptions object, not %s.' % type(my_flags))
  attended_data = brain_dataset.create_dataset('test', mixup_batch=False)
  unattended_data = brain_dataset.create_dataset('test', mixup_batch=True)
  decoder = infer_decoder.create_decoder(my_flags.dnn_regressor,
                                         reduction=my_flags.correlation_reducer, model=trained_model)
  dprime = decoder.train(unattended_data, attended_data, window_size=my_flags.correlation_frames)
  return dprime, decoder


def run_decoding_experiment(my_flags):
  """One experiment: data, model, training, testing, the LDA stage and the summary.  Returns
  (train_results, test_results, d')."""
  if my_flags.debug:
    logging.getLogger().setLevel(logging.DEBUG)
  if my_flags.pre_context + 1 + my_flags.post_context < my_flags.min_context:
    my_flags.post_context = my_flags.min_context - (my_flags.pre_context + 1)
  if not my_flags.summary_dir.endswith('/'):
    my_flags.summary_dir = my_flags.summary_dir + '/'
  logging.info('Params string is: %s', my_flags.experiment_parameters())
  logging.info('TFRecord data from: %s with %s', my_flags.tfexample_dir, my_flags.tfexample_pattern)

  if my_flags.check_file_pattern:
    check_files(my_flags.tfexample_dir, my_flags.tfexample_pattern)
    return {}, {}, 0.0

  test_brain_data = brain_data.create_brain_dataset(
      my_flags.data, my_flags.input_field, my_flags.output_field,
      attended_field=my_flags.attended_field, frame_rate=my_flags.frame_rate,
      pre_context=my_flags.pre_context, post_context=my_flags.post_context,
      in2_fields=my_flags.input2_field, in2_pre_context=my_flags.input2_pre_context,
      in2_post_context=my_flags.input2_post_context, input_offset=my_flags.input_offset,
      final_batch_size=my_flags.batch_size, shuffle_buffer_size=my_flags.shuffle_buffer_size,
      data_dir=my_flags.tfexample_dir, data_pattern=my_flags.tfexample_pattern,
      train_file_pattern=my_flags.train_file_pattern,
      validate_file_pattern=my_flags.validate_file_pattern,
      test_file_pattern=my_flags.test_file_pattern)
  some_dataset = test_brain_data.create_dataset('train')
  test_model = create_brain_model(my_flags, some_dataset)
  train_results, test_results = train_and_test(my_flags, test_brain_data, test_model,
                                               epochs=my_flags.epoch_count)
  # what a saved model carries besides its weights: the options (infer builds its datasets from
  # them) and the shapes of the model's inputs and output
  test_model.add_metadata(my_flags.as_dict(), dataset=some_dataset)

  dprime, final_decoder = None, None
  if my_flags.dnn_regressor != 'classifier':      # (no decoder is built around a classifier)
    dprime, final_decoder = train_lda_model(test_brain_data, test_model, my_flags)

  logging.info('train_and_test got these results: %s and test %s', train_results, test_results)
  print('train_and_test got these results: %s and test %s' % (train_results, test_results))
  if dprime is not None:
    logging.info('Calculated dprime is %g.', dprime)
    print('Calculated dprime is %g.' % dprime)

  if my_flags.summary_dir:
    write_experiment_summary(my_flags, train_results, test_results, dprime)
    print('Wrote train/test results to %s.' % my_flags.summary_dir)

  if my_flags.saved_model_dir and final_decoder is not None:
    os.makedirs(my_flags.saved_model_dir, exist_ok=True)
    # the fitted model goes INSIDE decoder_model.json (key 'decoding_model'): the directory keeps
    # its one file, and infer.load_model finds both halves there
    final_decoder.save_parameters(
        os.path.join(my_flags.saved_model_dir, infer_decoder.DECODER_PARAM_FILE_NAME),
        decoding_model=brain_model.model_to_dict(test_model))
    print('Wrote saved model to %s.' % my_flags.saved_model_dir)
  return train_results, test_results, dprime


# ---------------------------------------------------------------- command line
_CHOICES = {
    'correlation_reducer': ['lda', 'first', 'second', 'mean', 'mean-squared'],
    'data': ['tfrecords'],
    'dnn_regressor': ['fullyconnected', 'tf', 'linear', 'linear_with_bias', 'cca', 'classifier'],
    'loss': ['mse', 'pearson'],
}
# The one flag whose default is not the option's (the reference defines it with '').
_FLAG_DEFAULTS = {'attended_field': ''}


def _parse_bool(text):
  if text.lower() in ('true', 't', '1', 'yes', 'y'):
    return True
  if text.lower() in ('false', 'f', '0', 'no', 'n'):
    return False
  raise argparse.ArgumentTypeError('not a boolean: %r' % text)


def make_parser():
  """One option per DecodingOptions field, under the reference's flag names.  A boolean is given as
  --flag, --noflag or --flag=true|false."""
  parser = argparse.ArgumentParser(prog='decoding', description=__doc__.split('\n')[0])
  for name, default in DecodingOptions._DEFAULTS:
    default = _FLAG_DEFAULTS.get(name, default)
    if isinstance(default, bool):
      parser.add_argument('--' + name, dest=name, nargs='?', const=True, default=default,
                          type=_parse_bool)
      parser.add_argument('--no' + name, dest=name, action='store_const', const=False)
    else:
      kind = str if default is None else type(default)
      parser.add_argument('--' + name, dest=name, default=default, type=kind,
                          choices=_CHOICES.get(name))
  return parser


def main(argv=None):
  """argv: the command line's arguments without the program name (None: sys.argv[1:])."""
  my_flags = DecodingOptions().set_flags(make_parser().parse_args(argv))
  run_decoding_experiment(my_flags)


if __name__ == '__main__':
  main()
