"""Saved models without a GPU: model_to_dict -> JSON -> model_from_dict keeps every
weight bit for bit, add_metadata's contents and TypeError, restore_parameters on a decoder_model.json that
also holds the model, and infer.load_model's error cases (reference test/infer_test.py:209-227)."""
import json
import os

import numpy as np
import pytest

from telluride_decoding_amd import brain_data
from telluride_decoding_amd import brain_model
from telluride_decoding_amd import cca
from telluride_decoding_amd import infer
from telluride_decoding_amd import infer_decoder


def _dataset(frames=40, c1=6, c2=3, d=2, pre=0, post=3, pre2=0, post2=1, batch=10):
  rng = np.random.default_rng(3)
  f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
  return brain_data.Dataset([(f32(frames, c1), f32(frames, c2), f32(frames, d), np.zeros((frames, 1), np.float32))],
                            batch, pre, post, pre2, post2)


def _round_trip(model):
  text = json.dumps(brain_model.model_to_dict(model))
  return brain_model.model_from_dict(json.loads(text))


def _same_bits(got, want):
  assert len(got) == len(want)
  for g, w in zip(got, want):
    g, w = np.asarray(g), np.asarray(w)
    assert g.dtype == w.dtype and g.shape == w.shape
    assert g.tobytes() == w.tobytes()


def _awkward(rng, shape, dtype):
  """Values whose bits a decimal round trip would not keep for free: denormals, -0, huge, tiny, NaN payloads aside."""
  a = rng.standard_normal(shape).astype(dtype)
  flat = a.reshape(-1)
  specials = [np.finfo(dtype).tiny / 4, -0.0, np.finfo(dtype).max, np.finfo(dtype).eps / 3, np.inf, 1.0 / 3.0]
  flat[:min(len(specials), flat.size)] = np.asarray(specials[:flat.size], dtype)
  return a


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_array_round_trip_is_bit_exact(dtype):
  rng = np.random.default_rng(0)
  for shape in ((7, 3), (5,), (0, 4), ()):
    a = _awkward(rng, shape, dtype)
    d = json.loads(json.dumps(brain_model.array_to_dict(a)))
    assert set(d) == {'dtype', 'shape', 'data'} and d['dtype'] == np.dtype(dtype).name
    _same_bits([brain_model.array_from_dict(d)], [a])
  big = np.arange(6, dtype='>f8').reshape(2, 3)            # a big-endian array is stored little-endian
  d = brain_model.array_to_dict(big)
  assert np.frombuffer(__import__('base64').b64decode(d['data']), '<f8').tolist() == big.reshape(-1).tolist()
  _same_bits([brain_model.array_from_dict(d)], [big.astype('f8')])


def test_linear_regression_round_trip():
  ds = _dataset()
  model = brain_model.BrainModelLinearRegression(ds, 0.25)
  rng = np.random.default_rng(1)
  model.set_weights([_awkward(rng, (ds.input1_width, 2), np.float32), _awkward(rng, (2,), np.float32)])
  loaded = _round_trip(model)
  assert type(loaded) is brain_model.BrainModelLinearRegression
  _same_bits(loaded.weight_matrices, model.weight_matrices)
  assert (loaded._input_width, loaded._output_width, loaded._regularization_lambda) == (ds.input1_width, 2, 0.25)
  assert (loaded._c1, loaded._pre, loaded._post) == (6, 0, 3)
  unfit = _round_trip(brain_model.BrainModelLinearRegression(ds))
  assert unfit.w_estimate is None and unfit.b_estimate is None


@pytest.mark.parametrize('hidden', [[], [8, 4]])
def test_dnn_round_trip(hidden):
  ds = _dataset()
  model = brain_model.BrainModelDNN(ds, list(hidden), seed=5)
  model.compile(optimizer=brain_model.RMSprop(learning_rate=0.02, rho=0.8, epsilon=1e-6), loss='pearson')
  rng = np.random.default_rng(2)
  model.set_weights([_awkward(rng, w.shape, np.float32) for w in model.get_weights()])
  d = brain_model.model_to_dict(model)
  assert d['format_version'] == brain_model.MODEL_FORMAT_VERSION and d['class_name'] == 'BrainModelDNN'
  assert d['constructor'] == {'input_widths': [ds.input1_width], 'output_width': 2, 'num_hidden_list': list(hidden),
                              'seed': 5}
  assert d['compile'] == {'optimizer': {'class': 'RMSprop', 'config': {
      'learning_rate': 0.02, 'rho': 0.8, 'momentum': 0.0, 'epsilon': 1e-6, 'centered': False}}, 'loss': 'pearson'}
  loaded = _round_trip(model)
  assert type(loaded) is brain_model.BrainModelDNN and loaded.num_hidden_list == list(hidden)
  _same_bits(loaded.get_weights(), model.get_weights())
  assert loaded.loss == 'pearson' and vars(loaded.optimizer) == vars(model.optimizer)
  assert loaded.optimizer is not model.optimizer and loaded._state is None      # a fresh optimizer
  # a model that was never compiled stays uncompiled
  assert _round_trip(brain_model.BrainModelDNN(ds, list(hidden))).optimizer is None


def test_classifier_round_trip():
  ds = _dataset(d=1)
  model = brain_model.BrainModelClassifier(ds, [8, 4], seed=9)
  model.compile(optimizer=brain_model.Adam(learning_rate=0.003, beta_1=0.8), learning_rate=0.003)
  rng = np.random.default_rng(4)
  model.set_weights([_awkward(rng, w.shape, np.float32) for w in model.get_weights()])
  loaded = _round_trip(model)
  assert type(loaded) is brain_model.BrainModelClassifier
  assert (loaded._input_width, loaded._input2_width) == (ds.input1_width, ds.input2_width)
  _same_bits(loaded.get_weights(), model.get_weights())
  assert vars(loaded.optimizer) == vars(model.optimizer) and loaded._updates == 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cca_round_trip(dtype):
  ds = _dataset()
  model = cca.BrainModelCCA(ds, cca_dims=3, regularization_lambda=0.5)
  rng = np.random.default_rng(6)
  k1, k2 = ds.input1_width, ds.input2_width
  model.set_weights([_awkward(rng, (1, k1), dtype), _awkward(rng, (1, k2), dtype), _awkward(rng, (k1, 3), dtype),
                     _awkward(rng, (k2, 3), dtype)])
  loaded = _round_trip(model)
  assert type(loaded) is cca.BrainModelCCA and loaded.output_dims == model.output_dims == 3
  assert (loaded._cca_dims, loaded._regularization_lambda) == (3, 0.5)
  _same_bits(loaded.weight_matrices, model.weight_matrices)
  _same_bits([loaded.mean_x, loaded.mean_y, loaded.rot_x, loaded.rot_y], model.get_weights())
  assert all(w is None for w in _round_trip(cca.BrainModelCCA(ds)).weight_matrices)


def test_save_and_load_model_files(tmp_path):
  ds = _dataset()
  model = brain_model.BrainModelLinearRegression(ds, 0.1)
  model.set_weights([np.ones((ds.input1_width, 2), np.float32) / 3, np.arange(2, dtype=np.float32)])
  model.add_metadata({'input_field': 'eeg', 'pre_context': 0}, ds)
  model_dir = str(tmp_path / 'nested' / 'linear_model')
  model.save(model_dir)
  assert os.listdir(model_dir) == ['brain_model.json']
  loaded = brain_model.load_model(model_dir)
  _same_bits(loaded.weight_matrices, model.weight_matrices)
  assert loaded.telluride_metadata == {'input_field': 'eeg', 'pre_context': 0}
  assert loaded.telluride_inputs == model.telluride_inputs and loaded.telluride_output == [None, 2]
  with pytest.raises(ValueError, match='format version'):
    brain_model.model_from_dict(dict(brain_model.model_to_dict(model), format_version=99))
  with pytest.raises(TypeError):
    brain_model.model_to_dict(object())


def test_add_metadata():
  ds = _dataset()
  for model in (brain_model.BrainModelLinearRegression(ds), brain_model.BrainModelDNN(ds, [4]),
                brain_model.BrainModelClassifier(_dataset(d=1), [4]), cca.BrainModelCCA(ds)):
    flags = {'input_field': 'eeg', 'post_context': 3, 'saved_model_dir': None, 'frame_rate': 100.0}
    model.add_metadata(flags)
    assert model.telluride_metadata == flags and not hasattr(model, 'telluride_inputs')
    model.add_metadata(flags, dataset=ds)
    assert model.telluride_inputs == {'input_1': [None, ds.input1_width], 'input_2': [None, ds.input2_width],
                                      'attended_speaker': [None, 1]}
    assert model.telluride_output == [None, ds.d]
    json.dumps([model.telluride_metadata, model.telluride_inputs, model.telluride_output])
    # any iterable of minibatches: the first one's shapes, batch size included (reference brain_model.py:274-280)
    batches = [({'input_1': np.zeros((10, 24)), 'input_2': np.zeros((10, 6))}, np.zeros((10, 2)))]
    model.add_metadata(flags, dataset=batches)
    assert model.telluride_inputs == {'input_1': [10, 24], 'input_2': [10, 6]} and model.telluride_output == [10, 2]
    with pytest.raises(TypeError, match='dataset parameter must be tf.data.Dataset type.'):
      model.add_metadata(flags, dataset=42)
    with pytest.raises(TypeError):                       # the flags must be JSON-able
      model.add_metadata({'bad': object()})
    d = json.loads(json.dumps(brain_model.model_to_dict(model)))
    assert d['telluride_metadata'] == flags and d['telluride_output'] == [10, 2]


def _decoder_with_parameters():
  dec = infer_decoder.LinearRegressionDecoder(lambda d: d['input_1'], reduction='lda')
  rng = np.random.default_rng(8)
  dec._set_correlation_params([17] + [rng.standard_normal(2) for _ in range(7)])
  return dec


def test_restore_parameters_ignores_the_embedded_model(tmp_path):
  dec = _decoder_with_parameters()
  plain, with_model = str(tmp_path / 'plain.json'), str(tmp_path / 'decoder_model.json')
  dec.save_parameters(plain)
  model = brain_model.BrainModelLinearRegression(_dataset())
  model.set_weights([np.ones((24, 2), np.float32), np.zeros(2, np.float32)])
  dec.save_parameters(with_model, decoding_model=brain_model.model_to_dict(model))
  with open(plain) as f:
    plain_contents = json.load(f)
  with open(with_model) as f:
    contents = json.load(f)
  assert list(plain_contents) == ['correlation_params', 'lda_params']        # the output of before
  assert list(contents) == ['correlation_params', 'lda_params', 'decoding_model']
  assert {k: contents[k] for k in plain_contents} == plain_contents
  for path in (plain, with_model):
    other = infer_decoder.LinearRegressionDecoder(lambda d: d['input_1'], reduction='lda')
    other.restore_parameters(path)
    assert other.correlation_params.count == 17
    for got, want in zip(other.correlation_params[1:], dec.correlation_params[1:]):
      np.testing.assert_array_equal(got, want)
  # ... and load_decoding_model finds the model there when the directory has no brain_model.json
  loader = infer_decoder.LinearRegressionDecoder(reduction='lda')
  loader.load_decoding_model(str(tmp_path), {})
  _same_bits(loader.decoding_model.weight_matrices, model.weight_matrices)
  assert loader.decoding_model_params == {} and loader.model_inputs == {'input_1': (None, 24)}


def test_load_decoding_model(tmp_path):
  ds = _dataset()
  model = cca.BrainModelCCA(ds, cca_dims=2)
  rng = np.random.default_rng(10)
  model.set_weights([rng.standard_normal((1, 24)), rng.standard_normal((1, 6)), rng.standard_normal((24, 2)),
                     rng.standard_normal((6, 2))])
  model.add_metadata({'input_field': 'eeg'}, ds)
  model_dir = str(tmp_path / 'cca_model')
  model.save(model_dir)
  dec = infer_decoder.CCADecoder(reduction='first')
  with pytest.raises(TypeError, match=r'Must provide a file name \(string\) to load-model'):
    dec.load_decoding_model(None, {})
  with pytest.raises(TypeError, match='If providing an object dictionary, it must be a dict'):
    dec.load_decoding_model(model_dir, ['not', 'a', 'dict'])
  with pytest.raises(IOError, match='SavedModel file does not exist at: %s' % str(tmp_path / 'nowhere')):
    dec.load_decoding_model(str(tmp_path / 'nowhere'), {})
  dec.load_decoding_model(model_dir, {'BrainCcaLayer': cca.BrainCcaLayer})
  assert isinstance(dec.decoding_model, cca.BrainModelCCA)
  assert dec.decoding_model_params == {'input_field': 'eeg'}
  assert dec.model_inputs == {'input_1': [None, 24], 'input_2': [None, 6], 'attended_speaker': [None, 1]}
  assert dec.model_output == [None, 2]
  dec.check_model_and_data(ds)
  with pytest.raises(TypeError, match='has the wrong shape'):
    dec.check_model_and_data(_dataset(c1=5))


def test_load_model_errors(tmp_path):
  """Reference test/infer_test.py:209-227."""
  with pytest.raises(ValueError, match='Couldn\'t determine model type'):
    infer.load_model('/foo/bar', 'none')
  with pytest.raises(ValueError, match='Unknown reduction technique'):
    infer.load_model('/foo/cca', 'none')
  with pytest.raises(IOError, match='SavedModel file does not exist|No file or directory found'):
    infer.load_model('/foo/cca', 'lda')
  # a model directory without decoder_model.json
  model = brain_model.BrainModelLinearRegression(_dataset())
  model_dir = str(tmp_path / 'linear_model')
  model.save(model_dir)
  with pytest.raises(IOError, match='Can not load decoder model parameters from %s' %
                     os.path.join(model_dir, 'decoder_model.json')):
    infer.load_model(model_dir, 'lda')
  # ... and with it
  _decoder_with_parameters().save_parameters(os.path.join(model_dir, 'decoder_model.json'))
  loaded = infer.load_model(model_dir, 'first')
  assert isinstance(loaded, infer_decoder.LinearRegressionDecoder) and loaded.correlation_params.count == 17
  assert isinstance(loaded.decoding_model, brain_model.BrainModelLinearRegression)
