"""Saved models on the GPU: each of the four model classes is fitted, saved,
loaded with brain_model.load_model, and the loaded model predicts and evaluates exactly as the original."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILES, FRAMES, CHANNELS = 2, 600, 8


@pytest.fixture(scope='module')
def datasets():
  """Two recordings of 600 frames and 8 channels, post_context = 3: one dataset with two regression targets
  (and a two-channel input 2 with a context of its own, for CCA), one with a 0/1 label for the classifier."""
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(24)
  regress, classify = [], []
  for _ in range(FILES):
    x = rng.standard_normal((FRAMES, CHANNELS)).astype(np.float32)
    x2 = (x[:, :2] + 0.5 * rng.standard_normal((FRAMES, 2))).astype(np.float32)
    y = (x[:, :2] @ np.array([[1.0, -0.5], [0.25, 2.0]]) + 0.1 * rng.standard_normal((FRAMES, 2))).astype(np.float32)
    label = (rng.uniform(size=(FRAMES, 1)) < 0.5).astype(np.float32)
    zeros = np.zeros((FRAMES, 1), np.float32)
    regress.append((x, x2, y, zeros))
    classify.append((x, x2, label, zeros))
  make = lambda files: brain_data.Dataset(files, 100, 0, 3, 0, 2)
  return make(regress), make(classify)


def _models(regress, classify):
  from telluride_decoding_amd import brain_model, cca
  linear = brain_model.BrainModelLinearRegression(regress, 0.1)
  linear.compile()
  dnn = brain_model.BrainModelDNN(regress, [8, 4], seed=3)
  dnn.compile(learning_rate=0.01)
  classifier = brain_model.BrainModelClassifier(classify, [8], seed=4)
  classifier.compile(learning_rate=0.01)
  cca_model = cca.BrainModelCCA(regress, cca_dims=2, regularization_lambda=0.01)
  cca_model.compile()
  return [('linear', linear, regress), ('dnn', dnn, regress), ('classifier', classifier, classify),
          ('cca', cca_model, regress)]


@pytest.mark.parametrize('index', range(4), ids=['linear', 'dnn', 'classifier', 'cca'])
def test_saved_model_predicts_and_evaluates_as_the_original(datasets, tmp_path, index):
  from telluride_decoding_amd import brain_model
  name, model, ds = _models(*datasets)[index]
  if name in ('dnn', 'classifier'):
    model.fit(ds, epochs=2, shuffle_seed=1)
  else:
    model.fit(ds)
  model.add_metadata({'model': name}, ds)
  model_dir = str(tmp_path / name)
  model.save(model_dir)
  assert os.listdir(model_dir) == ['brain_model.json']
  loaded = brain_model.load_model(model_dir)
  assert type(loaded) is type(model) and loaded is not model
  assert loaded.telluride_metadata == {'model': name}
  for got, want in zip(loaded.weight_matrices, model.weight_matrices):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()

  want, got = model.predict(ds), loaded.predict(ds)
  assert want.shape[0] == FILES * FRAMES and np.all(np.isfinite(want)) and np.any(want != 0)
  assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
  for feats, _ in ds:                              # ... and on one already-lagged minibatch (`call`)
    want_call, got_call = np.asarray(model.call(feats)), np.asarray(loaded.call(feats))
    assert want_call.shape[0] == 100 and got_call.tobytes() == want_call.tobytes()
    break
  want_eval, got_eval = model.evaluate(ds), loaded.evaluate(ds)
  assert set(got_eval) == set(want_eval) and all(np.isfinite(v) for v in want_eval.values())
  assert got_eval == want_eval
  # a loaded model trains on: compiled as the original was, with a fresh optimizer
  if name in ('dnn', 'classifier'):
    assert vars(loaded.optimizer) == vars(model.optimizer)
    history = loaded.fit(ds, epochs=1).history
    assert len(history['loss']) == 1 and np.isfinite(history['loss'][0])
