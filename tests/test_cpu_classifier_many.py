"""brain_model.fit_many for classifiers, brain_model.evaluate_many and regression.jackknife_classifier without a GPU
(DESIGN section 19): the ctypes prototype of td_clf_train_many against the C header, and every guard (each raises
before any device call; past them a machine without a GPU gets HotPathUnavailable)."""
import re

import numpy as np
import pytest

from tests.dnn_common import make_files
from tests.test_cpu_dnn import _kind_of_ctype

LENGTHS = [101, 130, 95, 64, 37, 5]
BATCH = 32


def _files(c=3, c2=2):
  return make_files(np.random.default_rng(0), LENGTHS, c, 1, c2=c2)


def _dataset(files=None, **kwargs):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(files or _files(), BATCH, 2, 2, 1, 1, **kwargs)


def _models(ds, n, hidden=(8, 4)):
  from telluride_decoding_amd import brain_model
  out = []
  for i in range(n):
    m = brain_model.BrainModelClassifier(ds, list(hidden), seed=i)
    m.compile()
    out.append(m)
  return out


def test_argtypes_match_the_header_prototype():
  """td_clf_train_many: exactly one prototype of that name, outside the td_mlp_* / td_mlpc_* / td_dnn_* patterns the
  other suites pin, and as many argtypes as it has parameters, each of the parameter's kind (the method of
  tests/test_cpu_dnn_many.py)."""
  from telluride_decoding_amd import _lib
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = re.findall(r'\bint\s+(td_clf_train_many)\s*\(([^)]*)\)\s*;', text)
  assert len(protos) == 1
  assert not re.fullmatch(r'td_mlpc?_\w+', 'td_clf_train_many')
  assert not re.fullmatch(r'td_dnn_\w+', 'td_clf_train_many')
  assert 'td_clf_train_many' in _lib.header_symbols()
  kinds = []
  for param in protos[0][1].split(','):
    words = param.replace('*', ' * ').split()
    assert len(words) >= 2 and words[-1].isidentifier(), param
    kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
  assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
  assert [_kind_of_ctype(t) for t in _lib.SIGNATURES['td_clf_train_many']] == kinds
  # td_mlpc_train's shared arguments in its order, then epochs, update, num_models, nine arrays, stats_dev
  names = [param.replace('*', ' ').split()[-1] for param in protos[0][1].split(',')]
  assert names[:3] == ['h', 'x_dev', 'ldx'] and names[3:5] == ['x2_dev', 'ldx2']
  assert names[-14:] == ['batch_rows', 'epochs', 'update', 'num_models', 'rows_used_host', 'params_dev_host',
                         'state_dev_host', 'lr_host', 'beta1_host', 'beta2_host', 'eps_host', 'step0_host',
                         'shuffle_seed_host', 'stats_dev']


def _no_device(monkeypatch):
  from telluride_decoding_amd import device

  def no_device(*args, **kwargs):
    raise AssertionError('a guard let the call reach the device')
  monkeypatch.setattr(device, 'default_handle', no_device)
  monkeypatch.setattr(device, 'clf_train_many', no_device)
  monkeypatch.setattr(device, 'dnn_train_many', no_device)
  monkeypatch.setattr(device, 'mlpc_train', no_device)


def test_fit_many_guards_raise_without_a_device(monkeypatch):
  from telluride_decoding_amd import brain_data, brain_model
  _no_device(monkeypatch)
  files = _files()
  ds = _dataset(files)
  good = _models(ds, 3)
  with pytest.raises(RuntimeError, match='compile'):                      # an uncompiled model
    brain_model.fit_many(good[:2] + [brain_model.BrainModelClassifier(ds, [8, 4])], ds)
  dnn = brain_model.BrainModelDNN(ds, [8, 4])
  dnn.compile()
  for mixed in (good[:2] + [dnn], [dnn] + good[:2]):                      # mixed classes
    with pytest.raises(ValueError, match='one model family'):
      brain_model.fit_many(mixed, ds)
  with pytest.raises(TypeError, match='BrainModelDNN'):                   # neither family
    brain_model.fit_many(good[:2] + [brain_model.BrainModelLinearRegression(ds)], ds)
  with pytest.raises(ValueError, match='one architecture'):               # unequal widths
    brain_model.fit_many(good[:2] + _models(ds, 1, hidden=(8, 5)), ds)
  with pytest.raises(TypeError, match='brain_data.Dataset'):
    brain_model.fit_many(good, list(ds))
  with pytest.raises(ValueError, match='mixup_batch'):
    brain_model.fit_many(good, _dataset(files, mixup_batch=True))
  with pytest.raises(ValueError, match='limited to 2 minibatches'):       # take()
    brain_model.fit_many(good, ds.take(2))
  with pytest.raises(ValueError, match='input_2 is 9 wide, the model 6'):     # _check_limits' own message
    brain_model.fit_many(good, brain_data.Dataset(make_files(np.random.default_rng(1), LENGTHS, 3, 1, c2=3), BATCH,
                                                  2, 2, 1, 1))
  with pytest.raises(ValueError, match='3 models but 2 held_out'):        # wrong list lengths
    brain_model.fit_many(good, ds, held_out=[[0], [1]])
  with pytest.raises(ValueError, match='3 models but 2 shuffle seeds'):
    brain_model.fit_many(good, ds, shuffle_seeds=[1, 2])
  with pytest.raises(ValueError, match='held_out must name files'):       # a file index out of range
    brain_model.fit_many(good, ds, held_out=[[0], [1], [6]])
  with pytest.raises(ValueError, match='model 2 is left with 5 frames, no full minibatch of 32'):
    brain_model.fit_many(good, ds, held_out=[[0], None, [0, 1, 2, 3, 4]])
  with pytest.raises(ValueError, match='shuffle_seed must be in'):        # bad shuffle seed
    brain_model.fit_many(good, ds, shuffle_seeds=[1, None, -3])
  with pytest.raises(ValueError, match='shuffle_seed must be in'):
    brain_model.fit_many(good, ds, shuffle_seeds=2 ** 63)
  with pytest.raises(NotImplementedError, match='amsgrad'):               # compile refuses it ...
    brain_model.BrainModelClassifier(ds, [8, 4]).compile(optimizer=brain_model.Adam(amsgrad=True))
  good[1].optimizer.amsgrad = True                                        # ... and fit_many, set behind its back
  with pytest.raises(NotImplementedError, match=r'amsgrad=True is not supported \(model 1\)'):
    brain_model.fit_many(good, ds)
  good[1].optimizer.amsgrad = False
  hist = brain_model.fit_many(good, ds, epochs=0)                         # nothing to do: fit's empty history
  assert [h.history for h in hist] == [{'loss': [], 'accuracy': []}] * 3
  assert [m._updates for m in good] == [0, 0, 0] and all(m._state is None for m in good)


def test_evaluate_many_guards_raise_without_a_device(monkeypatch):
  from telluride_decoding_amd import brain_model
  _no_device(monkeypatch)
  files = _files()
  ds = _dataset(files)
  good = _models(ds, 3)
  dnn = brain_model.BrainModelDNN(ds, [8, 4])
  assert brain_model.evaluate_many([], ds, files=[]) == []
  with pytest.raises(TypeError, match='BrainModelClassifier'):            # mixed classes
    brain_model.evaluate_many(good[:2] + [dnn], ds, files=[[0], [1], [2]])
  with pytest.raises(ValueError, match='one architecture'):               # unequal widths
    brain_model.evaluate_many(good[:2] + _models(ds, 1, hidden=(8, 5)), ds, files=[[0], [1], [2]])
  with pytest.raises(TypeError, match='brain_data.Dataset'):
    brain_model.evaluate_many(good, list(ds), files=[[0], [1], [2]])
  with pytest.raises(ValueError, match='mixup_batch'):
    brain_model.evaluate_many(good, _dataset(files, mixup_batch=True), files=[[0], [1], [2]])
  with pytest.raises(ValueError, match='limited to 2 minibatches'):
    brain_model.evaluate_many(good, ds.take(2), files=[[0], [1], [2]])
  with pytest.raises(ValueError, match='3 models but 2 files'):           # wrong list lengths
    brain_model.evaluate_many(good, ds, files=[[0], [1]])
  for bad in ([6], [-1]):                                                 # a file index out of range
    with pytest.raises(ValueError, match=r'files\[2\] must name files'):
      brain_model.evaluate_many(good, ds, files=[[0], [1], bad])
  # files without a minibatch: NaN, and with none left there is no device call at all
  out = brain_model.evaluate_many(good, ds, files=[[5], [], [5]])
  assert len(out) == 3 and all(np.isnan(o['loss']) and np.isnan(o['accuracy']) for o in out)
  # an uncompiled model is scored as evaluate scores it: past the guards (no device here: the call is reached)
  with pytest.raises(AssertionError, match='reach the device'):
    brain_model.evaluate_many([brain_model.BrainModelClassifier(ds, [8, 4])], ds, files=[[0]])


def test_jackknife_classifier_checks_its_arguments(monkeypatch):
  from telluride_decoding_amd import regression
  _no_device(monkeypatch)
  files = _files()
  ds = _dataset(files)
  with pytest.raises(ValueError, match='Could not find metric pearson_correlation_first'):
    regression.jackknife_classifier(ds, [8, 4], test_metric='pearson_correlation_first')
  with pytest.raises(ValueError, match='_route'):
    regression.jackknife_classifier(ds, [8, 4], _route='sequential')
  with pytest.raises(ValueError, match='at least two files'):
    regression.jackknife_classifier(_dataset(files[:1]), [8, 4])
  for folds in ([6], [-1, 2], []):                                        # a file index out of range
    with pytest.raises(ValueError, match='folds must name files'):
      regression.jackknife_classifier(ds, [8, 4], folds=folds)
  with pytest.raises(ValueError, match='learning rate'):
    regression.jackknife_classifier(ds, [8, 4], learning_rates=())
  for route in ('batched', 'per_fold'):
    with pytest.raises(ValueError, match='shuffle_seed must be in'):      # bad shuffle seed
      regression.jackknife_classifier(ds, [8, 4], shuffle_seed=-1, _route=route)
  with pytest.raises(ValueError, match='mixup_batch'):
    regression.jackknife_classifier(_dataset(files, mixup_batch=True), [8, 4], _route='batched')
  with pytest.raises(ValueError, match='limited to 2 minibatches'):
    regression.jackknife_classifier(ds.take(2), [8, 4], _route='batched')
  # a fold without a minibatch: two short files, each fold's training stream is the other one
  short = _dataset(make_files(np.random.default_rng(2), [40, 20], 3, 1, c2=2))
  with pytest.raises(ValueError, match='model 0 is left with 20 frames, no full minibatch of 32'):
    regression.jackknife_classifier(short, [8, 4], _route='batched')


def test_past_the_guards_there_is_no_cpu_fallback():
  from telluride_decoding_amd import _lib, brain_model, device, regression
  ds = _dataset()
  models = _models(ds, 2)
  if device.gpu_available():
    hist = brain_model.fit_many(models, ds, held_out=[None, [1]])
    assert [len(h.history['loss']) for h in hist] == [1, 1]
    return
  with pytest.raises(_lib.HotPathUnavailable):
    brain_model.fit_many(models, ds, held_out=[None, [1]])
  with pytest.raises(_lib.HotPathUnavailable):
    brain_model.evaluate_many(models, ds, files=[[0], [1]])
  with pytest.raises(_lib.HotPathUnavailable):
    regression.jackknife_classifier(ds, [8, 4])
