"""brain_model.fit_many / regression.jackknife_dnn without a GPU: the fold rule of fold_rows_used against Dataset's
own batching, the ctypes prototype of td_dnn_train_many against the C header, and every guard of fit_many (each
raises before any device call; past them a machine without a GPU gets HotPathUnavailable)."""
import re

import numpy as np
import pytest

from tests.dnn_common import make_files
from tests.test_cpu_dnn import _kind_of_ctype

LENGTHS = [101, 130, 95, 64, 37, 5]
BATCH = 32
HELD = [[]] + [[f] for f in range(len(LENGTHS))] + [[1, 4], [0, 5]]


def _files(c=3, d=2):
  return make_files(np.random.default_rng(0), LENGTHS, c, d)


def _dataset(files=None, offset=0, **kwargs):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(files or _files(), BATCH, 2, 2, input_offset=offset, **kwargs)


@pytest.mark.parametrize('offset', [-1, 0, 1])
def test_fold_rows_used_is_the_batching_of_the_remaining_files(offset):
  from telluride_decoding_amd import brain_model
  files = _files()
  ds = _dataset(files, offset)
  assert brain_model.fold_rows_used(ds) == ds.rows_used()
  assert brain_model.fold_rows_used(ds, []) == ds.rows_used()
  steps, swallowed = [], 0
  for held in HELD:
    rest = [f for f in range(len(files)) if f not in held]
    want = iter(_dataset([files[f] for f in rest], offset).rows_used())
    want = [0 if f in held else next(want) for f in range(len(files))]
    got = brain_model.fold_rows_used(ds, held)
    assert got == want, (offset, held)
    assert sum(got) % BATCH == 0
    steps.append(sum(got) // BATCH)
    # the tail of the stream swallows the whole 5-frame file and part of the file before it
    if 5 not in held and got[5] == 0 and got[4] < ds.zipped_lengths()[4] and 4 not in held:
      swallowed += 1
  if offset == 0:
    assert steps[:7] == [13, 10, 9, 10, 11, 12, 13]
  assert swallowed >= 2


def test_fold_rows_used_refuses_a_file_that_is_not_there():
  from telluride_decoding_amd import brain_model
  ds = _dataset()
  for held in ([6], [-1], [0, 17]):
    with pytest.raises(ValueError, match='held_out must name files'):
      brain_model.fold_rows_used(ds, held)


def test_argtypes_match_the_header_prototype():
  """td_dnn_train_many: as many argtypes as the prototype of include/td_hotpath.h has parameters, each of the
  parameter's kind (the method of tests/test_cpu_dnn.py).  Its name stays out of the td_mlp_* family's pattern."""
  from telluride_decoding_amd import _lib, device
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_dnn_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ['td_dnn_train_many']
  assert not re.fullmatch(r'td_mlpc?_\w+', 'td_dnn_train_many')
  kinds = []
  for param in protos['td_dnn_train_many'].split(','):
    words = param.replace('*', ' * ').split()
    assert len(words) >= 2 and words[-1].isidentifier(), param
    kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
  assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
  assert [_kind_of_ctype(t) for t in _lib.SIGNATURES['td_dnn_train_many']] == kinds
  # the cap of the binding is the header's
  cap = re.search(r'#define\s+TD_DNN_MANY_MAX_MODELS\s+(\d+)', raw)
  assert cap and int(cap.group(1)) == device.DNN_MANY_MAX_MODELS


def _models(ds, n, hidden=(8, 4), loss='mse'):
  from telluride_decoding_amd import brain_model
  out = []
  for i in range(n):
    m = brain_model.BrainModelDNN(ds, list(hidden), seed=i)
    m.compile(loss=loss)
    out.append(m)
  return out


def test_guards_raise_without_a_device(monkeypatch):
  from telluride_decoding_amd import brain_data, brain_model, device

  def no_device(*args, **kwargs):
    raise AssertionError('a guard let the call reach the device')
  monkeypatch.setattr(device, 'default_handle', no_device)
  monkeypatch.setattr(device, 'dnn_train_many', no_device)
  files = _files()
  ds = _dataset(files)
  good = _models(ds, 3)
  assert brain_model.fit_many([], ds) == []
  with pytest.raises(RuntimeError, match='compile'):                      # an uncompiled model
    brain_model.fit_many(good[:2] + [brain_model.BrainModelDNN(ds, [8, 4])], ds)
  with pytest.raises(TypeError, match='BrainModelDNN'):                   # a non-DNN model
    brain_model.fit_many(good[:2] + [brain_model.BrainModelLinearRegression(ds)], ds)
  with pytest.raises(ValueError, match='one architecture'):               # different widths
    brain_model.fit_many(good[:2] + _models(ds, 1, hidden=(8, 5)), ds)
  with pytest.raises(ValueError, match='one loss'):                       # different losses
    brain_model.fit_many(good[:2] + _models(ds, 1, loss='pearson'), ds)
  with pytest.raises(TypeError, match='brain_data.Dataset'):
    brain_model.fit_many(good, list(ds))
  with pytest.raises(ValueError, match='mixup_batch'):
    brain_model.fit_many(good, _dataset(files, mixup_batch=True))
  with pytest.raises(ValueError, match='limited to 2 minibatches'):       # max_batches set
    brain_model.fit_many(good, ds.take(2))
  with pytest.raises(ValueError, match='input_1 is 20 wide, the model 15'):   # _check_limits' own message
    brain_model.fit_many(good, brain_data.Dataset(make_files(np.random.default_rng(1), LENGTHS, 4, 2), BATCH, 2, 2))
  with pytest.raises(ValueError, match='3 models but 2 held_out'):
    brain_model.fit_many(good, ds, held_out=[[0], [1]])
  with pytest.raises(ValueError, match='held_out must name files'):       # an index out of range
    brain_model.fit_many(good, ds, held_out=[[0], [1], [6]])
  with pytest.raises(ValueError, match='model 2 is left with 5 frames, no full minibatch of 32'):
    brain_model.fit_many(good, ds, held_out=[[0], None, [0, 1, 2, 3, 4]])
  with pytest.raises(ValueError, match='3 models but 2 shuffle seeds'):
    brain_model.fit_many(good, ds, shuffle_seeds=[1, 2])
  with pytest.raises(ValueError, match='shuffle_seed must be in'):
    brain_model.fit_many(good, ds, shuffle_seeds=[1, None, -3])
  hist = brain_model.fit_many(good, ds, epochs=0)                         # nothing to do: fit's empty history
  assert [h.history for h in hist] == [{'loss': [], 'pearson_correlation_first': [], 'mse': []}] * 3


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
    regression.jackknife_dnn(ds, [8, 4])


def test_jackknife_dnn_checks_its_arguments():
  from telluride_decoding_amd import regression
  files = _files()
  ds = _dataset(files)
  with pytest.raises(ValueError, match='Could not find metric accuracy'):
    regression.jackknife_dnn(ds, [8, 4], test_metric='accuracy')
  with pytest.raises(ValueError, match='_route'):
    regression.jackknife_dnn(ds, [8, 4], _route='sequential')
  with pytest.raises(ValueError, match='at least two files'):
    regression.jackknife_dnn(_dataset(files[:1]), [8, 4])
  with pytest.raises(ValueError, match='folds must name files'):
    regression.jackknife_dnn(ds, [8, 4], folds=[6])
  with pytest.raises(ValueError, match='learning rate'):
    regression.jackknife_dnn(ds, [8, 4], learning_rates=())
