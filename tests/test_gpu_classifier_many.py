"""brain_model.fit_many for classifiers, brain_model.evaluate_many and regression.jackknife_classifier on the MI355X
(DESIGN section 19).  The yardsticks are the single-model path, BrainModelClassifier.fit / evaluate on a Dataset of
the fold's files -- pinned to float64 by tests/test_gpu_classifier.py -- which a batched model must equal bit for bit,
and the float64 restatement of tests/host_classifier.py itself, with test_gpu_classifier.py's trajectory bounds.

One recipe throughout: 3 channels, pre 2 / post 2 (K1 = 15) and a second view of 2 channels, pre2 1 / post2 1 (K2 = 6):
K = 21, W1 slices of 4, 4, 4, 4, 4 and 1 rows, the fourth across the two views; hidden [8, 4], 1 output, minibatches of
32, six recordings of 101, 130, 95, 64, 37 and 5 frames, 3 epochs; seven models: every recording, then each of the six
held out (9 .. 13 steps an epoch, so most models idle through the last rounds of a call; the folds' streams lose the
whole last recording).  Every model has its own learning_rate, beta_1, beta_2 and epsilon."""
import functools

import numpy as np
import pytest

from tests import host_classifier as hc
from tests import host_dnn
from tests import parity_log
from tests.dnn_common import make_files

pytestmark = pytest.mark.gpu

C, PRE, POST, C2, PRE2, POST2, D, BATCH, HIDDEN, EPOCHS = 3, 2, 2, 2, 1, 1, 1, 32, [8, 4], 3
LENGTHS = [101, 130, 95, 64, 37, 5]
WIDTHS = [C * (PRE + 1 + POST) + C2 * (PRE2 + 1 + POST2)] + HIDDEN + [D]
HELD = [[]] + [[f] for f in range(len(LENGTHS))]        # model 0: nothing held out; model f + 1: recording f
STEPS = [13, 10, 9, 10, 11, 12, 13]
SHUFFLE = 12345
SEEDS = [21, 22, 23, 24, 25, 26, 27]
ADAM = [dict(learning_rate=lr, beta_1=b1, beta_2=b2, epsilon=eps) for lr, b1, b2, eps in (
    (1e-3, 0.9, 0.999, 1e-7), (3e-3, 0.8, 0.99, 1e-6), (2e-3, 0.85, 0.995, 1e-8), (5e-4, 0.95, 0.9995, 3e-7),
    (4e-3, 0.7, 0.98, 1e-5), (1.5e-3, 0.92, 0.9985, 2e-7), (2.5e-3, 0.88, 0.997, 5e-8))]
NUM_MODELS_ARG = 22                                     # td_clf_train_many's num_models, counted from the handle


def _dataset(files, offset=0):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(files, BATCH, PRE, POST, PRE2, POST2, input_offset=offset)


def _without(files, held):
  return [f for i, f in enumerate(files) if i not in held]


def _snapshot(model):
  """(weights, Adam's m and v, the updates applied) of a model as host values."""
  state = None if model._state is None else model._state.cpu().numpy().copy()
  return [w.copy() for w in model.get_weights()], state, model._updates


def _assert_same_bits(got, want, what):
  for a, b in zip(got[0], want[0]):
    np.testing.assert_array_equal(a, b, err_msg='weights of %s' % (what,))
  np.testing.assert_array_equal(got[1], want[1], err_msg='m, v of %s' % (what,))
  assert got[2] == want[2], ('_updates of %s' % (what,), got[2], want[2])


def _new_models(ds, seeds, settings):
  from telluride_decoding_amd import brain_model
  models = []
  for seed, adam in zip(seeds, settings):
    m = brain_model.BrainModelClassifier(ds, HIDDEN, seed=seed)
    m.compile(optimizer=brain_model.Adam(**adam))
    models.append(m)
  return models


@functools.lru_cache(maxsize=None)
def _files():
  return make_files(np.random.default_rng(169), LENGTHS, C, D, c2=C2)


@functools.lru_cache(maxsize=None)
def _sequential(shuffle):
  """The yardstick: every model by its own BrainModelClassifier.fit on a Dataset of the recordings it trains on."""
  out = []
  for held, seed, adam in zip(HELD, SEEDS, ADAM):
    ds = _dataset(_without(_files(), held))
    m, = _new_models(ds, [seed], [adam])
    hist = m.fit(ds, epochs=EPOCHS, shuffle_seed=shuffle).history
    out.append((_snapshot(m), hist))
  return out


def _batched(shuffle):
  from telluride_decoding_amd import brain_model
  ds = _dataset(_files())
  models = _new_models(ds, SEEDS, ADAM)
  hists = brain_model.fit_many(models, ds, held_out=HELD, epochs=EPOCHS, shuffle_seeds=shuffle)
  return [(_snapshot(m), h.history) for m, h in zip(models, hists)], models


# ---- 1. bit for bit the single fit -------------------------------------------------------------------------
@pytest.mark.parametrize('shuffle', [None, SHUFFLE], ids=['in_order', 'shuffled'])
def test_every_model_equals_its_own_fit(shuffle):
  from telluride_decoding_amd import brain_model
  assert [sum(brain_model.fold_rows_used(_dataset(_files()), h)) // BATCH for h in HELD] == STEPS
  want = _sequential(shuffle)
  got, _ = _batched(shuffle)
  for i, ((snap_g, hist_g), (snap_w, hist_w)) in enumerate(zip(got, want)):
    _assert_same_bits(snap_g, snap_w, (shuffle, 'model %d' % i))
    assert snap_g[2] == EPOCHS * STEPS[i]
    assert hist_g == hist_w, (shuffle, i)
    assert sorted(hist_g) == ['accuracy', 'loss']
    assert all(len(v) == EPOCHS and np.all(np.isfinite(v)) for v in hist_g.values())
  # the models did train, their Adam state is there, and they are apart from each other
  assert not np.array_equal(got[0][0][0][0], host_dnn.glorot(WIDTHS, SEEDS[0])[0])
  assert np.count_nonzero(got[0][0][1]) > 0
  assert not np.array_equal(got[1][0][0][0], got[3][0][0][0])


# ---- 2. continuation ---------------------------------------------------------------------------------------
def test_two_calls_continue_as_one():
  """2 + 2 epochs = 4 epochs in bits: Adam's t (step0 of the lr_t table), m and v carry over.  Model 2 starts from the
  10 updates of a single fit on its own fold, and is also followed through single fits alone."""
  from telluride_decoding_amd import brain_model
  ds = _dataset(_files())
  fold2 = _dataset(_without(_files(), HELD[2]))
  once, twice = _new_models(ds, SEEDS, ADAM), _new_models(ds, SEEDS, ADAM)
  alone, = _new_models(fold2, SEEDS[2:3], ADAM[2:3])
  for m in (once[2], twice[2], alone):
    m.fit(fold2, epochs=1)
    assert m._updates == STEPS[2]
  h4 = brain_model.fit_many(once, ds, held_out=HELD, epochs=4)
  h2a = brain_model.fit_many(twice, ds, held_out=HELD, epochs=2)
  h2b = brain_model.fit_many(twice, ds, held_out=HELD, epochs=2)
  for i, (a, b) in enumerate(zip(twice, once)):
    _assert_same_bits(_snapshot(a), _snapshot(b), 'model %d' % i)
    assert a._updates == 4 * STEPS[i] + (STEPS[2] if i == 2 else 0)
    for key in ('loss', 'accuracy'):
      assert h2a[i].history[key] + h2b[i].history[key] == h4[i].history[key]
  halone = alone.fit(fold2, epochs=4).history
  _assert_same_bits(_snapshot(once[2]), _snapshot(alone), 'model 2 against single fits')
  assert h4[2].history == halone


# ---- 3. scoring ----------------------------------------------------------------------------------------------
def test_evaluate_many_is_every_models_own_evaluate():
  from telluride_decoding_amd import brain_model
  files = _files()
  ds = _dataset(files)
  _, models = _batched(SHUFFLE)
  before = [_snapshot(m) for m in models]
  scored = [[]] + [[f] for f in range(len(files))] + [[1, 3], [3, 1, 5]]
  entrants = models + [models[0], models[0]]                 # (one model may be scored more than once)
  got = brain_model.evaluate_many(entrants, ds, files=scored)
  assert len(got) == 9 and all(sorted(g) == ['accuracy', 'loss'] for g in got)
  assert np.isnan(got[0]['loss']) and np.isnan(got[0]['accuracy'])           # no file at all
  for f in range(len(files)):
    want = models[f + 1].evaluate(_dataset([files[f]]))
    if f == 5:                                               # 5 frames are no minibatch: Keras' empty mean
      assert np.isnan(want['loss']) and np.isnan(got[6]['loss']) and np.isnan(got[6]['accuracy'])
      continue
    assert np.isfinite(want['loss']) and 0.0 <= want['accuracy'] <= 1.0
    assert got[f + 1] == want, (f, got[f + 1], want)
  want = models[0].evaluate(_dataset([files[1], files[3]]))
  assert got[7] == want and np.isfinite(want['loss'])
  assert got[8] == models[0].evaluate(_dataset([files[1], files[3], files[5]]))
  for i, (m, snap) in enumerate(zip(models, before)):
    _assert_same_bits(_snapshot(m), snap, 'model %d after scoring' % i)


# ---- 4. the float64 restatement ----------------------------------------------------------------------------
F64_HELD, F64_RATES, F64_EPOCHS, F64_MARGIN, F64_DRAWS = [[], [1], [4]], [1e-3, 3e-3, 1e-3], 2, 1e-5, 4


@functools.lru_cache(maxsize=None)
def float64_case(offset, shuffle):
  """Host only.  Draw d: the recordings of default_rng(270 + d), model i from the weights of seed d + i.  The first draw
  of at most four in which, in float64, every hidden pre-activation and output logit of the three trajectories and of
  their held-out scorings stays 1e-5 (relative to its sum of |terms|: host_classifier's margin) away from 0."""
  for draw in range(F64_DRAWS):
    files = make_files(np.random.default_rng(270 + draw), LENGTHS, C, D, c2=C2)
    runs, margin = [], np.inf
    for mi, (held, lr) in enumerate(zip(F64_HELD, F64_RATES)):
      x64, y64 = hc.stream(_without(files, held), BATCH, PRE, POST, PRE2, POST2, input_offset=offset)
      w64, _, hist64, mg = hc.train(host_dnn.glorot(WIDTHS, draw + mi), x64, y64, BATCH, F64_EPOCHS, lr=lr,
                                    shuffle_seed=shuffle)
      margin = min(margin, mg)
      score64, held_steps = None, 0
      if held:
        xh, yh = hc.stream([files[f] for f in held], BATCH, PRE, POST, PRE2, POST2, input_offset=offset)
        score64, mg = hc.evaluate(w64, xh, yh, BATCH)
        margin = min(margin, mg)
        held_steps = xh.shape[0] // BATCH
      runs.append((w64, hist64, score64, x64.shape[0] // BATCH, held_steps))
    if margin >= F64_MARGIN:
      return draw, files, runs, margin
  return None


def _count(mean_accuracy, entries):
  count = mean_accuracy * entries
  assert abs(count - round(count)) < 1e-6, count
  return int(round(count))


@pytest.mark.parametrize('offset,shuffle', [(-1, None), (0, None), (1, None), (0, SHUFFLE)])
def test_models_match_float64(offset, shuffle):
  from telluride_decoding_amd import brain_model
  case = float64_case(offset, shuffle)
  assert case is not None, 'no draw of %d keeps the three trajectories %g away from the kinks and the threshold' % (
      F64_DRAWS, F64_MARGIN)
  draw, files, runs, margin = case
  ds = _dataset(files, offset)
  models = _new_models(ds, [draw + mi for mi in range(3)], [dict(learning_rate=lr) for lr in F64_RATES])
  hists = brain_model.fit_many(models, ds, held_out=F64_HELD, epochs=F64_EPOCHS, shuffle_seeds=shuffle)
  scores = brain_model.evaluate_many(models, ds, files=F64_HELD)
  wdist = hdist = sdist = 0.0
  exact = []
  for m, hist, score, (w64, hist64, score64, steps, held_steps) in zip(models, hists, scores, runs):
    wmax = max(float(np.max(np.abs(b))) for b in w64)
    wdist = max(wdist, max(float(np.max(np.abs(a - b))) for a, b in zip(m.get_weights(), w64)) / wmax)
    got, want = np.asarray(hist.history['loss']), np.asarray(hist64['loss'])
    assert got.shape == (F64_EPOCHS,)
    hdist = max(hdist, float(np.max(np.abs(got - want) / np.abs(want))))
    entries = steps * BATCH * D
    exact.append(([_count(a, entries) for a in hist.history['accuracy']],
                  [_count(a, entries) for a in hist64['accuracy']]))
    if score64 is None:
      assert np.isnan(score['loss'])
      continue
    sdist = max(sdist, abs(score['loss'] - score64['loss']) / abs(score64['loss']))
    exact.append((_count(score['accuracy'], held_steps * BATCH * D),
                  _count(score64['accuracy'], held_steps * BATCH * D)))
  print('classifier_many float64: offset %d shuffle %s draw %d margin %.3g weights %.3g history %.3g scoring %.3g '
        'counts %s' % (offset, shuffle, draw, margin, wdist, hdist, sdist, exact))
  parity_log.record('classifier_many_float64', offset=offset, shuffle=str(shuffle), draw=draw, margin=margin,
                    weights=wdist, history=hdist, scoring=sdist)
  assert wdist <= 1e-4, wdist
  assert hdist <= 1e-5, hdist
  assert sdist <= 1e-5, sdist
  for got, want in exact:
    assert got == want, exact


# ---- 5. atomicity ----------------------------------------------------------------------------------------------
def test_a_bad_model_fails_the_whole_call():
  from telluride_decoding_amd import brain_model, device
  ds = _dataset(_files())
  models = _new_models(ds, SEEDS[:4], ADAM[:4])
  brain_model.fit_many(models, ds, held_out=HELD[:4], epochs=1)            # (so that there is a state to keep)
  before = [_snapshot(m) for m in models]
  assert [s[2] for s in before] == STEPS[:4]
  # the third model is left without a minibatch: fit_many's own guard
  with pytest.raises(ValueError, match='model 2 is left with'):
    brain_model.fit_many(models, ds, held_out=[[], [0], [0, 1, 2, 3, 4], [2]], epochs=2)
  # the third model's stream asks for more rows than its file has: the C entry point's check, nothing queued
  h = device.default_handle()
  x, x2, y, offs = ds.device_arrays(h)
  used = [brain_model.fold_rows_used(ds, held) for held in HELD[:4]]
  used[2][1] = LENGTHS[1] + 1
  opts = [m.optimizer for m in models]
  args = (x, x2, y, offs, PRE, POST, PRE2, POST2, HIDDEN, [m._device_params(h) for m in models])
  adam = ([o.learning_rate for o in opts], [o.beta_1 for o in opts], [o.beta_2 for o in opts],
          [o.epsilon for o in opts], [m._updates for m in models])
  with pytest.raises(ValueError, match='rows_used'):
    device.clf_train_many(*args, [m._state for m in models], BATCH, 2, used, *adam, handle=h)
  with pytest.raises(ValueError, match='rows_used'):                       # ... scoring checks the same
    device.clf_train_many(*args, None, BATCH, 1, used, update=False, handle=h)
  used[2][1] = 0
  with pytest.raises(ValueError, match='one pass'):                        # scoring is one epoch
    device.clf_train_many(*args, None, BATCH, 2, used, update=False, handle=h)
  # two models on one buffer
  with pytest.raises(ValueError, match='share'):
    brain_model.fit_many([models[0], models[1], models[0]], ds, epochs=1)
  h.synchronize()
  for i, (m, snap) in enumerate(zip(models, before)):
    _assert_same_bits(_snapshot(m), snap, 'model %d' % i)


# ---- 6. one model, and chunking ----------------------------------------------------------------------------
def test_one_model_is_fit():
  from telluride_decoding_amd import brain_model
  ds = _dataset(_files())
  for shuffle in (None, SHUFFLE):
    a, b = _new_models(ds, [5, 5], [ADAM[1], ADAM[1]])
    ha = brain_model.fit_many([a], ds, epochs=EPOCHS, shuffle_seeds=shuffle)[0].history
    hb = b.fit(ds, epochs=EPOCHS, shuffle_seed=shuffle).history
    _assert_same_bits(_snapshot(a), _snapshot(b), shuffle)
    assert ha == hb
    assert brain_model.evaluate_many([a], ds, files=[range(len(LENGTHS))]) == [b.evaluate(ds)]


def test_more_models_than_a_call_takes(monkeypatch):
  from telluride_decoding_amd import brain_model, device
  want, trained = _batched(SHUFFLE)
  scored = [[f] for f in (0, 1, 2, 3, 4, 0, 1)]
  want_scores = brain_model.evaluate_many(trained, _dataset(_files()), files=scored)
  monkeypatch.setattr(device, 'DNN_MANY_MAX_MODELS', 2)
  calls = []
  real = device._lib.load().td_clf_train_many
  monkeypatch.setattr(device.default_handle().lib, 'td_clf_train_many',
                      lambda *args: calls.append(args[NUM_MODELS_ARG]) or real(*args))
  got, models = _batched(SHUFFLE)
  assert calls == [2, 2, 2, 1]                                             # num_models of every call
  for i, ((snap_g, hist_g), (snap_w, hist_w)) in enumerate(zip(got, want)):
    _assert_same_bits(snap_g, snap_w, 'model %d' % i)
    assert hist_g == hist_w
  assert brain_model.evaluate_many(models, _dataset(_files()), files=scored) == want_scores
  assert calls == [2, 2, 2, 1] * 2


# ---- 7. the sweep ------------------------------------------------------------------------------------------
def test_jackknife_classifier():
  from telluride_decoding_amd import regression
  files = _files()
  ds = _dataset(files)
  rates = [1e-3, 3e-3]
  regression.LAST_SWEEP.pop('classifier_route', None)
  res = regression.jackknife_classifier(ds, HIDDEN, learning_rates=rates, epochs=EPOCHS, seed=4,
                                        shuffle_seed=SHUFFLE, _route='batched')
  assert list(res) == rates + ['all_runs', 'models', 'history']
  assert regression.LAST_SWEEP['classifier_route'] == 'batched'
  runs = res['all_runs']
  assert runs.shape == (2, len(files))
  for li, lr in enumerate(rates):
    for f in range(len(files)):
      train = _dataset(_without(files, [f]))
      m, = _new_models(train, [4], [dict(learning_rate=lr)])
      hist = m.fit(train, epochs=EPOCHS, shuffle_seed=SHUFFLE).history
      want = m.evaluate(_dataset([files[f]]))['accuracy']
      _assert_same_bits(_snapshot(res['models'][li][f]), _snapshot(m), (lr, f))
      assert res['history'][li][f] == hist
      if np.isnan(want):                  # (the 5-frame recording is no minibatch of its own: Keras' empty mean)
        assert f == 5 and np.isnan(runs[li, f])
        continue
      assert runs[li, f] == want, (lr, f, runs[li, f], want)
    assert np.all((runs[li, :5] >= 0.0) & (runs[li, :5] <= 1.0))
  assert all(len(res[lr]) == 2 for lr in rates)
  # folds=: the two routes, on the other metric
  a = regression.jackknife_classifier(ds, HIDDEN, learning_rates=rates, epochs=EPOCHS, seed=4, folds=[4, 1],
                                      test_metric='loss', _route='per_fold')
  assert regression.LAST_SWEEP['classifier_route'] == 'per_fold'
  b = regression.jackknife_classifier(ds, HIDDEN, learning_rates=rates, epochs=EPOCHS, seed=4, folds=[4, 1],
                                      test_metric='loss', _route='batched')
  assert regression.LAST_SWEEP['classifier_route'] == 'batched'
  assert a['all_runs'].shape == (2, 2) and np.all(np.isfinite(a['all_runs']))
  np.testing.assert_array_equal(a['all_runs'], b['all_runs'])
  assert a['history'] == b['history']
  for lr in rates:
    assert a[lr] == b[lr] and np.isfinite(a[lr][0])
    assert a[lr][0] == pytest.approx(float(np.mean(a['all_runs'][rates.index(lr)])), rel=1e-12)
  for row_a, row_b in zip(a['models'], b['models']):
    for ma, mb in zip(row_a, row_b):
      _assert_same_bits(_snapshot(ma), _snapshot(mb), 'routes')
  # the default route is one of the two and is recorded
  regression.jackknife_classifier(ds, HIDDEN, folds=[0], epochs=1)
  assert regression.LAST_SWEEP['classifier_route'] == regression.CLASSIFIER_ROUTE
