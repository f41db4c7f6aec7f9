"""brain_model.fit_many and regression.jackknife_dnn on the MI355X.  The yardsticks are the
single-fit path, BrainModelDNN.fit on a Dataset of the fold's files -- pinned to float64 by tests/test_gpu_dnn.py and
tests/test_gpu_dnn_pearson.py -- which a batched model must equal bit for bit, and the float64 restatements of
tests/host_dnn.py / tests/host_dnn_pearson.py themselves, with test_gpu_dnn.py's bounds.

One recipe throughout: 3 channels, pre 2 / post 2 (K = 15: W1 slices of 4, 4, 4 and 3 rows), hidden [8, 4], 2 outputs,
minibatches of 32, six recordings of 101, 130, 95, 64, 37 and 5 frames, 3 epochs; seven models: every recording, then
each of the six held out (9 .. 13 steps an epoch, so most models idle through the last rounds of a call; the folds'
streams lose the whole last recording and part of the one before it)."""
import functools

import numpy as np
import pytest

from tests import host_dnn
from tests import host_dnn_pearson
from tests import parity_log
from tests.dnn_common import make_files

pytestmark = pytest.mark.gpu

C, PRE, POST, D, BATCH, HIDDEN, EPOCHS = 3, 2, 2, 2, 32, [8, 4], 3
LENGTHS = [101, 130, 95, 64, 37, 5]
WIDTHS = [C * (PRE + 1 + POST)] + HIDDEN + [D]
HELD = [[]] + [[f] for f in range(len(LENGTHS))]        # model 0: nothing held out; model f + 1: recording f
SHUFFLE = 12345


def _dataset(files, offset=0):
  from telluride_decoding_amd import brain_data
  return brain_data.Dataset(files, BATCH, PRE, POST, input_offset=offset)


def _without(files, held):
  return [f for i, f in enumerate(files) if i not in held]


def _snapshot(model):
  """(weights, RMSprop state) of a model as host arrays."""
  state = None if model._state is None else model._state.cpu().numpy().copy()
  return [w.copy() for w in model.get_weights()], state


def _assert_same_bits(got, want, what):
  for a, b in zip(got[0], want[0]):
    np.testing.assert_array_equal(a, b, err_msg='weights of %s' % (what,))
  np.testing.assert_array_equal(got[1], want[1], err_msg='state of %s' % (what,))


def _new_models(ds, loss, seeds, rates):
  from telluride_decoding_amd import brain_model
  models = []
  for seed, lr in zip(seeds, rates):
    m = brain_model.BrainModelDNN(ds, HIDDEN, seed=seed)
    m.compile(optimizer=brain_model.RMSprop(learning_rate=lr), loss=loss)
    models.append(m)
  return models


SEEDS = [11, 12, 13, 14, 15, 16, 17]
RATES = [1e-3, 3e-3, 1e-3, 3e-3, 1e-3, 3e-3, 1e-3]


@functools.lru_cache(maxsize=None)
def _files():
  return make_files(np.random.default_rng(69), LENGTHS, C, D)


@functools.lru_cache(maxsize=None)
def _sequential(loss, shuffle):
  """The yardstick: every model by its own BrainModelDNN.fit on a Dataset of the recordings it trains on."""
  out = []
  for held, seed, lr in zip(HELD, SEEDS, RATES):
    ds = _dataset(_without(_files(), held))
    m, = _new_models(ds, loss, [seed], [lr])
    hist = m.fit(ds, epochs=EPOCHS, shuffle_seed=shuffle).history
    out.append((_snapshot(m), hist))
  return out


def _batched(loss, shuffle):
  from telluride_decoding_amd import brain_model
  ds = _dataset(_files())
  models = _new_models(ds, loss, SEEDS, RATES)
  hists = brain_model.fit_many(models, ds, held_out=HELD, epochs=EPOCHS, shuffle_seeds=shuffle)
  return [(_snapshot(m), h.history) for m, h in zip(models, hists)]


# ---- 1. bit for bit the single fit -------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['mse', 'pearson'])
@pytest.mark.parametrize('shuffle', [None, SHUFFLE], ids=['in_order', 'shuffled'])
def test_every_model_equals_its_own_fit(loss, shuffle):
  want = _sequential(loss, shuffle)
  got = _batched(loss, shuffle)
  steps = [13, 10, 9, 10, 11, 12, 13]
  for i, ((snap_g, hist_g), (snap_w, hist_w)) in enumerate(zip(got, want)):
    _assert_same_bits(snap_g, snap_w, (loss, shuffle, 'model %d' % i))
    assert hist_g == hist_w, (loss, shuffle, i)
    assert all(len(v) == EPOCHS and np.all(np.isfinite(v)) for v in hist_g.values())
  from telluride_decoding_amd import brain_model
  assert [sum(brain_model.fold_rows_used(_dataset(_files()), h)) // BATCH for h in HELD] == steps
  # the models did train, and apart from each other
  assert not np.array_equal(got[0][0][0][0], host_dnn.glorot(WIDTHS, SEEDS[0])[0])
  assert not np.array_equal(got[1][0][0][0], got[3][0][0][0])


# ---- 2. the float64 restatement ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float64(loss, offset, shuffle, max_draws=8):
  """(draw, files, per model (w64, hist64), kink) of the first draw whose seven float64 trajectories all stay 1e-5
  away from the ReLU kinks (the redraw rule of tests/test_gpu_dnn.py's _trajectory)."""
  train = host_dnn_pearson.train if loss == 'pearson' else host_dnn.train
  for draw in range(max_draws):
    files = make_files(np.random.default_rng(70 + draw), LENGTHS, C, D)
    runs, kink = [], np.inf
    for mi, held in enumerate(HELD):
      x64, y64 = host_dnn.stream(_without(files, held), BATCH, PRE, POST, input_offset=offset)
      w64, _, hist64, k = train(host_dnn.glorot(WIDTHS, draw + mi), x64, y64, BATCH, EPOCHS, 1e-3,
                                shuffle_seed=shuffle)
      runs.append((w64, hist64))
      kink = min(kink, k)
    if kink >= 1e-5:
      return draw, files, runs, kink
  pytest.fail('no draw of %d keeps the seven trajectories away from the ReLU kinks' % max_draws)


@pytest.mark.parametrize('loss,offset,shuffle', [('mse', -1, None), ('mse', 0, None), ('mse', 1, None),
                                                 ('mse', 0, SHUFFLE), ('pearson', 0, None), ('pearson', 0, SHUFFLE)])
def test_models_match_float64(loss, offset, shuffle):
  from telluride_decoding_amd import brain_model
  draw, files, runs, kink = _float64(loss, offset, shuffle)
  ds = _dataset(files, offset)
  models = _new_models(ds, loss, [draw + mi for mi in range(len(HELD))], [1e-3] * len(HELD))
  hists = brain_model.fit_many(models, ds, held_out=HELD, epochs=EPOCHS, shuffle_seeds=shuffle)
  wdist = hdist = lrel = 0.0
  for m, hist, (w64, hist64) in zip(models, hists, runs):
    wmax = max(float(np.max(np.abs(b))) for b in w64)
    wdist = max(wdist, max(float(np.max(np.abs(a - b))) for a, b in zip(m.get_weights(), w64)) / wmax)
    for key in ('loss', 'pearson_correlation_first', 'mse'):
      got, want = np.asarray(hist.history[key]), np.asarray(hist64[key])
      assert got.shape == (EPOCHS,)
      # (a correlation's scale is 1: near r = 0 its relative error is not meaningful.  The Pearson loss is
      # -(1 / B) x a sum of correlations -- 1e-4 at these untrained weights -- and is held to the rule
      # tests/test_gpu_dnn_pearson.py holds it to: B |dL| <= 1e-5, absolute on the sum of correlations; its
      # relative distance is recorded)
      if key == 'pearson_correlation_first':
        scale = np.maximum(np.abs(want), 1.0)
      elif key == 'loss' and loss == 'pearson':
        scale = 1.0 / BATCH
        lrel = max(lrel, float(np.max(np.abs(got - want) / np.abs(want))))
      else:
        scale = np.abs(want)
      hdist = max(hdist, float(np.max(np.abs(got - want) / scale)))
  print('dnn_many float64: loss %s offset %d shuffle %s draw %d kink %.3g weights %.3g history %.3g '
        '(Pearson loss, relative: %.3g)' % (loss, offset, shuffle, draw, kink, wdist, hdist, lrel))
  parity_log.record('dnn_many_float64', loss=loss, offset=offset, shuffle=str(shuffle), draw=draw, kink=kink,
                    weights=wdist, history=hdist, pearson_loss_rel=lrel)
  assert wdist <= 1e-4, wdist
  assert hdist <= 1e-5, hdist


# ---- 3. continuation and atomicity -------------------------------------------------------------------------
def test_two_calls_continue_as_one():
  from telluride_decoding_amd import brain_model
  ds = _dataset(_files())
  once = _new_models(ds, 'mse', SEEDS, RATES)
  twice = _new_models(ds, 'mse', SEEDS, RATES)
  h4 = brain_model.fit_many(once, ds, held_out=HELD, epochs=4)
  h2a = brain_model.fit_many(twice, ds, held_out=HELD, epochs=2)
  h2b = brain_model.fit_many(twice, ds, held_out=HELD, epochs=2)
  for i, (a, b) in enumerate(zip(twice, once)):
    _assert_same_bits(_snapshot(a), _snapshot(b), 'model %d' % i)
    for key in ('loss', 'pearson_correlation_first', 'mse'):
      assert h2a[i].history[key] + h2b[i].history[key] == h4[i].history[key]


def test_a_bad_model_fails_the_whole_call():
  from telluride_decoding_amd import brain_model, device
  ds = _dataset(_files())
  models = _new_models(ds, 'mse', SEEDS[:4], RATES[:4])
  brain_model.fit_many(models, ds, held_out=HELD[:4], epochs=1)            # (so that there is a state to keep)
  before = [_snapshot(m) for m in models]
  # the third model is left without a minibatch: fit_many's own guard
  with pytest.raises(ValueError, match='model 2 is left with'):
    brain_model.fit_many(models, ds, held_out=[[], [0], [0, 1, 2, 3, 4], [2]], epochs=2)
  # the third model's stream asks for more rows than its file has: the C entry point's check, nothing queued
  h = device.default_handle()
  x, _, y, offs = ds.device_arrays(h)
  used = [brain_model.fold_rows_used(ds, held) for held in HELD[:4]]
  used[2][1] = LENGTHS[1] + 1
  opt = models[0].optimizer
  with pytest.raises(ValueError, match='rows_used'):
    device.dnn_train_many(x, y, offs, PRE, POST, HIDDEN, [m._device_params(h) for m in models],
                          [m._state for m in models], BATCH, 2, [opt.learning_rate] * 4, [opt.rho] * 4,
                          [opt.epsilon] * 4, used, handle=h)
  # two models on one buffer
  with pytest.raises(ValueError, match='share'):
    brain_model.fit_many([models[0], models[1], models[0]], ds, epochs=1)
  for i, (m, snap) in enumerate(zip(models, before)):
    _assert_same_bits(_snapshot(m), snap, 'model %d' % i)


# ---- 4. one model, and chunking ----------------------------------------------------------------------------
def test_one_model_is_fit():
  from telluride_decoding_amd import brain_model
  ds = _dataset(_files())
  for loss, shuffle in (('mse', None), ('pearson', SHUFFLE)):
    a, b = _new_models(ds, loss, [5, 5], [2e-3, 2e-3])
    ha = brain_model.fit_many([a], ds, epochs=EPOCHS, shuffle_seeds=shuffle)[0].history
    hb = b.fit(ds, epochs=EPOCHS, shuffle_seed=shuffle).history
    _assert_same_bits(_snapshot(a), _snapshot(b), (loss, shuffle))
    assert ha == hb


def test_more_models_than_a_call_takes(monkeypatch):
  from telluride_decoding_amd import device
  want = _batched('mse', SHUFFLE)
  monkeypatch.setattr(device, 'DNN_MANY_MAX_MODELS', 2)
  calls = []
  real = device._lib.load().td_dnn_train_many
  monkeypatch.setattr(device.default_handle().lib, 'td_dnn_train_many',
                      lambda *args: calls.append(args[17]) or real(*args))
  got = _batched('mse', SHUFFLE)
  assert calls == [2, 2, 2, 1]                                             # num_models of every call
  for i, ((snap_g, hist_g), (snap_w, hist_w)) in enumerate(zip(got, want)):
    _assert_same_bits(snap_g, snap_w, 'model %d' % i)
    assert hist_g == hist_w


# ---- 5. the sweep ------------------------------------------------------------------------------------------
def test_jackknife_dnn():
  from telluride_decoding_amd import brain_model, regression
  files = _files()
  ds = _dataset(files)
  rates = [1e-3, 3e-3]
  regression.LAST_SWEEP.pop('dnn_route', None)
  res = regression.jackknife_dnn(ds, HIDDEN, learning_rates=rates, epochs=EPOCHS, seed=4, shuffle_seed=SHUFFLE,
                                 _route='batched')
  assert list(res) == rates + ['all_runs', 'models', 'history']
  assert regression.LAST_SWEEP['dnn_route'] == 'batched'
  runs = res['all_runs']
  assert runs.shape == (2, len(files))
  dist = 0.0
  for li, lr in enumerate(rates):
    for f in range(len(files)):
      train = _dataset(_without(files, [f]))
      m, = _new_models(train, 'mse', [4], [lr])
      hist = m.fit(train, epochs=EPOCHS, shuffle_seed=SHUFFLE).history
      want = m.evaluate(_dataset([files[f]]))['pearson_correlation_first']
      _assert_same_bits(_snapshot(res['models'][li][f]), _snapshot(m), (lr, f))
      assert res['history'][li][f] == hist
      if np.isnan(want):                  # (the 5-frame recording is no minibatch of its own: Keras' empty mean)
        assert f == 5 and np.isnan(runs[li, f])
        continue
      dist = max(dist, abs(runs[li, f] - want))
      # the same weights through the same forward and window-sums kernels: the same number
      assert runs[li, f] == want, (lr, f, runs[li, f], want)
    five = runs[li, :5]
    assert np.all(np.abs(five) <= 1.0)
  parity_log.record('dnn_many_sweep', held_out_r=dist)
  # (a recording without a minibatch makes the mean over all folds NaN, as it does for the other sweeps)
  assert all(len(res[lr]) == 2 for lr in rates)
  # folds=: the two routes
  a = regression.jackknife_dnn(ds, HIDDEN, learning_rates=rates, epochs=EPOCHS, seed=4, folds=[4, 1],
                               _route='per_fold')
  assert regression.LAST_SWEEP['dnn_route'] == 'per_fold'
  b = regression.jackknife_dnn(ds, HIDDEN, learning_rates=rates, epochs=EPOCHS, seed=4, folds=[1, 4],
                               _route='batched')
  assert regression.LAST_SWEEP['dnn_route'] == 'batched'
  assert a['all_runs'].shape == (2, 2)
  np.testing.assert_array_equal(a['all_runs'], b['all_runs'])
  assert a['history'] == b['history']
  for lr in rates:
    assert a[lr] == b[lr] and np.isfinite(a[lr][0])
    assert a[lr][0] == pytest.approx(float(np.mean(a['all_runs'][rates.index(lr)])), rel=1e-12)
  for row_a, row_b in zip(a['models'], b['models']):
    for ma, mb in zip(row_a, row_b):
      _assert_same_bits(_snapshot(ma), _snapshot(mb), 'routes')
  # the default route is one of the two and is recorded
  regression.jackknife_dnn(ds, HIDDEN, folds=[0], epochs=1)
  assert regression.LAST_SWEEP['dnn_route'] == regression.DNN_ROUTE
