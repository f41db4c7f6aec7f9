"""The kernels of csrc/mlp.hip on the MI355X at their tile edges (the cases of tests/dnn_edges.py, which
tests/test_cpu_dnn_edges.py shows to reach them): first-layer widths between and at the slab kernel's tile widths,
batches that leave the last 64-row chunk and the last head workgroup partly filled, W1 slices whose last one is short,
and training at shapes with several head workgroups, row chunks and slices, where the update refreshes a tile with dead
columns.  The references, the redraw rules, the assertions and the bounds are those of tests/test_gpu_dnn.py,
tests/test_gpu_dnn_pearson.py, tests/test_gpu_classifier.py and the two *_many suites at their own shapes; the observed
distances are in DESIGN section 14."""
import numpy as np
import pytest

from tests import dnn_edges as de
from tests import host_dnn
from tests import host_dnn_pearson
from tests import parity_log
from tests.dnn_common import GRAD_BOUND, assert_within, flat, grad_distances, make_files, split, tensor_names
from tests.test_gpu_classifier import LOSS_BOUND, _counts, _run_grad
from tests.test_gpu_dnn_pearson import _r_of_sums

pytestmark = pytest.mark.gpu


# ---- 1. gradients against float64 -----------------------------------------------------------------------------------
def _device_grad(case, shape, loss):
  from telluride_decoding_amd import device
  hidden, c, pre, post, batch, d, off = shape
  h = device.default_handle()
  res = case['ds'].resolved()
  x, _, y, offs = res.device_arrays(h)
  params = h.to_device(flat(case['weights']))
  extra = dict(loss='pearson') if loss == 'pearson' else {}
  grad, sums = device.mlp_grad(x, y, offs, pre, post, hidden, params, batch, case['s'], input_offset=off,
                               rows_used=res.rows_used(), handle=h, **extra)
  return split(grad.cpu().numpy(), case['widths']), sums.cpu().numpy()


@pytest.mark.parametrize('shape', de.MSE_GRID, ids=de.regressor_id)
def test_mse_gradients_match_float64(shape):
  case = de.regressor_grad_case('mse', *shape)
  if case is None:
    pytest.fail('no seed keeps the ReLU inputs away from their kinks')
  batch, d = shape[4], shape[5]
  got, s6 = _device_grad(case, shape, 'mse')
  dists = grad_distances(got, case['g64'])
  loss_rel = abs(s6[5] / (batch * d) - case['loss']) / case['loss']
  print('dnn edge grad %s: per tensor %s, loss rel %.3g, kink %.3g' % (shape, dists, loss_rel, case['kink']))
  parity_log.record('dnn_edge_grad', shape=str(shape), rel=max(dists.values()), loss_rel=loss_rel, kink=case['kink'])
  assert s6.shape == (6,) and all(np.all(np.isfinite(g)) for g in got)
  assert_within(dists, GRAD_BOUND)
  assert abs(s6[5] / (batch * d) - case['loss']) <= 1e-6 * case['loss']


@pytest.mark.parametrize('shape', de.PEARSON_GRID, ids=de.regressor_id)
def test_pearson_gradients_match_float64(shape):
  case = de.regressor_grad_case('pearson', *shape)
  if case is None:
    pytest.fail('no seed keeps the ReLU inputs away from their kinks')
  batch, d = shape[4], shape[5]
  assert case['widths'][-2] >= 2
  got, s7 = _device_grad(case, shape, 'pearson')
  g64, p64, y64 = case['g64'], case['p64'], case['y64']
  assert s7.shape == (7,)
  dists = grad_distances(got, g64[:-1])
  loss_dist = abs(batch * s7[6] - batch * case['loss'])
  mse64 = float(np.mean((p64 - y64) ** 2))
  mse_dist = abs(s7[5] / (batch * d) - mse64) / mse64
  r_dist = abs(_r_of_sums(s7, batch) - host_dnn.pearson_first(p64, y64))
  print('pearson edge grad %s: per tensor %s, B |dL| %.3g, mse rel %.3g, r abs %.3g, kink %.3g' % (
      shape, dists, loss_dist, mse_dist, r_dist, case['kink']))
  parity_log.record('dnn_pearson_edge_grad', shape=str(shape), rel=max(dists.values()), loss_times_b=loss_dist,
                    mse_rel=mse_dist, r_abs=r_dist, kink=case['kink'])
  assert all(np.all(np.isfinite(g)) for g in got) and np.all(np.isfinite(s7))
  assert_within(dists, GRAD_BOUND)
  assert np.all(got[-1] == 0.0), got[-1]                       # the output bias: exactly zero
  assert np.all(g64[-1] == 0.0)
  assert loss_dist <= 1e-5 * d, loss_dist
  assert mse_dist <= 1e-6, mse_dist
  assert r_dist <= 1e-5, r_dist


@pytest.mark.parametrize('shape', de.CLASSIFIER_GRID, ids=de.classifier_id)
def test_classifier_gradients_match_float64(shape):
  case = de.classifier_grad_case(*shape)
  worst, loss_rel = _run_grad(case, shape[0], shape[7], shape[8], shape[9])    # (bound, finite loss, exact count)
  parity_log.record('classifier_edge_grad', shape=str(shape), rel=worst, loss_rel=loss_rel, margin=case['margin'],
                    draws=case['draws'])
  assert loss_rel <= LOSS_BOUND


# ---- 2. training trajectories -----------------------------------------------------------------------------------------
def _weights_distance(got, w64):
  wmax = max(float(np.max(np.abs(b))) for b in w64)
  return {n: float(np.max(np.abs(a - b))) / wmax for n, a, b in zip(tensor_names(len(w64)), got, w64)}


def _regressor_fits(case, shuffle, losses):
  """One fit per entry of `losses` from the case's weights: [(model, history)], asserted bitwise equal."""
  from telluride_decoding_amd import brain_model
  t = case['t']
  ds = de.dataset_of(t, case['files'])
  runs = []
  for loss in losses:
    m = brain_model.BrainModelDNN(ds, t['hidden'], seed=case['seed'])
    m.compile(**({} if loss is None else dict(loss=loss)))
    runs.append((m, m.fit(ds, epochs=t['epochs'], shuffle_seed=shuffle).history))
  for a, b in zip(runs[0][0].get_weights(), runs[1][0].get_weights()):
    np.testing.assert_array_equal(a, b)                      # bitwise reproducible
  assert runs[0][1] == runs[1][1]
  return ds, runs


@pytest.mark.parametrize('shuffle', [None, de.SHUFFLE], ids=['in_order', 'shuffled'])
@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_mse_trajectory(name, shuffle):
  case = de.regressor_trajectory_case('mse', name, shuffle)
  if case is None:
    pytest.fail('no seed keeps the trajectory away from the ReLU kinks')
  t, w64, hist64 = case['t'], case['w64'], case['hist64']
  _, runs = _regressor_fits(case, shuffle, [None, None])
  per_tensor = _weights_distance(runs[0][0].get_weights(), w64)
  wdist = max(per_tensor.values())
  hdist = 0.0
  for key in ('loss', 'pearson_correlation_first', 'mse'):
    got, want = np.asarray(runs[0][1][key]), np.asarray(hist64[key])
    assert got.shape == (t['epochs'],)
    scale = np.maximum(np.abs(want), 1.0) if key == 'pearson_correlation_first' else np.abs(want)
    hdist = max(hdist, float(np.max(np.abs(got - want) / scale)))
  print('dnn edge trajectory %s (shuffle %s): weights %s, history %.3g, kink %.3g' % (name, shuffle, per_tensor,
                                                                                       hdist, case['kink']))
  parity_log.record('dnn_edge_trajectory', shape=name, shuffle=str(shuffle), weights=wdist, history=hdist,
                    kink=case['kink'], draws=case['draws'])
  assert not np.array_equal(runs[0][0].get_weights()[0], host_dnn.glorot(de.widths_of(t), case['seed'])[0])
  assert wdist <= 1e-4, per_tensor
  assert hdist <= 1e-5, hdist


@pytest.mark.parametrize('shuffle', [None, de.SHUFFLE], ids=['in_order', 'shuffled'])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_pearson_trajectory(name, shuffle):
  from telluride_decoding_amd import brain_model
  case = de.regressor_trajectory_case('pearson', name, shuffle)
  if case is None:
    pytest.fail('no seed keeps the trajectory away from the ReLU kinks')
  t, w64, hist64 = case['t'], case['w64'], case['hist64']
  batch = t['batch']
  ds, runs = _regressor_fits(case, shuffle, [brain_model.PearsonCorrelationLoss(), 'pearson'])
  m, hist = runs[0]
  per_tensor = _weights_distance(m.get_weights(), w64)
  wdist = max(per_tensor.values())
  for key in ('loss', 'pearson_correlation_first', 'mse'):
    assert np.asarray(hist[key]).shape == (t['epochs'],)
  ldist = float(np.max(np.abs(np.asarray(hist['loss']) - np.asarray(hist64['loss'])))) * batch
  rdist = float(np.max(np.abs(np.asarray(hist['pearson_correlation_first']) -
                              np.asarray(hist64['pearson_correlation_first']))))
  mdist = float(np.max(np.abs(np.asarray(hist['mse']) - np.asarray(hist64['mse'])) / np.asarray(hist64['mse'])))
  # evaluate at the trained weights: the float64 per-minibatch means of the restatement
  w = m.get_weights()
  losses, rs, mses = [], [], []
  batches = list(ds)
  assert len(batches) == case['steps']
  for feats, y in batches:
    p = host_dnn.forward(w, np.asarray(feats['input_1'], np.float64))[0]
    y = np.asarray(y, np.float64)
    losses.append(host_dnn_pearson.loss_and_dz(p, y)[0])
    rs.append(host_dnn.pearson_first(p, y))
    mses.append(np.mean((p - y) ** 2))
  ev, ev_it = m.evaluate(ds), m.evaluate(batches)
  edist = max(abs(e['loss'] - np.mean(losses)) * batch for e in (ev, ev_it))
  print('pearson edge trajectory %s (shuffle %s): weights %s, B |dL| %.3g, r %.3g, mse rel %.3g, evaluate B |dL| %.3g, '
        'kink %.3g' % (name, shuffle, per_tensor, ldist, rdist, mdist, edist, case['kink']))
  parity_log.record('dnn_pearson_edge_trajectory', shape=name, shuffle=str(shuffle), weights=wdist, loss_times_b=ldist,
                    r_abs=rdist, mse_rel=mdist, evaluate_loss_times_b=edist, kink=case['kink'], draws=case['draws'])
  assert wdist <= 1e-4, per_tensor
  assert ldist <= 1e-5, ldist
  assert rdist <= 1e-5, rdist
  assert mdist <= 1e-5, mdist
  assert edist <= 1e-5, edist
  for e in (ev, ev_it):
    assert sorted(e) == ['loss', 'mse', 'pearson_correlation_first']
    assert abs(e['mse'] - np.mean(mses)) <= 1e-5 * np.mean(mses)
    assert abs(e['pearson_correlation_first'] - np.mean(rs)) <= 1e-5
  # the history's loss is the correlation loss, not the mse, and the net was trained on it (as in float64)
  assert all(v < 0.0 for v in hist64['loss'][1:]) and hist64['loss'][-1] < hist64['loss'][0]
  assert all(v < 0.0 for v in hist['loss'][1:]) and all(v > 0.0 for v in hist['mse'])
  assert hist['loss'][-1] < hist['loss'][0]
  np.testing.assert_array_equal(w[-1], 0.0)                  # the output bias never moves on this loss


@pytest.mark.parametrize('shuffle', [None, de.SHUFFLE], ids=['in_order', 'shuffled'])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_classifier_trajectory(name, shuffle):
  from telluride_decoding_amd import brain_model
  case = de.classifier_trajectory_case(name, shuffle)
  if case is None:
    pytest.fail('no draw keeps the trajectory away from the kinks and the threshold')
  t, w64, want = case['t'], case['w64'], case['hist64']
  ds = de.dataset_of(t, case['files'])
  runs = []
  for _ in range(2):
    m = brain_model.BrainModelClassifier(ds, t['hidden'], seed=case['seed'])
    m.compile()
    hist = m.fit(ds, epochs=t['epochs'], shuffle_seed=shuffle).history
    runs.append((m.get_weights(), hist))
  for a, b in zip(runs[0][0], runs[1][0]):
    np.testing.assert_array_equal(a, b)                      # two identical fits: bitwise
  assert runs[0][1] == runs[1][1]
  per_tensor = _weights_distance(runs[0][0], w64)
  got = runs[0][1]
  assert sorted(got) == ['accuracy', 'loss'] and len(got['loss']) == t['epochs']
  hdist = float(np.max(np.abs(np.asarray(got['loss']) - want['loss']) / np.abs(want['loss'])))
  print('classifier edge trajectory', name, shuffle, per_tensor, 'loss rel', hdist, 'margin', case['margin'])
  wdist = max(per_tensor.values())
  parity_log.record('classifier_edge_trajectory', shape=name, shuffle=str(shuffle), weights=wdist, history=hdist,
                    margin=case['margin'], draws=case['draws'])
  assert wdist <= 1e-4, per_tensor
  assert hdist <= 1e-5, hdist
  entries = case['steps'] * t['batch'] * t['d']            # the history's accuracy as a count: exact
  assert _counts(got['accuracy'], entries) == _counts(want['accuracy'], entries)


# ---- 3. the many-model kernels and the forward ---------------------------------------------------------------------
def _snapshot(model):
  """(weights, optimizer state, a classifier's count of updates) of a model as host values."""
  state = None if model._state is None else model._state.cpu().numpy().copy()
  return [w.copy() for w in model.get_weights()], state, getattr(model, '_updates', None)


def _assert_same_bits(got, want, what):
  for a, b in zip(got[0], want[0]):
    np.testing.assert_array_equal(a, b, err_msg='weights of %s' % (what,))
  np.testing.assert_array_equal(got[1], want[1], err_msg='optimizer state of %s' % (what,))
  assert got[2] == want[2], ('_updates of %s' % (what,), got[2], want[2])


def _every_model_equals_its_own_fit(t, files, held_out, new_model):
  """fit_many over the folds of `held_out` against each model's own fit on a Dataset of the recordings it trains on."""
  from telluride_decoding_amd import brain_model
  ds = de.dataset_of(t, files)
  models = [new_model(ds, i) for i in range(len(held_out))]
  hists = brain_model.fit_many(models, ds, held_out=held_out, epochs=de.MANY_EPOCHS, shuffle_seeds=de.SHUFFLE)
  for i, held in enumerate(held_out):
    fold = de.dataset_of(t, [f for fi, f in enumerate(files) if fi not in held])
    steps = sum(brain_model.fold_rows_used(ds, held)) // t['batch']
    assert steps == fold.num_batches() and steps >= 2
    alone = new_model(fold, i)
    start = [w.copy() for w in alone.get_weights()]
    hist = alone.fit(fold, epochs=de.MANY_EPOCHS, shuffle_seed=de.SHUFFLE).history
    _assert_same_bits(_snapshot(models[i]), _snapshot(alone), 'model %d' % i)
    assert hists[i].history == hist, i
    assert all(len(v) == de.MANY_EPOCHS and np.all(np.isfinite(v)) for v in hist.values())
    assert not np.array_equal(alone.get_weights()[0], start[0])          # (it did train)
  assert not np.array_equal(models[0].get_weights()[0], models[1].get_weights()[0])


@pytest.mark.parametrize('loss', ['mse', 'pearson'])
def test_every_regressor_of_a_batched_fit_equals_its_own_fit(loss):
  """td_dnn_train_many at shape A: mlp_slab_many_kernel<16> with three dead columns, two head workgroups a model."""
  from telluride_decoding_amd import brain_model
  t = de.TRAJ_A
  files = make_files(np.random.default_rng(71), t['lengths'], t['c'], t['d'])

  def new_model(ds, i):
    m = brain_model.BrainModelDNN(ds, t['hidden'], seed=de.MANY_SEEDS[i])
    m.compile(optimizer=brain_model.RMSprop(learning_rate=de.MANY_RATES[i]), loss=loss)
    return m
  _every_model_equals_its_own_fit(t, files, de.MANY_HELD_A, new_model)


def test_every_classifier_of_a_batched_fit_equals_its_own_fit():
  """td_clf_train_many at the classifier's shape B: mlp_slab_many_kernel<32>, three head workgroups a model."""
  from telluride_decoding_amd import brain_model
  t = de.TRAJ_CB
  files = make_files(np.random.default_rng(171), t['lengths'], t['c'], t['d'], c2=t['c2'])

  def new_model(ds, i):
    m = brain_model.BrainModelClassifier(ds, t['hidden'], seed=de.MANY_SEEDS[i])
    m.compile(optimizer=brain_model.Adam(learning_rate=de.MANY_RATES[i]))
    return m
  _every_model_equals_its_own_fit(t, files, de.MANY_HELD_CB, new_model)


def test_inference_across_the_forward_chunks_matches_float64():
  from oracle import lag as o_lag
  from telluride_decoding_amd import brain_data, brain_model
  t = de.PREDICT
  rng = np.random.default_rng(7)
  files = make_files(rng, t['lengths'], t['c'], t['d'])
  ds = brain_data.Dataset(files, t['batch'], t['pre'], t['post'], input_offset=t['offset'])
  m = brain_model.BrainModelDNN(ds, t['hidden'], seed=1)
  w = m.get_weights()
  pred = m.predict(ds)
  want = np.concatenate([host_dnn.forward(w, o_lag.window_streams(*f, pre=t['pre'], post=t['post'],
                                                                  input_offset=t['offset'])[0])[0] for f in files])
  want = brain_model.rows_of_stream(want, ds.zipped_lengths(), ds.rows_used())
  assert pred.shape == want.shape and pred.shape[0] > 2 * 4096
  dist = float(np.max(np.abs(pred - want)) / np.max(np.abs(want)))
  print('dnn edge forward: %.3g' % dist)
  parity_log.record('dnn_edge_forward', rel=dist)
  assert dist <= 1e-5, dist
