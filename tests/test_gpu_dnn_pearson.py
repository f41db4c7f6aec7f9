"""BrainModelDNN trained on the Pearson correlation loss, on the MI355X against the float64 restatement of
tests/host_dnn_pearson.py: the gradients of td_mlp_grad_loss over shapes that stress the
head, short training trajectories, the invariance to the target's scale, the zero rule, the unchanged mse
path, the reference's data recipes trained on the new loss, and the limits."""
import numpy as np
import pytest

from tests import host_dnn
from tests import host_dnn_pearson
from tests import parity_log
from tests.dnn_common import (GRAD_BOUND, KINK, assert_within, flat, grad_distances, iir, make_files, simply_scaled,
                              split)

pytestmark = pytest.mark.gpu

# (hidden, channels, pre, post, batch, outputs, input_offset).  The loss changes only the head: one partial
# workgroup; a partial second workgroup (its invalid rows must stay out of the moments); 32 partials; the
# rest as the mse grid's.  The output layer's fan-in is >= 2 everywhere (a single output weight has an
# identically zero gradient, like the output bias).
GRID = [
    ([], 2, 0, 1, 32, 1, 0),
    ([], 4, 1, 1, 100, 8, 1),
    ([20, 20], 2, 0, 2, 2048, 8, 0),
    ([20, 20], 64, 15, 21, 128, 1, -1),
    ([40, 20, 10], 2, 1, 1, 1000, 2, 0),
    ([64] * 4, 4, 1, 2, 128, 8, 0),
]


def _grad_case(hidden, c, pre, post, batch, d, off, mixup=False):
  from telluride_decoding_amd import brain_data, device
  h = device.default_handle()
  k = c * (pre + 1 + post)
  widths = [k] + hidden + [d]
  assert widths[-2] >= 2
  for seed in range(8):
    rng = np.random.default_rng(1000 + seed)
    lengths = [int(batch * f) + 7 for f in (0.6, 1.3, 0.45, 1.9)]          # ragged files
    files = make_files(rng, lengths, c, d)
    ds = brain_data.Dataset(files, batch, pre, post, input_offset=off, mixup_batch=mixup, mixup_seed=seed)
    batches = list(ds)
    # the minibatch that straddles the first file boundary
    first = max(lengths[0] - abs(off), 0)
    s = min(first // batch, len(batches) - 1)
    weights = host_dnn.glorot(widths, seed)
    weights = [w + np.float32(0.05) * rng.standard_normal(w.shape).astype(np.float32) for w in weights]
    x64 = np.asarray(batches[s][0]['input_1'], np.float64)
    y64 = np.asarray(batches[s][1], np.float64)
    loss, g64, p64, kink = host_dnn_pearson.loss_and_grads(weights, x64, y64)
    if kink >= KINK:
      break
  else:
    pytest.fail('no seed keeps the ReLU inputs %g away from their kinks' % KINK)
  res = ds.resolved()
  x, _, y, offs = res.device_arrays(h)
  params = h.to_device(flat(weights))
  grad, sums = device.mlp_grad(x, y, offs, pre, post, hidden, params, batch, s, input_offset=off,
                               rows_used=res.rows_used(), handle=h, loss='pearson')
  got = split(grad.cpu().numpy(), widths)
  s7 = sums.cpu().numpy()
  assert s7.shape == (7,)
  dists = grad_distances(got, g64[:-1])
  worst = max(dists.values())
  loss_dist = abs(batch * s7[6] - batch * loss)
  mse64 = float(np.mean((p64 - y64) ** 2))
  mse_dist = abs(s7[5] / (batch * d) - mse64) / mse64
  r_dist = abs(_r_of_sums(s7, batch) - host_dnn.pearson_first(p64, y64))
  print('pearson grad %s: per tensor %s, B |dL| %.3g, mse rel %.3g, r abs %.3g, kink %.3g' % (
      (hidden, c, pre, post, batch, d, off, mixup), dists, loss_dist, mse_dist, r_dist, kink))
  parity_log.record('dnn_pearson_grad', shape=str((hidden, c, pre, post, batch, d, off, mixup)), rel=worst,
                    loss_times_b=loss_dist, mse_rel=mse_dist, r_abs=r_dist, kink=kink)
  assert all(np.all(np.isfinite(g)) for g in got) and np.all(np.isfinite(s7))
  assert_within(dists, GRAD_BOUND)
  assert np.all(got[-1] == 0.0), got[-1]                       # the output bias: exactly zero
  assert np.all(g64[-1] == 0.0)
  assert loss_dist <= 1e-5 * d, loss_dist
  assert mse_dist <= 1e-6, mse_dist                            # the six old sums: the bounds of the mse tests
  assert r_dist <= 1e-5, r_dist


def _r_of_sums(s, rows):
  """Pearson r of output 0 from the first five step sums."""
  n = float(rows)
  va, vb, cov = s[2] - s[0] ** 2 / n, s[3] - s[1] ** 2 / n, s[4] - s[0] * s[1] / n
  return float(cov / np.sqrt(va * vb))


@pytest.mark.parametrize('case', GRID, ids=lambda c: '%s-c%d-l%d-B%d-D%d-o%d' % (
    'x'.join(map(str, c[0])) or 'none', c[1], c[2] + c[3] + 1, c[4], c[5], c[6]))
def test_gradients_match_float64(case):
  _grad_case(*case)


def test_gradients_of_a_mixup_batch_dataset():
  _grad_case([20, 20], 4, 2, 2, 128, 1, 0, mixup=True)


# ---- trajectories -----------------------------------------------------------------------------------------
C, PRE, POST, D, BATCH, HIDDEN = 4, 2, 1, 2, 32, [8, 4]
WIDTHS = [C * (PRE + 1 + POST)] + HIDDEN + [D]


def _trajectory_data(shuffle_seed, scale=1.0):
  """(seed, files, Dataset, float64 weights, float64 history, kink) of the first seed whose float64 trajectory
  stays 1e-5 away from the ReLU kinks."""
  from telluride_decoding_amd import brain_data
  for seed in range(8):
    rng = np.random.default_rng(50 + seed)
    files = make_files(rng, [101, 130, 95], C, D)
    if scale != 1.0:
      files = [(x, z, (np.float32(scale) * y).astype(np.float32), a) for x, z, y, a in files]
    ds = brain_data.Dataset(files, BATCH, PRE, POST)
    x64, y64 = host_dnn.stream(files, BATCH, PRE, POST)
    w0 = host_dnn.glorot(WIDTHS, seed)
    w64, _, hist64, kink = host_dnn_pearson.train(w0, x64, y64, BATCH, 3, 1e-3, shuffle_seed=shuffle_seed)
    if kink >= 1e-5:
      return seed, files, ds, w64, hist64, kink
  pytest.fail('no seed keeps the trajectory away from the ReLU kinks')


def _fit(ds, seed, shuffle_seed, loss):
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelDNN(ds, HIDDEN, seed=seed)
  m.compile(loss=loss)
  hist = m.fit(ds, epochs=3, shuffle_seed=shuffle_seed).history
  return m, hist


def _trajectory(shuffle_seed):
  from telluride_decoding_amd import brain_model
  seed, files, ds, w64, hist64, kink = _trajectory_data(shuffle_seed)
  runs = []
  for loss in (brain_model.PearsonCorrelationLoss(), 'pearson'):
    m, hist = _fit(ds, seed, shuffle_seed, loss)
    runs.append((m.get_weights(), hist, m))
  for a, b in zip(runs[0][0], runs[1][0]):
    np.testing.assert_array_equal(a, b)                      # bitwise reproducible
  assert runs[0][1] == runs[1][1]
  wmax = max(float(np.max(np.abs(b))) for b in w64)
  wdist = max(float(np.max(np.abs(a - b))) for a, b in zip(runs[0][0], w64)) / wmax
  hist = runs[0][1]
  for key in ('loss', 'pearson_correlation_first', 'mse'):
    assert np.asarray(hist[key]).shape == (3,)
  ldist = float(np.max(np.abs(np.asarray(hist['loss']) - np.asarray(hist64['loss'])))) * BATCH
  rdist = float(np.max(np.abs(np.asarray(hist['pearson_correlation_first']) -
                              np.asarray(hist64['pearson_correlation_first']))))
  mdist = float(np.max(np.abs(np.asarray(hist['mse']) - np.asarray(hist64['mse'])) / np.asarray(hist64['mse'])))
  # evaluate at the trained weights: the float64 per-minibatch means of the restatement
  m = runs[0][2]
  w = m.get_weights()
  losses, rs, mses = [], [], []
  batches = list(ds)
  for feats, y in batches:
    p = host_dnn.forward(w, np.asarray(feats['input_1'], np.float64))[0]
    y = np.asarray(y, np.float64)
    losses.append(host_dnn_pearson.loss_and_dz(p, y)[0])
    rs.append(host_dnn.pearson_first(p, y))
    mses.append(np.mean((p - y) ** 2))
  ev, ev_it = m.evaluate(ds), m.evaluate(batches)
  edist = max(abs(e['loss'] - np.mean(losses)) * BATCH for e in (ev, ev_it))
  print('pearson trajectory (shuffle %s): weights %.3g, B |dL| %.3g, r %.3g, mse rel %.3g, evaluate B |dL| %.3g, '
        'kink %.3g' % (shuffle_seed, wdist, ldist, rdist, mdist, edist, kink))
  parity_log.record('dnn_pearson_trajectory', shuffle=str(shuffle_seed), weights=wdist, loss_times_b=ldist,
                    r_abs=rdist, mse_rel=mdist, evaluate_loss_times_b=edist, kink=kink)
  assert wdist <= 1e-4, wdist
  assert ldist <= 1e-5, ldist
  assert rdist <= 1e-5, rdist
  assert mdist <= 1e-5, mdist
  assert edist <= 1e-5, edist
  for e in (ev, ev_it):
    assert sorted(e) == ['loss', 'mse', 'pearson_correlation_first']
    assert abs(e['mse'] - np.mean(mses)) <= 1e-5 * np.mean(mses)
    assert abs(e['pearson_correlation_first'] - np.mean(rs)) <= 1e-5
  # the history's loss is the correlation loss, not the mse, and the net was trained on it
  assert all(v < 0.0 for v in hist['loss'][1:]) and all(v > 0.0 for v in hist['mse'])
  assert hist['loss'][-1] < hist['loss'][0]


def test_trajectory_in_order():
  _trajectory(None)


def test_trajectory_shuffled():
  _trajectory(12345)


def test_compile_for_another_loss_starts_afresh_and_trains_differently():
  seed, files, ds, _, _, _ = _trajectory_data(None)
  m_p, _ = _fit(ds, seed, None, 'pearson')
  m_m, _ = _fit(ds, seed, None, 'mse')
  assert any(not np.array_equal(a, b) for a, b in zip(m_p.get_weights(), m_m.get_weights()))
  # the output bias never moves on the correlation loss; on the mse it does
  np.testing.assert_array_equal(m_p.get_weights()[-1], 0.0)
  assert np.all(m_m.get_weights()[-1] != 0.0)
  # compile(loss=...) resets the optimizer: the same three epochs again from the same weights
  w0 = host_dnn.glorot(WIDTHS, seed)
  m_m.set_weights(w0)
  m_m.compile(loss='pearson')
  m_m.fit(ds, epochs=3)
  for a, b in zip(m_m.get_weights(), m_p.get_weights()):
    np.testing.assert_array_equal(a, b)


# ---- scale invariance ---------------------------------------------------------------------------------------
def test_the_targets_scale_does_not_change_the_fit():
  seed, _, ds1, w64, _, _ = _trajectory_data(None)
  seed4, _, ds4, _, _, _ = _trajectory_data(None, scale=4.0)
  assert seed4 == seed
  m1, h1 = _fit(ds1, seed, None, 'pearson')
  m4, h4 = _fit(ds4, seed, None, 'pearson')
  wmax = max(float(np.max(np.abs(w))) for w in m1.get_weights())
  dist = max(float(np.max(np.abs(a - b))) for a, b in zip(m1.get_weights(), m4.get_weights())) / wmax
  bitwise = all(np.array_equal(a, b) for a, b in zip(m1.get_weights(), m4.get_weights()))
  print('pearson scale invariance: weights %.3g, bitwise %s' % (dist, bitwise))
  parity_log.record('dnn_pearson_scale', weights=dist, bitwise=str(bitwise))
  assert dist <= 1e-6, dist
  assert h1['loss'] == pytest.approx(h4['loss'], rel=1e-9, abs=1e-12)
  assert not np.allclose(h1['mse'], h4['mse'], rtol=1e-2)     # (the mse does see the scale)


# ---- the zero rule on the device ---------------------------------------------------------------------------
def test_a_constant_target_column_contributes_nothing():
  from telluride_decoding_amd import brain_data, device
  h = device.default_handle()
  rng = np.random.default_rng(5)
  files = [(x, z, np.concatenate([y[:, :1], np.zeros_like(y[:, :1])], axis=1), a)
           for x, z, y, a in make_files(rng, [70, 90], C, D)]
  ds = brain_data.Dataset(files, BATCH, PRE, POST)
  batches = list(ds)
  for seed in range(8):
    weights = host_dnn.glorot(WIDTHS, seed)
    weights = [w + np.float32(0.05) * rng.standard_normal(w.shape).astype(np.float32) for w in weights]
    x64, y64 = np.asarray(batches[2][0]['input_1'], np.float64), np.asarray(batches[2][1], np.float64)
    loss, g64, p64, kink = host_dnn_pearson.loss_and_grads(weights, x64, y64)
    if kink >= KINK:
      break
  else:
    pytest.fail('no seed keeps the ReLU inputs away from their kinks')
  assert np.all(y64[:, 1] == 0.0) and np.all(g64[-2][:, 1] == 0.0)
  x, _, y, offs = ds.device_arrays(h)
  grad, sums = device.mlp_grad(x, y, offs, PRE, POST, HIDDEN, h.to_device(flat(weights)), BATCH, 2,
                               rows_used=ds.rows_used(), handle=h, loss='pearson')
  got, s7 = split(grad.cpu().numpy(), WIDTHS), sums.cpu().numpy()
  assert all(np.all(np.isfinite(g)) for g in got) and np.all(np.isfinite(s7))
  assert np.all(got[-2][:, 1] == 0.0) and np.all(got[-1] == 0.0)
  dists = [float(np.max(np.abs(gg - gw)) / np.max(np.abs(gw))) for gg, gw in zip(got[:-1], g64[:-1])]
  ldist = abs(s7[6] - loss) * BATCH
  one = host_dnn_pearson.loss_and_dz(p64[:, :1], y64[:, :1])[0]
  print('pearson zero column: per tensor %s, B |dL| %.3g' % (dists, ldist))
  parity_log.record('dnn_pearson_zero_column', rel=max(dists), loss_times_b=ldist)
  assert max(dists) <= GRAD_BOUND
  assert ldist <= 1e-5 * D
  assert abs(loss - one) <= 1e-15                             # the loss is the other column's alone


def test_a_constant_prediction_leaves_every_weight_as_it_was():
  from telluride_decoding_amd import brain_data, brain_model
  rng = np.random.default_rng(6)
  ds = brain_data.Dataset(make_files(rng, [BATCH + 5], C, D), BATCH, PRE, POST)
  assert ds.num_batches() == 1
  m = brain_model.BrainModelDNN(ds, HIDDEN, seed=1)
  w0 = m.get_weights()
  w0[-2][:] = 0.0
  w0[-1][:] = np.float32(0.3)
  m.set_weights(w0)
  m.compile(loss=brain_model.PearsonCorrelationLoss(), learning_rate=1e-2)
  hist = m.fit(ds, epochs=1).history
  for a, b in zip(m.get_weights(), w0):
    np.testing.assert_array_equal(a, b)
  assert hist['loss'] == [0.0] and hist['pearson_correlation_first'] == [0.0]
  assert np.isfinite(hist['mse'][0])
  assert m.evaluate(ds)['loss'] == 0.0


# ---- the old path --------------------------------------------------------------------------------------------
def _abi_args(h, ds, weights):
  from telluride_decoding_amd import _lib, device
  x, _, y, offs = ds.device_arrays(h)
  offs_a, offs_p = _lib.i64_array(offs)
  used_a, used_p = _lib.i64_array(ds.rows_used())
  hid_a, hid_p = device._i32_array(HIDDEN)
  keep = (x, y, offs_a, used_a, hid_a)
  head = (h.ptr, device._ptr(x), x.stride(0), offs_p, len(offs_a) - 1, C, PRE, POST, 0, used_p, device._ptr(y),
          y.stride(0), D, hid_p, len(HIDDEN), BATCH)
  return keep, head, h.to_device(flat(weights))


def test_loss_zero_of_the_new_entry_points_is_the_old_path_bitwise():
  from telluride_decoding_amd import device
  h = device.default_handle()
  seed, _, ds, _, _, _ = _trajectory_data(12345)
  steps = ds.num_batches()
  w0 = host_dnn.glorot(WIDTHS, seed)
  out = []
  for new in (False, True):
    keep, head, params = _abi_args(h, ds, w0)
    state = h.zeros((int(params.numel()),))
    stats = h.zeros((3 * steps, 6), 'float64')
    tail = (3, device._ptr(params), device._ptr(state), 1e-3, 0.9, 1e-7, 12345, device._ptr(stats))
    h.check(h.lib.td_mlp_train_loss(*head, *tail, 0) if new else h.lib.td_mlp_train(*head, *tail))
    grad = h.zeros((int(params.numel()),))
    gstats = h.zeros((6,), 'float64')
    gtail = (1, device._ptr(params), device._ptr(grad), device._ptr(gstats))
    h.check(h.lib.td_mlp_grad_loss(*head, *gtail, 0) if new else h.lib.td_mlp_grad(*head, *gtail))
    out.append([t.cpu().numpy() for t in (params, state, stats, grad, gstats)])
  for a, b in zip(*out):
    np.testing.assert_array_equal(a, b)
  assert np.all(out[0][2][:, 5] > 0.0)                         # (every step reported its sums)
  assert not np.array_equal(out[0][0], flat(w0))             # (it did train)


# ---- the reference's recipes trained on the new loss ------------------------------------------------------------
def _fit_dnn(ds, hidden, epochs):
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelDNN(ds, hidden)
  m.compile(optimizer=brain_model.RMSprop(learning_rate=1e-3), loss=brain_model.PearsonCorrelationLoss(),
            metrics=[brain_model.pearson_correlation_first])
  hist = m.fit(ds, epochs=epochs)
  return m, hist, m.evaluate(ds)


def test_sin_target_trained_on_the_correlation():
  """Thresholds from the float64 restatement: r = 0.832 .. 0.862 over glorot seeds 0 - 4 (a float32 emulation:
  0.830 .. 0.871); its mse stays near 0.47, which an mse-trained net brings to 0.12."""
  ds = simply_scaled()
  _, hist, metrics = _fit_dnn(ds, [40, 20, 10], 100)
  print('pearson sin target: %s' % metrics)
  parity_log.record('dnn_pearson_sin', **metrics)
  assert len(hist.history['loss']) == 100 and np.all(np.isfinite(hist.history['loss']))
  assert metrics['pearson_correlation_first'] > 0.80
  assert metrics['loss'] < -0.80 / 1000
  assert metrics['mse'] > 0.3


def test_iir_target_trained_on_the_correlation():
  """Thresholds from the float64 restatement: r = 0.9993 with 32 frames of context, 0.831 without."""
  _, _, m32 = _fit_dnn(iir(32), [40, 20, 10], 10)
  _, _, m0 = _fit_dnn(iir(0), [40, 20, 10], 10)
  print('pearson iir target: pre 32 %s, pre 0 %s' % (m32, m0))
  parity_log.record('dnn_pearson_iir', r32=m32['pearson_correlation_first'], loss32=m32['loss'],
                    r0=m0['pearson_correlation_first'], loss0=m0['loss'])
  assert m32['pearson_correlation_first'] > 0.95
  assert 0.8 < m0['pearson_correlation_first'] < 0.95


# ---- limits and errors -----------------------------------------------------------------------------------------
def test_limits_and_a_wrong_loss_code():
  from telluride_decoding_amd import _lib, brain_data, brain_model, device
  h = device.default_handle()
  rng = np.random.default_rng(3)

  def ds_of(c, pre, post, d, batch, n=4200):
    return brain_data.Dataset(make_files(rng, [n], c, d), batch, pre, post)
  for ds, hidden in [(ds_of(2, 0, 0, 9, 64), [4]), (ds_of(2, 0, 0, 1, 2049), [4]), (ds_of(2, 0, 0, 1, 64), [65])]:
    m = brain_model.BrainModelDNN(ds, hidden)
    m.compile(loss='pearson')
    before = m.get_weights()
    with pytest.raises(ValueError):
      m.fit(ds)
    for a, b in zip(before, m.get_weights()):
      np.testing.assert_array_equal(a, b)
  # the C entry points refuse the same shapes and an unknown loss code with nothing queued
  ds = ds_of(2, 0, 0, 1, 64)
  x, _, y, offs = ds.device_arrays(h)
  params = h.to_device(np.ones(2 * 65 + 65 + 65 + 1, np.float32))
  state = h.zeros((int(params.numel()),))
  with pytest.raises(ValueError, match='hidden layer'):
    device.mlp_train(x, y, offs, 0, 0, [65], params, state, 64, 1, 1e-3, 0.9, 1e-7, handle=h, loss='pearson')
  with pytest.raises(ValueError, match='batch'):
    device.mlp_train(x, y, offs, 0, 0, [4], params, state, 2049, 1, 1e-3, 0.9, 1e-7, handle=h, loss='pearson')
  ds = brain_data.Dataset(make_files(rng, [200], C, D), BATCH, PRE, POST)
  keep, head, params = _abi_args(h, ds, host_dnn.glorot(WIDTHS, 0))
  state = h.zeros((int(params.numel()),))
  stats = h.zeros((ds.num_batches(), 7), 'float64')
  grad = h.zeros((int(params.numel()),))
  before = params.cpu().numpy()
  for code in (2, -1):
    assert h.lib.td_mlp_train_loss(*head, 1, device._ptr(params), device._ptr(state), 1e-3, 0.9, 1e-7, -1,
                                   device._ptr(stats), code) == _lib.TD_ERR_INVALID
    assert h.lib.td_mlp_grad_loss(*head, 0, device._ptr(params), device._ptr(grad), device._ptr(stats),
                                  code) == _lib.TD_ERR_INVALID
  h.synchronize()
  np.testing.assert_array_equal(params.cpu().numpy(), before)
  assert float(state.abs().sum()) == 0.0 and float(stats.abs().sum()) == 0.0
