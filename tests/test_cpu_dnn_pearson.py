"""BrainModelDNN on the Pearson correlation loss without a GPU: what compile accepts, the float64 restatement of
tests/host_dnn_pearson.py itself (finite differences, the exact-zero output bias gradient, the zero rule) and
the history the seven per-step sums give."""
import numpy as np
import pytest

from tests import host_dnn
from tests import host_dnn_pearson


def _dataset(c=2, pre=1, post=1, d=1, n=300, batch=50):
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(0)
  x = rng.standard_normal((n, c)).astype(np.float32)
  y = rng.standard_normal((n, d)).astype(np.float32)
  z = np.zeros((n, 1), np.float32)
  return brain_data.Dataset([(x, z, y, z)], batch, pre, post)


def test_compile_accepts_the_pearson_loss():
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelDNN(_dataset(), [4])
  assert m.loss == 'mse'
  m.compile(loss=brain_model.PearsonCorrelationLoss())
  assert m.loss == 'pearson' and isinstance(m.optimizer, brain_model.RMSprop)
  m.compile()
  assert m.loss == 'mse'
  m.compile(loss=[brain_model.PearsonCorrelationLoss()])
  assert m.loss == 'pearson'
  m.compile(loss=['mse'])
  assert m.loss == 'mse'
  m.compile(loss='pearson', learning_rate=0.02)
  assert m.loss == 'pearson' and m.optimizer.learning_rate == 0.02
  m._state = object()
  m.compile(loss='pearson')                                   # every compile starts a fresh optimizer state
  assert m._state is None
  with pytest.raises(NotImplementedError, match='mae'):
    m.compile(loss='mae')
  assert m.loss == 'pearson'                                  # a refused compile changes nothing
  with pytest.raises(NotImplementedError, match='Loss'):
    m.compile(loss=['pearson', 'pearson'])
  with pytest.raises(NotImplementedError, match='Loss'):
    m.compile(loss=['mse', brain_model.PearsonCorrelationLoss()])
  with pytest.raises(NotImplementedError, match='Loss'):
    m.compile(loss=brain_model.PearsonCorrelationLoss)        # the class, not an instance: Keras would call it
  assert m.metrics_names == ['loss', 'pearson_correlation_first', 'mse']


def test_device_wrappers_refuse_an_unknown_loss_before_touching_the_device():
  from telluride_decoding_amd import device
  with pytest.raises(ValueError, match='loss'):
    device.mlp_train(None, None, [0, 1], 0, 0, [], None, None, 1, 1, 1e-3, 0.9, 1e-7, handle=object(), loss='mae')
  with pytest.raises(ValueError, match='loss'):
    device.mlp_grad(None, None, [0, 1], 0, 0, [], None, 1, 0, handle=object(), loss=1)


def _net(seed=7):
  rng = np.random.default_rng(seed)
  widths = [6, 5, 3, 2]
  w = [v.astype(np.float64) for v in host_dnn.glorot(widths, seed)]
  w = [v + 0.1 * rng.standard_normal(v.shape) for v in w]
  return w, rng.standard_normal((40, 6)), rng.standard_normal((40, 2))


def test_restatement_gradient_matches_central_differences():
  w, x, y = _net()
  loss, grads, _, kink = host_dnn_pearson.loss_and_grads(w, x, y)
  assert kink > 1e-6
  h = 1e-6
  worst, gmax = 0.0, max(float(np.max(np.abs(g))) for g in grads)
  for t in range(len(w)):
    for idx in np.ndindex(w[t].shape):
      wp = [v.copy() for v in w]
      wm = [v.copy() for v in w]
      wp[t][idx] += h
      wm[t][idx] -= h
      fd = (host_dnn_pearson.loss_and_grads(wp, x, y)[0] - host_dnn_pearson.loss_and_grads(wm, x, y)[0]) / (2 * h)
      worst = max(worst, abs(fd - grads[t][idx]))
  print('max |fd - g| = %.3g at max |g| = %.3g' % (worst, gmax))
  assert gmax > 1e-3
  assert worst <= 1e-9, worst


def test_restatement_loss_is_minus_the_mean_correlation_sum():
  rng = np.random.default_rng(3)
  p, y = rng.standard_normal((40, 3)), rng.standard_normal((40, 3))
  loss, dz, r = host_dnn_pearson.loss_and_dz(p, y)
  want = [np.corrcoef(p[:, o], y[:, o])[0, 1] for o in range(3)]
  np.testing.assert_allclose(r, want, rtol=1e-12)
  assert loss == pytest.approx(-np.sum(want) / 40, rel=1e-12)
  # invariant to the scale and offset of either side, and dL/dp sums to zero over the rows
  loss2, dz2, _ = host_dnn_pearson.loss_and_dz(p, 4.0 * y + 3.0)
  assert loss2 == pytest.approx(loss, rel=1e-12)
  np.testing.assert_allclose(dz2, dz, rtol=1e-9, atol=1e-15)
  assert np.max(np.abs(dz.sum(axis=0))) <= 1e-15


def test_restatement_output_bias_gradient_is_exactly_zero():
  w, x, y = _net(5)
  _, grads, _, _ = host_dnn_pearson.loss_and_grads(w, x, y)
  assert np.all(grads[-1] == 0.0) and grads[-1].shape == (2,)
  assert all(np.max(np.abs(g)) > 0 for g in grads[:-1])


def test_restatement_zero_rule():
  w, x, y = _net(9)
  # a constant target column: r = 0 and no gradient from it; the other column is untouched
  yc = y.copy()
  yc[:, 1] = 0.25
  p = host_dnn.forward(w, x)[0]
  loss, dz, r = host_dnn_pearson.loss_and_dz(p, yc)
  loss0, dz0, r0 = host_dnn_pearson.loss_and_dz(p[:, :1], y[:, :1])
  assert r[1] == 0.0 and np.all(dz[:, 1] == 0.0)
  assert r[0] == pytest.approx(r0[0], rel=1e-13) and loss == pytest.approx(loss0, rel=1e-13)
  np.testing.assert_allclose(dz[:, 0], dz0[:, 0], rtol=1e-12, atol=1e-18)
  _, grads, _, _ = host_dnn_pearson.loss_and_grads(w, x, yc)
  assert all(np.all(np.isfinite(g)) for g in grads)
  assert np.all(grads[-2][:, 1] == 0.0)
  # a constant column that is not a round number: the raw sums leave a residue, the rule still fires
  yc[:, 1] = 0.1 + 1e-3 * np.pi
  assert host_dnn_pearson.constant_columns(p, yc).tolist() == [False, True]
  # an all-zero output layer: p is constant, L = 0 and every gradient is zero
  wz = [v.copy() for v in w]
  wz[-2][:] = 0.0
  wz[-1][:] = 0.3
  loss, grads, p, _ = host_dnn_pearson.loss_and_grads(wz, x, y)
  assert loss == 0.0 and np.all(p == 0.3)
  assert all(np.all(g == 0.0) for g in grads)
  w1, _ = host_dnn.rmsprop(wz, [np.zeros_like(v) for v in wz], grads, 1e-3)
  assert all(np.array_equal(a, b) for a, b in zip(w1, wz))


def test_history_from_the_seven_step_sums():
  from telluride_decoding_amd import brain_model
  rng = np.random.default_rng(1)
  rows, d, epochs, steps = 40, 3, 2, 3
  sums = np.zeros((epochs, steps, 7))
  want = {'loss': [], 'pearson_correlation_first': [], 'mse': []}
  for e in range(epochs):
    losses, rs, mses = [], [], []
    for s in range(steps):
      p, y = rng.standard_normal((rows, d)), rng.standard_normal((rows, d))
      if (e, s) == (1, 2):
        p[:, 0] = 0.5                                          # a constant column: r = 0
      step_loss = host_dnn_pearson.loss_and_dz(p, y)[0]
      sums[e, s] = [p[:, 0].sum(), y[:, 0].sum(), (p[:, 0] ** 2).sum(), (y[:, 0] ** 2).sum(),
                    (p[:, 0] * y[:, 0]).sum(), ((p - y) ** 2).sum(), step_loss]
      losses.append(step_loss)
      mses.append(np.mean((p - y) ** 2))
      rs.append(host_dnn.pearson_first(p, y))
      # the evaluate route: the same loss from the five raw sums of every column
      s5 = np.stack([p.sum(0), y.sum(0), (p * p).sum(0), (y * y).sum(0), (p * y).sum(0)], axis=-1)
      assert float(brain_model.pearson_loss_from_sums(s5, rows)) == pytest.approx(step_loss, rel=1e-12)
    want['loss'].append(np.mean(losses))
    want['mse'].append(np.mean(mses))
    want['pearson_correlation_first'].append(np.mean(rs))
  hist = brain_model.History(brain_model.history_from_sums(sums, rows, d)).history
  assert sorted(hist) == ['loss', 'mse', 'pearson_correlation_first']
  assert all(len(v) == epochs for v in hist.values())
  np.testing.assert_allclose(hist['loss'], want['loss'], rtol=1e-15)
  np.testing.assert_allclose(hist['mse'], want['mse'], rtol=1e-12)
  np.testing.assert_allclose(hist['pearson_correlation_first'], want['pearson_correlation_first'], rtol=1e-10)
  assert np.all(np.asarray(hist['loss']) < 0.5) and not np.allclose(hist['loss'], hist['mse'])
  # six slots: as before, 'loss' is the mse
  hist6 = brain_model.history_from_sums(sums[..., :6], rows, d)
  assert hist6['loss'] == hist6['mse'] == hist['mse']
