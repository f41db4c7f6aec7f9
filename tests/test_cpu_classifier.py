"""BrainModelClassifier without a GPU: the call surface against the reference's (G14), the constructor and
compile errors, the history the per-step sums give, the float64 restatement of tests/host_classifier.py itself
(finite differences, two Adam steps by hand), and brain_data.mismatch_batch_randomization with the properties
the reference's own test checks (test/brain_data_test.py)."""
import numpy as np
import pytest

from tests import host_classifier as hc
from tests import host_dnn
from tests.surface import member_rows
from tests.test_cpu_surface import _golden, _leading_matches


def _dataset(c=2, pre=1, post=1, c2=1, pre2=0, post2=2, d=1, n=300, batch=50):
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(0)
  x = rng.standard_normal((n, c)).astype(np.float32)
  x2 = rng.standard_normal((n, c2)).astype(np.float32)
  y = (rng.standard_normal((n, d)) > 0).astype(np.float32)
  z = np.zeros((n, 1), np.float32)
  return brain_data.Dataset([(x, x2, y, z)], batch, pre, post, pre2, post2)


def test_surface_matches_the_reference():
  from telluride_decoding_amd import brain_model
  ref = _golden()['surface']['brain_model']['BrainModelClassifier']
  problems = []
  for name, rows in ref['members'].items():
    assert hasattr(brain_model.BrainModelClassifier, name), name
    where = ('brain_model', 'BrainModelClassifier', name)
    ours = member_rows(brain_model.BrainModelClassifier, name)
    if name == 'compile':        # the optimizer and loss defaults name TF objects there
      theirs = {r[0]: r[2] for r in rows}
      ours = [r if r[0] not in ('optimizer', 'loss') else [r[0], r[1], theirs[r[0]]] for r in ours]
    problems += _leading_matches(rows, ours, where)
  assert not problems, problems
  assert brain_model.BrainModelClassifier(_dataset()).metrics_names == ['loss', 'accuracy']


def test_constructor_errors_and_widths():
  from telluride_decoding_amd import brain_model
  ds = _dataset(c=3, pre=2, post=1, c2=2, pre2=1, post2=1, d=2)
  with pytest.raises(TypeError, match='Dataset must be a tf.data.datasert'):      # TypeError, unlike BrainModelDNN
    brain_model.BrainModelClassifier([1, 2, 3])
  with pytest.raises(TypeError, match='Num_hidden_list must be an list'):
    brain_model.BrainModelClassifier(ds, (20, 20))
  m = brain_model.BrainModelClassifier(ds, tensorboard_dir='/nonexistent')
  assert [w.shape for w in m.get_weights()] == [(12 + 6, 2), (2,)]
  m = brain_model.BrainModelClassifier(ds, [5, 4], seed=3)
  assert [w.shape for w in m.get_weights()] == [(18, 5), (5,), (5, 4), (4,), (4, 2), (2,)]
  for u, v in zip(m.get_weights(), host_dnn.glorot([18, 5, 4, 2], 3)):           # fan_in = K1 + K2
    np.testing.assert_array_equal(u, v)
  w = [a + 1 for a in m.get_weights()]
  m.set_weights(w)
  for u, v in zip(m.weight_matrices, w):
    np.testing.assert_array_equal(u, v)
  with pytest.raises(ValueError):
    m.set_weights(w[:-1])


def test_compile_forms_and_errors():
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelClassifier(_dataset(), [4])
  m.compile()
  opt = m.optimizer
  assert isinstance(opt, brain_model.Adam)
  assert (opt.learning_rate, opt.beta_1, opt.beta_2, opt.epsilon, opt.amsgrad) == (1e-3, 0.9, 0.999, 1e-7, False)
  m.compile(learning_rate=0.01)
  assert m.optimizer.learning_rate == 0.01
  m.compile(optimizer='adam', loss='binary_crossentropy', metrics=['accuracy'], learning_rate=0.02)
  assert m.optimizer.learning_rate == 0.02
  m.compile(optimizer=brain_model.Adam, loss=[brain_model.BinaryCrossentropy()])
  m.compile(optimizer=brain_model.Adam(learning_rate=0.03, beta_1=0.8), loss=['binary_crossentropy'])
  assert (m.optimizer.learning_rate, m.optimizer.beta_1) == (0.03, 0.8)
  m.compile(optimizer=lambda learning_rate: brain_model.Adam(learning_rate=learning_rate, epsilon=1e-6),
            learning_rate=0.04)
  assert (m.optimizer.learning_rate, m.optimizer.epsilon) == (0.04, 1e-6)
  with pytest.raises(NotImplementedError, match='amsgrad'):
    m.compile(optimizer=brain_model.Adam(amsgrad=True))
  with pytest.raises(NotImplementedError, match='rmsprop'):
    m.compile(optimizer='rmsprop')
  with pytest.raises(NotImplementedError, match='Optimizer'):
    m.compile(optimizer=brain_model.RMSprop())
  with pytest.raises(NotImplementedError, match='Optimizer'):
    m.compile(optimizer=lambda learning_rate: object())
  with pytest.raises(NotImplementedError, match='mse'):
    m.compile(loss='mse')
  with pytest.raises(NotImplementedError, match='Loss'):
    m.compile(loss=['binary_crossentropy', 'binary_crossentropy'])
  with pytest.raises(NotImplementedError, match='from_logits'):
    brain_model.BinaryCrossentropy(from_logits=True)
  with pytest.raises(NotImplementedError, match='label_smoothing'):
    brain_model.BinaryCrossentropy(label_smoothing=0.1)
  with pytest.raises(RuntimeError, match='compile'):
    brain_model.BrainModelClassifier(_dataset(), [4]).fit(_dataset())
  # BrainModelDNN stays RMSprop / mse only
  with pytest.raises(NotImplementedError):
    brain_model.BrainModelDNN(_dataset(), [4]).compile(optimizer=brain_model.Adam)


def test_compile_resets_the_optimizer_state():
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelClassifier(_dataset(), [4])
  m.compile()
  m._state, m._updates = object(), 17          # what a fit leaves behind
  m.compile()
  assert m._state is None and m._updates == 0


def test_history_from_the_step_sums():
  from telluride_decoding_amd import brain_model
  rng = np.random.default_rng(1)
  rows, d, epochs, steps = 40, 3, 2, 3
  sums = np.zeros((epochs, steps, 6))
  want = {'loss': [], 'accuracy': []}
  for e in range(epochs):
    losses, accs = [], []
    for s in range(steps):
      z = 3 * rng.standard_normal((rows, d))
      y = (rng.standard_normal((rows, d)) > 0).astype(np.float64)
      sums[e, s, 0] = hc.correct(z, y)
      sums[e, s, 5] = hc.entry_losses(z, y).sum()
      losses.append(np.mean(hc.entry_losses(z, y)))
      accs.append(np.mean((z > 0) == (y > 0.5)))
    want['loss'].append(np.mean(losses))
    want['accuracy'].append(np.mean(accs))
  hist = brain_model.History(brain_model.classifier_history_from_sums(sums, rows, d)).history
  assert sorted(hist) == ['accuracy', 'loss']
  assert all(len(v) == epochs for v in hist.values())
  np.testing.assert_allclose(hist['loss'], want['loss'], rtol=1e-12)
  np.testing.assert_allclose(hist['accuracy'], want['accuracy'], rtol=1e-12)


def test_restatement_loss_is_the_clipped_probability_form_where_both_are_defined():
  """-[y log s + (1 - y) log(1 - s)] of s = sigma(z), for moderate |z|."""
  rng = np.random.default_rng(5)
  z = 4 * rng.standard_normal((50, 3))
  y = (rng.standard_normal((50, 3)) > 0).astype(np.float64)
  s = hc.sigmoid(z)
  np.testing.assert_allclose(hc.entry_losses(z, y), -(y * np.log(s) + (1 - y) * np.log1p(-s)), rtol=1e-12)
  big = np.array([[800.0, -800.0]])
  assert np.all(np.isfinite(hc.entry_losses(big, np.array([[0.0, 0.0]]))))
  np.testing.assert_array_equal(hc.sigmoid(big), [[1.0, 0.0]])


def test_restatement_gradients_match_finite_differences():
  rng = np.random.default_rng(2)
  widths = [5, 4, 3, 2]
  w = [v.astype(np.float64) for v in host_dnn.glorot(widths, 7)]
  w = [v + 0.1 * rng.standard_normal(v.shape) for v in w]
  x = rng.standard_normal((9, 5))
  y = (rng.standard_normal((9, 2)) > 0).astype(np.float64)
  loss, grads, _, margin, _ = hc.loss_and_grads(w, x, y)
  assert margin > 1e-6
  h = 1e-6
  for t in range(len(w)):
    for idx in np.ndindex(w[t].shape):
      wp = [v.copy() for v in w]
      wm = [v.copy() for v in w]
      wp[t][idx] += h
      wm[t][idx] -= h
      fd = (hc.loss_and_grads(wp, x, y)[0] - hc.loss_and_grads(wm, x, y)[0]) / (2 * h)
      assert abs(fd - grads[t][idx]) <= 1e-7 * max(1.0, abs(fd)), (t, idx)


def test_restatement_adam_two_steps_by_hand():
  lr, b1, b2, eps = 0.1, 0.9, 0.999, 1e-7
  w, m, v = [np.array([1.0])], [np.array([0.0])], [np.array([0.0])]
  w, m, v = hc.adam(w, m, v, [np.array([0.5])], 1, lr, b1, b2, eps)
  m1, v1 = 0.1 * 0.5, 0.001 * 0.25
  lr1 = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
  w1 = 1.0 - lr1 * m1 / (np.sqrt(v1) + eps)
  assert m[0][0] == pytest.approx(m1, rel=1e-15) and v[0][0] == pytest.approx(v1, rel=1e-15)
  assert w[0][0] == pytest.approx(w1, rel=1e-15)
  assert w1 == pytest.approx(1.0 - lr, rel=1e-5)       # the first Adam step moves every weight by lr
  w, m, v = hc.adam(w, m, v, [np.array([-0.2])], 2, lr, b1, b2, eps)
  m2, v2 = 0.9 * m1 + 0.1 * -0.2, 0.999 * v1 + 0.001 * 0.04
  lr2 = lr * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
  assert m[0][0] == pytest.approx(m2, rel=1e-15) and v[0][0] == pytest.approx(v2, rel=1e-15)
  assert w[0][0] == pytest.approx(w1 - lr2 * m2 / (np.sqrt(v2) + eps), rel=1e-15)
  # train() counts t from 1 and carries (m, v, t) on
  rng = np.random.default_rng(3)
  x = rng.standard_normal((40, 3))
  y = (rng.standard_normal((40, 1)) > 0).astype(np.float64)
  w0 = host_dnn.glorot([3, 4, 1], 0)
  wa, sa, _, _ = hc.train(w0, x, y, 10, 2)
  wb, sb, _, _ = hc.train(w0, x, y, 10, 1)
  wb, sb, _, _ = hc.train(wb, x, y, 10, 1, state=sb[:2], t0=sb[2])
  assert sa[2] == sb[2] == 8
  for u, v_ in zip(wa, wb):
    np.testing.assert_array_equal(u, v_)


MISMATCH_SEED = 0


@pytest.mark.parametrize('n', [100000, 100001, 10, 11])      # the reference's two sizes, and two small ones
def test_mismatch_batch_randomization(n):
  """The properties of the reference's test: shapes, x and a untouched, the first ceil(n / 2) rows matched
  (label 0, x2[0::2]), the rest mismatched (label 1, a shuffle of x2[1::2]); over 100 repetitions fewer than
  150 rows of the shuffled half stay where they were (the reference's bound: the expectation is 100)."""
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(MISMATCH_SEED)
  x = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
  x2 = np.arange(n * 2, dtype=np.float32).reshape(n, 2) + 10
  y = np.full((n, 1), 7, np.float32)
  a = np.arange(n, dtype=np.float32).reshape(n, 1)
  half = (n + 1) // 2
  unmoved = 0
  for _ in range(100):
    nx, nx2, ny, na = brain_data.mismatch_batch_randomization(x, x2, y, a, rng=rng)
    assert nx is x and na is a
    assert nx2.shape == x2.shape and ny.shape == (n, 1)
    np.testing.assert_array_equal(nx2[:half], x2[0::2])
    np.testing.assert_array_equal(ny[:half], 0)
    np.testing.assert_array_equal(ny[half:], 1)
    np.testing.assert_array_equal(np.sort(np.asarray(nx2[half:]), axis=0), x2[1::2])   # a permutation of the odd rows
    unmoved += int(np.sum(np.all(np.asarray(nx2[half:]) == x2[1::2], axis=1)))
  assert unmoved < 150, unmoved
  # a seed is accepted in place of a Generator, and repeats
  p = brain_data.mismatch_batch_randomization(x, x2, y, a, rng=5)[1]
  q = brain_data.mismatch_batch_randomization(x, x2, y, a, rng=5)[1]
  np.testing.assert_array_equal(p, q)
