"""BrainModelDNN without a GPU: the call surface against the reference's (G14), the constructor and compile
errors, the seeded Glorot initialisation, the history the six per-step sums give, the ctypes prototypes of the
td_mlp_* / td_mlpc_* entry points against the C header, and the float64 oracle of tests/host_dnn.py itself
(finite differences, a hand-computed RMSprop step, the shuffle bijection)."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_dnn
from tests.surface import member_rows
from tests.test_cpu_surface import _golden, _leading_matches


def _dataset(c=2, pre=1, post=1, d=1, n=300, batch=50):
  from telluride_decoding_amd import brain_data
  rng = np.random.default_rng(0)
  x = rng.standard_normal((n, c)).astype(np.float32)
  y = rng.standard_normal((n, d)).astype(np.float32)
  z = np.zeros((n, 1), np.float32)
  return brain_data.Dataset([(x, z, y, z)], batch, pre, post)


def test_surface_matches_the_reference():
  from telluride_decoding_amd import brain_model
  ref = _golden()['surface']['brain_model']['BrainModelDNN']
  problems = []
  for name, rows in ref['members'].items():
    assert hasattr(brain_model.BrainModelDNN, name), name
    where = ('brain_model', 'BrainModelDNN', name)
    ours = member_rows(brain_model.BrainModelDNN, name)
    if name == 'compile':        # the optimizer default names a TF class there
      ours = [r if r[0] != 'optimizer' else ['optimizer', r[1], rows[1][2]] for r in ours]
    problems += _leading_matches(rows, ours, where)
  assert not problems, problems


def test_constructor_errors_and_widths():
  from telluride_decoding_amd import brain_model
  ds = _dataset(c=3, pre=2, post=1, d=2)
  with pytest.raises(ValueError, match='Dataset must be a tf.data.datasert'):
    brain_model.BrainModelDNN([1, 2, 3])
  with pytest.raises(TypeError, match='Num_hidden_list must be an list'):
    brain_model.BrainModelDNN(ds, (20, 20))
  m = brain_model.BrainModelDNN(ds, tensorboard_dir='/nonexistent')
  assert [w.shape for w in m.get_weights()] == [(12, 2), (2,)]       # [] = one Dense layer
  m = brain_model.BrainModelDNN(ds, [5, 4])
  assert [w.shape for w in m.get_weights()] == [(12, 5), (5,), (5, 4), (4,), (4, 2), (2,)]


def test_compile_forms_and_errors():
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelDNN(_dataset(), [4])
  m.compile()
  assert isinstance(m.optimizer, brain_model.RMSprop) and m.optimizer.learning_rate == 1e-3
  m.compile(learning_rate=0.01)
  assert m.optimizer.learning_rate == 0.01
  m.compile(optimizer='rmsprop', loss=['mse'], learning_rate=0.02)
  assert m.optimizer.learning_rate == 0.02
  m.compile(optimizer=brain_model.RMSprop(learning_rate=0.03, rho=0.8))
  assert (m.optimizer.learning_rate, m.optimizer.rho) == (0.03, 0.8)
  m.compile(optimizer=lambda learning_rate: brain_model.RMSprop(learning_rate=learning_rate, epsilon=1e-6),
            learning_rate=0.04)
  assert (m.optimizer.learning_rate, m.optimizer.epsilon) == (0.04, 1e-6)
  with pytest.raises(NotImplementedError, match='momentum'):
    m.compile(optimizer=brain_model.RMSprop(momentum=0.9))
  with pytest.raises(NotImplementedError, match='entered'):
    m.compile(optimizer=brain_model.RMSprop(centered=True))
  with pytest.raises(NotImplementedError, match='adam'):
    m.compile(optimizer='adam')
  with pytest.raises(NotImplementedError, match='Optimizer'):
    m.compile(optimizer=lambda learning_rate: object())
  with pytest.raises(NotImplementedError, match='mae'):
    m.compile(loss='mae')
  with pytest.raises(NotImplementedError, match='Loss'):
    m.compile(loss=['mse', 'mse'])
  with pytest.raises(RuntimeError, match='compile'):
    brain_model.BrainModelDNN(_dataset(), [4]).fit(_dataset())


MLP_ENTRY_POINTS = ['td_mlp_train', 'td_mlp_grad', 'td_mlp_train_loss', 'td_mlp_grad_loss', 'td_mlp_forward',
                    'td_mlpc_train', 'td_mlpc_grad', 'td_mlpc_forward']


def _kind_of_ctype(t):
  if t is ctypes.c_void_p or t is ctypes.c_char_p or issubclass(t, ctypes._Pointer):
    return 'pointer'
  return {ctypes.c_int64: 'int64_t', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double'}[t]


def test_argtypes_match_the_header_prototypes():
  """Each of the eight entry points: as many argtypes as the prototype of include/td_hotpath.h has parameters,
  each of the parameter's kind (pointer, int64_t, int, float, double).  A slip here is a silent ABI mismatch."""
  from telluride_decoding_amd import _lib
  with open(_lib.HEADER) as f:
    text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_mlpc?_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == sorted(MLP_ENTRY_POINTS)
  for name in MLP_ENTRY_POINTS:
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), (name, param)
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, (name, kinds)
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name


def test_glorot_initialisation_is_seeded():
  from telluride_decoding_amd import brain_model
  ds = _dataset(c=4, pre=3, post=0)
  a = brain_model.BrainModelDNN(ds, [20, 10], seed=3).get_weights()
  b = brain_model.BrainModelDNN(ds, [20, 10], seed=3).get_weights()
  c = brain_model.BrainModelDNN(ds, [20, 10], seed=4).get_weights()
  widths = [16, 20, 10, 1]
  for i, (fi, fo) in enumerate(zip(widths[:-1], widths[1:])):
    lim = np.sqrt(6.0 / (fi + fo))
    assert a[2 * i].dtype == np.float32 and np.all(np.abs(a[2 * i]) <= lim)
    if fi * fo >= 100:
      assert np.max(np.abs(a[2 * i])) > 0.8 * lim           # uniform over the whole range
    np.testing.assert_array_equal(a[2 * i + 1], 0)
  for u, v in zip(a, b):
    np.testing.assert_array_equal(u, v)
  assert not np.array_equal(a[0], c[0])
  for u, v in zip(a, host_dnn.glorot(widths, 3)):           # the documented recipe
    np.testing.assert_array_equal(u, v)
  m = brain_model.BrainModelDNN(ds, [20, 10])
  m.set_weights(a)
  for u, v in zip(m.weight_matrices, a):
    np.testing.assert_array_equal(u, v)
  with pytest.raises(ValueError):
    m.set_weights(a[:-1])
  with pytest.raises(ValueError):
    m.set_weights([w.T for w in a])


def test_history_from_the_step_sums():
  from telluride_decoding_amd import brain_model
  rng = np.random.default_rng(1)
  rows, d, epochs, steps = 40, 3, 2, 3
  sums = np.zeros((epochs, steps, 6))
  want = {'loss': [], 'pearson_correlation_first': []}
  for e in range(epochs):
    losses, rs = [], []
    for s in range(steps):
      p, y = rng.standard_normal((rows, d)), rng.standard_normal((rows, d))
      if (e, s) == (1, 2):
        p[:, 0] = 0.5                                          # a constant column: r = 0
      sums[e, s] = [p[:, 0].sum(), y[:, 0].sum(), (p[:, 0] ** 2).sum(), (y[:, 0] ** 2).sum(),
                    (p[:, 0] * y[:, 0]).sum(), ((p - y) ** 2).sum()]
      losses.append(np.mean((p - y) ** 2))
      rs.append(host_dnn.pearson_first(p, y))
    want['loss'].append(np.mean(losses))
    want['pearson_correlation_first'].append(np.mean(rs))
  hist = brain_model.History(brain_model.history_from_sums(sums, rows, d)).history
  assert sorted(hist) == ['loss', 'mse', 'pearson_correlation_first']
  assert all(len(v) == epochs for v in hist.values())
  np.testing.assert_allclose(hist['loss'], want['loss'], rtol=1e-12)
  np.testing.assert_allclose(hist['mse'], want['loss'], rtol=1e-12)
  np.testing.assert_allclose(hist['pearson_correlation_first'], want['pearson_correlation_first'], rtol=1e-10)


def test_oracle_gradients_match_finite_differences():
  rng = np.random.default_rng(2)
  widths = [5, 4, 3, 2]
  w = [v.astype(np.float64) for v in host_dnn.glorot(widths, 7)]
  w = [v + 0.1 * rng.standard_normal(v.shape) for v in w]
  x, y = rng.standard_normal((9, 5)), rng.standard_normal((9, 2))
  loss, grads, _, kink = host_dnn.loss_and_grads(w, x, y)
  assert kink > 1e-6
  h = 1e-6
  for t in range(len(w)):
    for idx in np.ndindex(w[t].shape):
      wp = [v.copy() for v in w]
      wm = [v.copy() for v in w]
      wp[t][idx] += h
      wm[t][idx] -= h
      fd = (host_dnn.loss_and_grads(wp, x, y)[0] - host_dnn.loss_and_grads(wm, x, y)[0]) / (2 * h)
      assert abs(fd - grads[t][idx]) <= 1e-7 * max(1.0, abs(fd)), (t, idx)


def test_oracle_rmsprop_by_hand():
  w, v = [np.array([1.0])], [np.array([0.0])]
  w, v = host_dnn.rmsprop(w, v, [np.array([0.5])], lr=0.1, rho=0.9, eps=1e-7)
  v1 = 0.1 * 0.25
  assert v[0][0] == pytest.approx(v1, rel=1e-15)
  assert w[0][0] == pytest.approx(1.0 - 0.1 * 0.5 / (np.sqrt(v1) + 1e-7), rel=1e-15)
  w, v = host_dnn.rmsprop(w, v, [np.array([-0.2])], lr=0.1, rho=0.9, eps=1e-7)
  v2 = 0.9 * v1 + 0.1 * 0.04
  assert v[0][0] == pytest.approx(v2, rel=1e-15)
  assert w[0][0] == pytest.approx(1.0 - 0.1 * 0.5 / (np.sqrt(v1) + 1e-7) + 0.1 * 0.2 / (np.sqrt(v2) + 1e-7),
                                  rel=1e-15)


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 7, 13, 15, 16, 17, 31, 63, 64, 65, 127, 128, 129, 255, 257, 997,
                               1023, 1024, 1025, 4095, 4096, 4097, 65521])
def test_shuffle_is_a_bijection(n):
  for seed, epoch in ((0, 0), (1, 0), (0, 1), (2 ** 40 + 5, 7)):
    perm = host_dnn.permutation(n, seed, epoch)
    np.testing.assert_array_equal(np.sort(perm), np.arange(n))
  if n >= 16:
    assert not np.array_equal(host_dnn.permutation(n, 0, 0), host_dnn.permutation(n, 0, 1))
    assert not np.array_equal(host_dnn.permutation(n, 0, 0), np.arange(n))
