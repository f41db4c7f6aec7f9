"""BrainModelDNN on the MI355X against the float64 restatement of tests/host_dnn.py: the gradients of
td_mlp_grad over a covering grid of shapes, short training trajectories, the reference's own behaviour tests
(test/brain_model_test.py:336-566, data recipes and thresholds unchanged), inference, the decoder's device
path and the limits."""
import numpy as np
import pytest

from tests import host_dnn
from tests import parity_log
from tests.dnn_common import (GRAD_BOUND, KINK, assert_within, flat, grad_distances, iir, make_files, simply_scaled,
                              split)

pytestmark = pytest.mark.gpu

# (hidden, channels, pre, post, batch, outputs, input_offset): every value of each axis next to small and
# large partners
GRID = [
    ([], 1, 0, 0, 2048, 8, 0),
    ([], 128, 31, 32, 512, 1, 1),
    ([20, 20], 64, 15, 21, 128, 1, 1),
    ([20, 20], 2, 0, 2, 2048, 8, 0),
    ([20, 20], 128, 0, 0, 512, 2, -1),
    ([40, 20, 10], 2, 1, 1, 2048, 2, -1),
    ([40, 20, 10], 64, 31, 32, 128, 2, 1),
    ([64] * 4, 1, 31, 32, 512, 2, -1),
    ([64] * 4, 64, 15, 21, 128, 8, 0),
]


def _grad_case(hidden, c, pre, post, batch, d, off, mixup=False):
  from telluride_decoding_amd import brain_data, device
  h = device.default_handle()
  k = c * (pre + 1 + post)
  widths = [k] + hidden + [d]
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
    loss, g64, _, kink = host_dnn.loss_and_grads(weights, x64, y64)
    if kink >= KINK:
      break
  else:
    pytest.fail('no seed keeps the ReLU inputs %g away from their kinks' % KINK)
  res = ds.resolved()
  x, _, y, offs = res.device_arrays(h)
  params = h.to_device(flat(weights))
  grad, sums = device.mlp_grad(x, y, offs, pre, post, hidden, params, batch, s, input_offset=off,
                               rows_used=res.rows_used(), handle=h)
  dists = grad_distances(split(grad.cpu().numpy(), widths), g64)
  worst = max(dists.values())
  assert_within(dists, GRAD_BOUND)
  s6 = sums.cpu().numpy()
  assert abs(s6[5] / (batch * d) - loss) <= 1e-6 * loss
  return worst, kink


@pytest.mark.parametrize('case', GRID, ids=lambda c: '%s-c%d-l%d-B%d-D%d-o%d' % (
    'x'.join(map(str, c[0])) or 'none', c[1], c[2] + c[3] + 1, c[4], c[5], c[6]))
def test_gradients_match_float64(case):
  worst, kink = _grad_case(*case)
  parity_log.record('dnn_grad', shape=str(case), rel=worst, kink=kink)


def test_gradients_of_a_mixup_batch_dataset():
  worst, kink = _grad_case([20, 20], 4, 2, 2, 128, 1, 0, mixup=True)
  parity_log.record('dnn_grad_mixup', rel=worst, kink=kink)


def _trajectory(shuffle_seed):
  from telluride_decoding_amd import brain_data, brain_model
  c, pre, post, d, batch, hidden = 4, 2, 1, 2, 32, [8, 4]
  k = c * (pre + 1 + post)
  widths = [k] + hidden + [d]
  for seed in range(8):
    rng = np.random.default_rng(50 + seed)
    files = make_files(rng, [101, 130, 95], c, d)
    ds = brain_data.Dataset(files, batch, pre, post)
    x64, y64 = host_dnn.stream(files, batch, pre, post)
    w0 = host_dnn.glorot(widths, seed)
    w64, _, hist64, kink = host_dnn.train(w0, x64, y64, batch, 3, 1e-3, shuffle_seed=shuffle_seed)
    if kink >= 1e-5:
      break
  else:
    pytest.fail('no seed keeps the trajectory away from the ReLU kinks')
  runs = []
  for _ in range(2):
    m = brain_model.BrainModelDNN(ds, hidden, seed=seed)
    m.compile()
    hist = m.fit(ds, epochs=3, shuffle_seed=shuffle_seed).history
    runs.append((m.get_weights(), hist))
  for a, b in zip(runs[0][0], runs[1][0]):
    np.testing.assert_array_equal(a, b)                      # bitwise reproducible
  assert runs[0][1] == runs[1][1]
  wmax = max(float(np.max(np.abs(b))) for b in w64)
  wdist = max(float(np.max(np.abs(a - b))) for a, b in zip(runs[0][0], w64)) / wmax
  assert wdist <= 1e-4, wdist
  hdist = 0.0
  for key in ('loss', 'pearson_correlation_first', 'mse'):
    got, want = np.asarray(runs[0][1][key]), np.asarray(hist64[key])
    assert got.shape == (3,)
    # (a correlation's scale is 1: near r = 0 its relative error is not meaningful)
    scale = np.maximum(np.abs(want), 1.0) if key == 'pearson_correlation_first' else np.abs(want)
    hdist = max(hdist, float(np.max(np.abs(got - want) / scale)))
  assert hdist <= 1e-5, hdist
  parity_log.record('dnn_trajectory', shuffle=str(shuffle_seed), weights=wdist, history=hdist, kink=kink)


def test_trajectory_in_order():
  _trajectory(None)


def test_trajectory_shuffled():
  _trajectory(12345)


# ---- the reference's behaviour tests (test/brain_model_test.py), recipes and thresholds unchanged ----------
def _fit_dnn(ds, hidden, epochs):
  from telluride_decoding_amd import brain_model
  m = brain_model.BrainModelDNN(ds, hidden)
  m.compile(optimizer=brain_model.RMSprop(learning_rate=1e-3), loss=['mse'],
            metrics=[brain_model.pearson_correlation_first])
  hist = m.fit(ds, epochs=epochs)
  return m, hist, m.evaluate(ds)


def test_regression_fullyconnected():          # brain_model_test.py:336-357
  from telluride_decoding_amd import brain_model
  ds = simply_scaled()
  _, hist, metrics = _fit_dnn(ds, [40, 20, 10], 100)
  assert len(hist.history['loss']) == 100 and np.all(np.isfinite(hist.history['loss']))
  assert metrics['loss'] < 0.35
  assert metrics['pearson_correlation_first'] > 0.85
  lin = brain_model.BrainModelLinearRegression(ds)
  lin.fit(ds)
  assert lin.evaluate(ds)['pearson_correlation_first'] < 0.1      # what the linear path cannot learn
  parity_log.record('dnn_ref_sin', **metrics)


@pytest.mark.parametrize('offset,r_min', [(1, 0.9), (-1, 0.88)])
def test_offset_regression(offset, r_min):     # :360-492
  ds = simply_scaled(data_offset=offset, channels=1, pre=1, post=1, batch=128)
  _, _, metrics = _fit_dnn(ds, [40, 20, 10], 100)
  assert metrics['loss'] < 0.4
  assert metrics['pearson_correlation_first'] > r_min
  parity_log.record('dnn_ref_offset', offset=offset, **metrics)


def test_simple_iir_regression():              # :505-566
  _, _, m32 = _fit_dnn(iir(32), [40, 20, 10], 10)
  assert m32['loss'] < 0.025
  assert m32['pearson_correlation_first'] > 0.95
  _, _, m0 = _fit_dnn(iir(0), [40, 20, 10], 10)
  assert m0['loss'] > 0.025
  assert m0['pearson_correlation_first'] > 0.8
  parity_log.record('dnn_ref_iir', loss32=m32['loss'], r32=m32['pearson_correlation_first'], loss0=m0['loss'],
                    r0=m0['pearson_correlation_first'])


# ---- inference ------------------------------------------------------------------------------------------
def test_inference_matches_float64():
  from oracle import lag as o_lag
  from telluride_decoding_amd import brain_data, brain_model
  rng = np.random.default_rng(7)
  c, pre, post, d, batch, hidden, off = 6, 3, 2, 2, 64, [16, 8], 1
  files = make_files(rng, [300, 5000, 170], c, d)
  ds = brain_data.Dataset(files, batch, pre, post, input_offset=off)
  m = brain_model.BrainModelDNN(ds, hidden, seed=1)
  w = m.get_weights()
  pred = m.predict(ds)
  want = np.concatenate([host_dnn.forward(w, o_lag.window_streams(*f, pre=pre, post=post,
                                                                  input_offset=off)[0])[0] for f in files])
  want = brain_model.rows_of_stream(want, ds.zipped_lengths(), ds.rows_used())
  assert pred.shape == want.shape
  dist = float(np.max(np.abs(pred - want)) / np.max(np.abs(want)))
  assert dist <= 1e-5, dist
  # call() on lagged minibatches = the matching rows of predict
  batches = list(ds)
  for s in (0, 3, len(batches) - 1):
    got = m(batches[s][0])
    np.testing.assert_allclose(got, pred[s * batch:(s + 1) * batch], rtol=0, atol=1e-5 * np.max(np.abs(want)))
  # evaluate = the float64 per-minibatch means
  losses, rs = [], []
  for feats, y in batches:
    p = host_dnn.forward(w, np.asarray(feats['input_1'], np.float64))[0]
    losses.append(np.mean((p - y) ** 2))
    rs.append(host_dnn.pearson_first(p, np.asarray(y, np.float64)))
  ev = m.evaluate(ds)
  assert abs(ev['loss'] - np.mean(losses)) <= 1e-5 * np.mean(losses)
  assert ev['mse'] == ev['loss']
  assert abs(ev['pearson_correlation_first'] - np.mean(rs)) <= 1e-5
  ev_it = m.evaluate(batches)                                  # the iterable route
  assert abs(ev_it['loss'] - ev['loss']) <= 1e-5 * ev['loss']
  parity_log.record('dnn_forward', rel=dist)
  # an iterable of minibatches trains like the Dataset it stands for
  a = brain_model.BrainModelDNN(ds, hidden, seed=2)
  b = brain_model.BrainModelDNN(ds, hidden, seed=2)
  a.compile()
  b.compile()
  zeros = np.zeros((len(batches) * batch, 1), np.float32)
  lagged = brain_data.Dataset([(np.concatenate([f['input_1'] for f, _ in batches]), zeros,
                                np.concatenate([y for _, y in batches]), zeros)], batch)
  ha = a.fit(batches, epochs=2).history
  hb = b.fit(lagged, epochs=2).history
  assert ha == hb


# ---- the decoder's device path ---------------------------------------------------------------------------
def test_decoder_runs_on_the_device(monkeypatch):
  from telluride_decoding_amd import brain_data, brain_model, infer_decoder, synth
  trials = synth.make_trials(4, 3, 1200, 8, switch_half=True)
  files = []
  for eeg, env, att in trials:
    attended = np.where(att > 0.5, env[:, 1:2], env[:, 0:1]).astype(np.float32)
    files.append((eeg, env, attended, att))
  train = brain_data.Dataset(files, 100, 0, 3)
  mixed = brain_data.Dataset(files, 100, 0, 3, mixup_batch=True, mixup_seed=1)
  model = brain_model.BrainModelDNN(train, [8], seed=0)
  model.compile(learning_rate=1e-2)
  model.fit(train, epochs=3)

  def fail(*args, **kwargs):
    raise AssertionError('decode_one called')
  fast = infer_decoder.create_decoder('fullyconnected', reduction='first', model=model)
  assert isinstance(fast, infer_decoder.LinearRegressionDecoder)
  with monkeypatch.context() as mp:
    mp.setattr(infer_decoder.LinearRegressionDecoder, 'decode_one', fail)
    d_fast = fast.train(mixed, train)
    s_fast, l_fast = fast.test_all(train)
  slow = infer_decoder.create_decoder('fullyconnected', reduction='first', model=model)
  with monkeypatch.context() as mp:
    mp.setattr(infer_decoder.LinearRegressionDecoder, '_decode_dataset_device', lambda self, data, h: None)
    d_slow = slow.train(mixed, train)
    s_slow, l_slow = slow.test_all(train)
  np.testing.assert_allclose(d_fast, d_slow, rtol=1e-5)
  np.testing.assert_allclose(s_fast, s_slow, rtol=1e-5, atol=1e-5)
  np.testing.assert_array_equal(l_fast, l_slow)
  assert fast._model_inputs == {'input_1': (None, model._input_width)}


# ---- limits -----------------------------------------------------------------------------------------------
def test_limits_raise_before_any_launch():
  from telluride_decoding_amd import brain_data, brain_model, device
  h = device.default_handle()
  rng = np.random.default_rng(3)

  def ds_of(c, pre, post, d, batch, n=4200):
    return brain_data.Dataset(make_files(rng, [n], c, d), batch, pre, post)
  cases = [(ds_of(129, 1, 0, 1, 64), [4]), (ds_of(2, 32, 32, 1, 64), [4]), (ds_of(2, 0, 0, 9, 64), [4]),
           (ds_of(2, 0, 0, 1, 2049), [4]), (ds_of(2, 0, 0, 1, 64), [4] * 5), (ds_of(2, 0, 0, 1, 64), [65])]
  for ds, hidden in cases:
    m = brain_model.BrainModelDNN(ds, hidden)
    m.compile()
    before = m.get_weights()
    with pytest.raises(ValueError):
      m.fit(ds)
    for a, b in zip(before, m.get_weights()):
      np.testing.assert_array_equal(a, b)
  # the C entry point itself refuses the same shapes (nothing queued: the parameters stay as they were)
  ds = ds_of(2, 0, 0, 1, 64)
  x, _, y, offs = ds.device_arrays(h)
  params = h.to_device(np.ones(2 * 65 + 65 + 65 + 1, np.float32))
  state = h.zeros((int(params.numel()),))
  with pytest.raises(ValueError, match='hidden layer'):
    device.mlp_train(x, y, offs, 0, 0, [65], params, state, 64, 1, 1e-3, 0.9, 1e-7, handle=h)
  assert float(params.sum()) == float(params.numel())
  with pytest.raises(ValueError, match='batch'):
    device.mlp_train(x, y, offs, 0, 0, [4], params, state, 2049, 1, 1e-3, 0.9, 1e-7, handle=h)


def test_codelab_shape_trains():
  """64 channels, pre 15 / post 21 (K = 2368), [20, 20], B = 512, 40 recordings x 6000 frames: 100 epochs."""
  from telluride_decoding_amd import brain_data, brain_model
  rng = np.random.default_rng(11)
  files = []
  for _ in range(40):
    x = rng.standard_normal((6000, 64)).astype(np.float32)
    y = (0.1 * x[:, :4].sum(axis=1, keepdims=True)).astype(np.float32)
    z = np.zeros((6000, 1), np.float32)
    files.append((x, z, y, z))
  ds = brain_data.Dataset(files, 512, 15, 21)
  assert ds.num_batches() == 468
  m = brain_model.BrainModelDNN(ds, [20, 20])
  m.compile()
  hist = m.fit(ds, epochs=100, shuffle_seed=1).history
  assert len(hist['loss']) == 100 and np.all(np.isfinite(hist['loss']))
  assert hist['loss'][-1] < hist['loss'][0]
  assert all(np.all(np.isfinite(w)) for w in m.get_weights())
