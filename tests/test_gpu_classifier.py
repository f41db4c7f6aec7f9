"""BrainModelClassifier on the MI355X against the float64 restatement of tests/host_classifier.py: the gradients of
td_mlpc_grad over a covering grid of shapes, one Adam step in isolation, short training trajectories, optimizer
state and determinism, inference and evaluation, the reference's own behaviour test
(test/brain_model_test.py:813-849, recipe and threshold unchanged) and the limits.

Every case is built on the host first (`*_case` below, no GPU needed) and redrawn with another seed, at most
MAX_DRAWS times, while in float64 a hidden pre-activation or an output logit lies within MARGIN of 0 relative to
its sum of |terms|: a ReLU branch or a 0.5 decision that float32 rounding could flip is never absorbed by a
looser bound, and with the rule in force the count of correct entries must equal float64's exactly."""
import numpy as np
import pytest

from tests import host_classifier as hc
from tests import host_dnn
from tests import parity_log
from tests.dnn_common import GRAD_BOUND, assert_within, flat, grad_distances, make_files, split, tensor_names

pytestmark = pytest.mark.gpu

MARGIN = 1e-6        # gradients, inference, evaluation
MARGIN_TRAJ = 1e-5   # trajectories
MAX_DRAWS = 3
LOSS_BOUND = 1e-5   # a step's loss against float64, relative: the bound of the history's loss, saturated case included
EPS32 = 2.0 ** -24   # half an ulp of a float32 in [1, 2): the relative error of one rounding


def _counts(accuracies, entries):
  """Mean accuracies over `entries` entries as the counts of correct entries they stand for."""
  counts = [a * entries for a in accuracies]
  assert all(abs(c - round(c)) < 1e-6 for c in counts), counts
  return [int(round(c)) for c in counts]


def _x64(feats):
  return np.concatenate([np.asarray(feats['input_1'], np.float64), np.asarray(feats['input_2'], np.float64)], axis=1)


# (hidden, c1, pre, post, c2, pre2, post2, batch, outputs, input_offset).  The slab kernel cuts W1's K1 + K2 rows
# into slices of ks = min(64, 4 ceil(ceil(K / 64) / 4)) rows; "straddle": K1 is no multiple of ks, so one slice
# gathers from both views.
GRID = [
    ([], 1, 0, 0, 1, 0, 0, 2048, 8, 0),               # K = 2: one slice holds both views
    ([20], 64, 15, 21, 1, 15, 21, 512, 1, 0),         # the match-mismatch shape; ks = 40, K1 = 2368: straddle
    ([], 120, 31, 32, 8, 31, 32, 512, 1, 1),          # K1 + K2 = 7680 + 512 = 8192
    ([20, 20], 128, 0, 0, 128, 0, 2, 128, 2, -1),
    ([64] * 4, 2, 1, 1, 128, 0, 0, 128, 2, -1),       # ks = 4, K1 = 6: straddle
    ([64] * 4, 64, 15, 21, 2, 31, 32, 128, 8, 1),     # ks = 40, K1 = 2368: straddle; 64 lags of input_2
    ([20], 1, 31, 32, 1, 0, 0, 2048, 2, 1),
    ([20, 20], 3, 2, 2, 5, 1, 3, 128, 1, 0),          # ks = 4, K1 = 15: straddle
]


def grad_case(hidden, c, pre, post, c2, pre2, post2, batch, d, off, mixup=False, logit_scale=None):
  """Host only: the dataset, the tested minibatch (the one across the first file boundary), the weights and the
  float64 results of an accepted draw.  logit_scale: the output layer is rescaled so max|z| is that."""
  from telluride_decoding_amd import brain_data
  widths = [c * (pre + 1 + post) + c2 * (pre2 + 1 + post2)] + hidden + [d]
  for seed in range(MAX_DRAWS):
    rng = np.random.default_rng(2000 + seed)
    lengths = [int(batch * f) + 7 for f in (0.6, 1.3, 0.45, 1.9)]          # ragged files
    files = make_files(rng, lengths, c, d, c2=c2)
    ds = brain_data.Dataset(files, batch, pre, post, pre2, post2, input_offset=off, mixup_batch=mixup,
                            mixup_seed=seed)
    batches = list(ds)
    first = max(lengths[0] - abs(off), 0)
    s = min(first // batch, len(batches) - 1)
    assert s * batch < first < (s + 1) * batch                             # across the file boundary
    weights = host_dnn.glorot(widths, seed)
    weights = [w + np.float32(0.05) * rng.standard_normal(w.shape).astype(np.float32) for w in weights]
    x64, y64 = _x64(batches[s][0]), np.asarray(batches[s][1], np.float64)
    if logit_scale is not None:
      z = hc.forward(weights, x64)[0]
      f = np.float32(logit_scale / np.max(np.abs(z)))
      weights[-2], weights[-1] = weights[-2] * f, weights[-1] * f
    loss, g64, z, margin, ok = hc.loss_and_grads(weights, x64, y64)
    if margin >= MARGIN:
      return dict(ds=ds, s=s, weights=weights, widths=widths, loss=loss, g64=g64, z=z, margin=margin, ok=ok,
                  draws=seed + 1)
  pytest.fail('no draw in %d keeps the ReLU inputs and the logits %g away from 0' % (MAX_DRAWS, MARGIN))


def _run_grad(case, hidden, batch, d, off):
  from telluride_decoding_amd import device
  h = device.default_handle()
  res = case['ds'].resolved()
  x, x2, y, offs = res.device_arrays(h)
  params = h.to_device(flat(case['weights']))
  grad, sums = device.mlpc_grad(x, x2, y, offs, res.pre, res.post, res.pre2, res.post2, hidden, params, batch,
                                case['s'], input_offset=off, rows_used=res.rows_used(), handle=h)
  s6 = sums.cpu().numpy()
  dists = grad_distances(split(grad.cpu().numpy(), case['widths']), case['g64'])
  loss32 = s6[5] / (batch * d)
  loss_rel = abs(loss32 - case['loss']) / case['loss']
  print('classifier grad', hidden, dists, 'loss rel', loss_rel, 'correct', s6[0], case['ok'], 'margin', case['margin'])
  assert_within(dists, GRAD_BOUND)
  assert np.isfinite(loss32)
  assert list(s6[1:5]) == [0.0] * 4
  assert s6[0] == case['ok']                           # exact under the redraw rule
  return max(dists.values()), loss_rel


def _id(c):
  return '%s-c%d-l%d-c2_%d-l2_%d-B%d-D%d-o%d' % ('x'.join(map(str, c[0])) or 'none', c[1], c[2] + c[3] + 1, c[4],
                                                  c[5] + c[6] + 1, c[7], c[8], c[9])


@pytest.mark.parametrize('shape', GRID, ids=_id)
def test_gradients_match_float64(shape):
  case = grad_case(*shape)
  worst, loss_rel = _run_grad(case, shape[0], shape[7], shape[8], shape[9])
  assert loss_rel <= LOSS_BOUND
  parity_log.record('classifier_grad', shape=str(shape), rel=worst, loss_rel=loss_rel, margin=case['margin'],
                    draws=case['draws'])


def test_gradients_of_a_mixup_batch_dataset():
  shape = ([20, 20], 4, 2, 2, 2, 1, 1, 128, 1, 0)
  case = grad_case(*shape, mixup=True)
  worst, loss_rel = _run_grad(case, shape[0], shape[7], shape[8], shape[9])
  assert loss_rel <= LOSS_BOUND
  parity_log.record('classifier_grad_mixup', rel=worst, loss_rel=loss_rel, margin=case['margin'])


def test_gradients_with_saturated_logits():
  """|z| up to 30: sigma(z) rounds to 0 or 1 in float32 and the clipped-probability form of the loss would
  differ; the logit form stays finite and close to float64."""
  shape = ([20], 4, 2, 2, 2, 1, 1, 128, 2, 0)
  case = grad_case(*shape, logit_scale=30.0)
  assert 29.0 <= np.max(np.abs(case['z'])) <= 31.0
  worst, loss_rel = _run_grad(case, shape[0], shape[7], shape[8], shape[9])
  assert loss_rel <= LOSS_BOUND
  parity_log.record('classifier_grad_saturated', rel=worst, loss_rel=loss_rel, margin=case['margin'])


# ---- one Adam step in isolation -----------------------------------------------------------------------------
@pytest.mark.parametrize('lr', [1e-3, 1e-1])
def test_one_adam_step_from_the_devices_own_gradient(lr):
  """td_mlpc_train's update against float64 Adam applied on the host to the DEVICE's float32 gradient, from
  nonzero m, v and step0: the optimizer's arithmetic apart from the gradient's rounding.

  The bound, per weight, from the float32 format alone (e = 2^-24, one rounding).  With M = b1 |m| + (1 - b1) |g|
  (the size of m's two terms), m' and v' the new accumulators and U = lr_t M / (sqrt(v') + eps) >= |update|:
    m' = fl(fl(b1) m) + fl(fl(1 - b1) g): two roundings per term and one for the sum     |dm'| <= 3 e M
    v' the same plus the rounding of g g, all terms positive                              |dv'| <= 4 e v'
    sqrt (half of v's error, one rounding), + fl(eps), the rounded lr_t, the product and the quotient:
                                                                              |d update| <= e (3 U + 7.5 |update|)
    w' = fl(w - update): half an ulp of the stored weight                                 <= e |w'|
  so |w' - w'_64| <= e (|w'| + 11 U).  With m, v drawn as below U <= lr, and the optimizer's own share, 11 e U, is
  6.6e-7 lr; the rest is the rounding any float32 weight carries."""
  from telluride_decoding_amd import brain_data, device
  h = device.default_handle()
  hidden, c, pre, post, c2, pre2, post2, batch, d = [20], 4, 2, 2, 2, 1, 1, 128, 1
  b1, b2, eps, step0 = 0.9, 0.999, 1e-7, 7
  rng = np.random.default_rng(77)
  files = make_files(rng, [150], c, d, c2=c2)
  ds = brain_data.Dataset(files, batch, pre, post, pre2, post2).take(1)          # one step
  widths = [c * (pre + 1 + post) + c2 * (pre2 + 1 + post2)] + hidden + [d]
  w0 = flat(host_dnn.glorot(widths, 1))
  w0[w0 == 0] = np.float32(0.01)                                                   # (the zero biases)
  x, x2, y, offs = ds.device_arrays(h)
  params = h.to_device(w0)
  grad, _ = device.mlpc_grad(x, x2, y, offs, pre, post, pre2, post2, hidden, params, batch, 0,
                             rows_used=ds.rows_used(), handle=h)
  g = grad.cpu().numpy().astype(np.float64)
  gs = np.sqrt(np.mean(g ** 2))
  m0 = (gs * rng.standard_normal(g.shape)).astype(np.float32)
  v0 = (2.0 * gs ** 2 * (0.5 + rng.random(g.shape))).astype(np.float32)           # v >~ m^2, g^2: updates <~ lr
  state = h.to_device(np.concatenate([m0, v0]))
  device.mlpc_train(x, x2, y, offs, pre, post, pre2, post2, hidden, params, state, batch, 1, lr, b1, b2, eps,
                    step0=step0, rows_used=ds.rows_used(), handle=h)
  w_new, st = params.cpu().numpy(), state.cpu().numpy()
  (w64,), (m64,), (v64,) = hc.adam([w0.astype(np.float64)], [m0.astype(np.float64)], [v0.astype(np.float64)], [g],
                                   step0 + 1, lr, b1, b2, eps)
  lr_t = lr * np.sqrt(1 - b2 ** (step0 + 1)) / (1 - b1 ** (step0 + 1))
  big_m = b1 * np.abs(m0.astype(np.float64)) + (1 - b1) * np.abs(g)
  big_u = lr_t * big_m / (np.sqrt(v64) + eps)
  assert np.max(big_u) <= 2 * lr                         # the premise "an update of size <= lr" (lr_t / lr = 0.16)
  assert np.all(np.abs(st[:g.size] - m64) <= 3 * EPS32 * big_m)
  assert np.all(np.abs(st[g.size:] - v64) <= 4 * EPS32 * v64)
  err = np.abs(w_new - w64)
  bound = EPS32 * (np.abs(w64) + 11 * big_u)
  worst = float(np.max(err / bound))
  opt_share = float(np.max(np.maximum(err - EPS32 * np.abs(w64), 0)) / lr)
  print('adam step lr', lr, 'max err / bound', worst, 'beyond the weight rounding, in lr', opt_share,
        'max err / lr', float(np.max(err)) / lr)
  assert worst <= 1.0, worst
  assert np.any(w_new != w0)
  parity_log.record('classifier_adam_step', lr=lr, err_over_bound=worst, err_over_lr=float(np.max(err)) / lr,
                    beyond_weight_rounding_over_lr=opt_share)


# ---- trajectories ---------------------------------------------------------------------------------------------
TRAJ = dict(c=4, pre=2, post=1, c2=2, pre2=1, post2=2, d=2, batch=32, hidden=[8, 4], lengths=[101, 130, 95])


def trajectory_case(shuffle_seed, epochs=3):
  """Host only: an accepted draw of 3 epochs x 10 steps."""
  t = TRAJ
  widths = [t['c'] * (t['pre'] + 1 + t['post']) + t['c2'] * (t['pre2'] + 1 + t['post2'])] + t['hidden'] + [t['d']]
  for seed in range(MAX_DRAWS):
    rng = np.random.default_rng(60 + seed)
    files = make_files(rng, t['lengths'], t['c'], t['d'], c2=t['c2'])
    x64, y64 = hc.stream(files, t['batch'], t['pre'], t['post'], t['pre2'], t['post2'])
    assert x64.shape[0] == 10 * t['batch']
    w0 = host_dnn.glorot(widths, seed)
    w64, _, hist64, margin = hc.train(w0, x64, y64, t['batch'], epochs, shuffle_seed=shuffle_seed)
    if margin >= MARGIN_TRAJ:
      return dict(files=files, seed=seed, w64=w64, hist64=hist64, margin=margin, draws=seed + 1)
  pytest.fail('no draw in %d keeps the trajectory %g away from the kinks and the threshold' % (MAX_DRAWS, MARGIN_TRAJ))


def _dataset_of(case):
  from telluride_decoding_amd import brain_data
  t = TRAJ
  return brain_data.Dataset(case['files'], t['batch'], t['pre'], t['post'], t['pre2'], t['post2'])


def _trajectory(shuffle_seed):
  from telluride_decoding_amd import brain_model
  case = trajectory_case(shuffle_seed)
  ds = _dataset_of(case)
  runs = []
  for _ in range(2):
    m = brain_model.BrainModelClassifier(ds, TRAJ['hidden'], seed=case['seed'])
    m.compile()
    hist = m.fit(ds, epochs=3, shuffle_seed=shuffle_seed).history
    runs.append((m.get_weights(), hist))
  for a, b in zip(runs[0][0], runs[1][0]):
    np.testing.assert_array_equal(a, b)                      # two identical fits: bitwise
  assert runs[0][1] == runs[1][1]
  w64 = case['w64']
  wmax = max(float(np.max(np.abs(b))) for b in w64)
  per_tensor = {n: float(np.max(np.abs(a - b))) / wmax for n, a, b in zip(tensor_names(len(w64)), runs[0][0], w64)}
  got, want = runs[0][1], case['hist64']
  assert sorted(got) == ['accuracy', 'loss'] and len(got['loss']) == 3
  hdist = float(np.max(np.abs(np.asarray(got['loss']) - want['loss']) / np.abs(want['loss'])))
  print('classifier trajectory', shuffle_seed, per_tensor, 'loss rel', hdist, 'margin', case['margin'])
  wdist = max(per_tensor.values())
  assert wdist <= 1e-4, per_tensor
  assert hdist <= 1e-5, hdist
  entries = 10 * TRAJ['batch'] * TRAJ['d']                 # the history's accuracy as a count: exact
  assert _counts(got['accuracy'], entries) == _counts(want['accuracy'], entries)
  parity_log.record('classifier_trajectory', shuffle=str(shuffle_seed), weights=wdist, history=hdist,
                    margin=case['margin'], draws=case['draws'])


def test_trajectory_in_order():
  _trajectory(None)


def test_trajectory_shuffled():
  _trajectory(12345)


# ---- state and determinism ------------------------------------------------------------------------------------
def test_adam_state_carries_across_fits_and_compile_resets_it():
  from telluride_decoding_amd import brain_model
  case = trajectory_case(None)
  ds = _dataset_of(case)

  def model():
    m = brain_model.BrainModelClassifier(ds, TRAJ['hidden'], seed=case['seed'])
    m.compile()
    return m
  whole = model()
  h4 = whole.fit(ds, epochs=4).history
  halves = model()
  h2a = halves.fit(ds, epochs=2).history
  h2b = halves.fit(ds, epochs=2).history
  for a, b in zip(whole.get_weights(), halves.get_weights()):
    np.testing.assert_array_equal(a, b)                      # t, m and v carried over: bitwise
  assert h4['loss'] == h2a['loss'] + h2b['loss'] and h4['accuracy'] == h2a['accuracy'] + h2b['accuracy']
  assert halves._updates == 40
  reset = model()
  reset.fit(ds, epochs=2)
  reset.compile()
  assert reset._updates == 0 and reset._state is None
  reset.fit(ds, epochs=2)
  assert any(not np.array_equal(a, b) for a, b in zip(whole.get_weights(), reset.get_weights()))


# ---- inference and evaluation -----------------------------------------------------------------------------------
def inference_case():
  """Host only: files, weights and float64 results of an accepted draw."""
  from oracle import lag as o_lag
  from telluride_decoding_amd import brain_data
  c, pre, post, c2, pre2, post2, d, batch, hidden, off = 6, 3, 2, 3, 1, 2, 2, 64, [16, 8], -1
  widths = [c * (pre + 1 + post) + c2 * (pre2 + 1 + post2)] + hidden + [d]
  for seed in range(MAX_DRAWS):
    rng = np.random.default_rng(7 + seed)
    files = make_files(rng, [300, 5000, 170], c, d, c2=c2)
    w = host_dnn.glorot(widths, seed + 1)
    w = [a + np.float32(0.05) * rng.standard_normal(a.shape).astype(np.float32) for a in w]
    parts, margin = [], np.inf
    for f in files:
      x1, x2l = o_lag.window_streams(*f, pre=pre, post=post, pre2=pre2, post2=post2, input_offset=off)[:2]
      z, _, _, mg = hc.forward(w, np.concatenate([x1, x2l], axis=1).astype(np.float64))
      parts.append(hc.sigmoid(z))
      margin = min(margin, mg)
    if margin >= MARGIN:
      ds = brain_data.Dataset(files, batch, pre, post, pre2, post2, input_offset=off)
      x64, y64 = hc.stream(files, batch, pre, post, pre2, post2, off)
      ev64, _ = hc.evaluate(w, x64, y64, batch)
      return dict(ds=ds, hidden=hidden, w=w, probs=np.concatenate(parts), ev64=ev64, margin=margin, batch=batch)
  pytest.fail('no draw in %d keeps the logits %g away from 0' % (MAX_DRAWS, MARGIN))


def test_inference_and_evaluate_match_float64():
  from telluride_decoding_amd import brain_model
  case = inference_case()
  ds, batch = case['ds'], case['batch']
  m = brain_model.BrainModelClassifier(ds, case['hidden'])
  m.set_weights(case['w'])
  m.compile()
  pred = m.predict(ds)
  want = brain_model.rows_of_stream(case['probs'], ds.zipped_lengths(), ds.rows_used())
  assert pred.shape == want.shape
  dist = float(np.max(np.abs(pred - want)))
  assert dist <= 1e-5, dist
  assert np.all((pred >= 0) & (pred <= 1))
  batches = list(ds)
  cdist = 0.0
  for s in (0, 4, len(batches) - 1):                      # call() on lagged minibatches = the matching rows
    got = np.asarray(m(batches[s][0]))
    cdist = max(cdist, float(np.max(np.abs(got - want[s * batch:(s + 1) * batch]))))
  assert cdist <= 1e-5, cdist
  ev = m.evaluate(ds)
  assert sorted(ev) == ['accuracy', 'loss']
  loss_rel = abs(ev['loss'] - case['ev64']['loss']) / case['ev64']['loss']
  print('classifier inference', dist, cdist, 'evaluate loss rel', loss_rel, ev, case['ev64'])
  assert loss_rel <= 1e-5, loss_rel
  entries = ds.num_batches() * batch * ds.d
  assert _counts([ev['accuracy']], entries) == _counts([case['ev64']['accuracy']], entries)
  ev_it = m.evaluate(batches)                               # the iterable route: same minibatches
  assert abs(ev_it['loss'] - ev['loss']) <= 1e-6 * ev['loss'] and ev_it['accuracy'] == ev['accuracy']
  for a, b in zip(m.get_weights(), case['w']):
    np.testing.assert_array_equal(a, b)                     # evaluate updates nothing
  # an iterable of minibatches trains like the Dataset it stands for
  a = brain_model.BrainModelClassifier(ds, case['hidden'], seed=2)
  b = brain_model.BrainModelClassifier(ds, case['hidden'], seed=2)
  a.compile()
  b.compile()
  assert a.fit(batches, epochs=2).history == b.fit(ds, epochs=2).history
  parity_log.record('classifier_forward', abs=dist, call_abs=cdist, evaluate_loss_rel=loss_rel,
                    margin=case['margin'])


# ---- the reference's behaviour test (test/brain_model_test.py:813-849), recipe and threshold unchanged ---------
def test_dnn_classifier():
  from telluride_decoding_amd import brain_data, brain_model
  rs = np.random.RandomState(0)
  num_samples, num_dim = 1000, 3
  input1 = rs.randn(num_samples, num_dim).astype(np.float32)
  output = (rs.randn(num_samples, 1) > 0.5).astype(np.float32)
  input2 = rs.randn(num_samples, num_dim - 1).astype(np.float32)
  input2 = output * 2 * input1[:, :-1] + (1 - output) * input2
  bd = brain_data.TestBrainData('input', 'output', 100.0, final_batch_size=128)
  bd.preserve_test_data(input_data=input1, input2_data=input2, output_data=output)
  ds = bd.create_dataset('train')
  ib, _ = list(ds.take(1))[0]
  model = brain_model.BrainModelClassifier(ds, num_hidden_list=[20])
  out = model(ib)
  assert out.shape == (128, 1) and np.all((out > 0) & (out < 1))
  model.compile(optimizer='adam', loss=brain_model.BinaryCrossentropy(), metrics=['accuracy'])
  hist = model.fit(ds, epochs=100).history
  assert len(hist['loss']) == 100 and np.all(np.isfinite(hist['loss']))
  metrics = model.evaluate(ds)
  print('classifier reference test', metrics)
  assert metrics['accuracy'] > 0.90
  parity_log.record('classifier_ref_match_mismatch', **metrics)


# ---- limits ---------------------------------------------------------------------------------------------------------
def test_limits_raise_before_any_launch():
  from telluride_decoding_amd import brain_data, brain_model, device
  h = device.default_handle()
  rng = np.random.default_rng(3)

  def ds_of(c, pre, post, c2, pre2, post2, d, batch, n=4200):
    return brain_data.Dataset(make_files(rng, [n], c, d, c2=c2), batch, pre, post, pre2, post2)
  cases = [
      (ds_of(128, 31, 31, 3, 21, 21, 1, 64), [4]),          # K1 + K2 = 8064 + 129 = 8193
      (ds_of(2, 0, 0, 129, 1, 0, 1, 64), [4]),              # c2 > 128 with context
      (ds_of(2, 0, 0, 2, 32, 32, 1, 64), [4]),              # pre2 + 1 + post2 = 65
      (ds_of(129, 1, 0, 1, 0, 0, 1, 64), [4]),              # the limits of section 14 hold for input_1 as before
      (ds_of(2, 32, 32, 1, 0, 0, 1, 64), [4]),
      (ds_of(2, 0, 0, 1, 0, 0, 9, 64), [4]),
      (ds_of(2, 0, 0, 1, 0, 0, 1, 2049), [4]),
      (ds_of(2, 0, 0, 1, 0, 0, 1, 64), [4] * 5),
      (ds_of(2, 0, 0, 1, 0, 0, 1, 64), [65]),
  ]
  for ds, hidden in cases:
    m = brain_model.BrainModelClassifier(ds, hidden)
    m.compile()
    before = m.get_weights()
    with pytest.raises(ValueError):
      m.fit(ds)
    with pytest.raises(ValueError):
      m.evaluate(ds)
    with pytest.raises(ValueError):
      m.predict_device(ds)
    for a, b in zip(before, m.get_weights()):
      np.testing.assert_array_equal(a, b)
    assert m._updates == 0
  # the C entry points themselves refuse the same shapes (nothing queued: the parameters stay as they were)
  for (ds, hidden), match in zip(cases[:3], ['lagged inputs of both views', 'second input', 'pre2']):
    x, x2, y, offs = ds.device_arrays(h)
    k = ds.input1_width + ds.input2_width
    n_par = k * hidden[0] + hidden[0] + hidden[0] * ds.d + ds.d
    params = h.to_device(np.ones(n_par, np.float32))
    state = h.zeros((2 * n_par,))
    with pytest.raises(ValueError, match=match):
      device.mlpc_train(x, x2, y, offs, ds.pre, ds.post, ds.pre2, ds.post2, hidden, params, state, 64, 1, handle=h)
    with pytest.raises(ValueError, match=match):
      device.mlpc_grad(x, x2, y, offs, ds.pre, ds.post, ds.pre2, ds.post2, hidden, params, 64, 0, handle=h)
    with pytest.raises(ValueError, match=match):
      device.mlpc_forward(x, x2, offs, ds.pre, ds.post, ds.pre2, ds.post2, hidden, ds.d, params, handle=h)
    assert float(params.sum()) == float(n_par) and float(state.sum()) == 0.0
  # a context-free second input may be wider than 128 channels (what a mixup_batch dataset resolves to)
  wide = ds_of(2, 0, 0, 200, 0, 0, 1, 64, n=200)
  m = brain_model.BrainModelClassifier(wide, [4])
  m.compile()
  assert np.isfinite(m.fit(wide).history['loss'][0])
