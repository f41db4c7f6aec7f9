"""GPU parity of ALREADY-LAGGED minibatches at real widths (the input the reference's callers pass:
brain_model.py:425-444, cca.py:304-332).  Every minibatch becomes a context-free "file" of K = C * L
channels, which sends K > 128 to the wide tile grid of the float32 lag kernel, the unfused targets
route, the three-call CCA moments and the lane-per-channel prediction.  Truth is float64: dense
X^T X for the moments, oracle/regression and oracle/cca for the weights.  Each end-to-end case
records the max-norm relative distance and the element-wise one (tests/host_device.py)."""
import numpy as np
import pytest

from oracle import cca as o_cca
from oracle import lag as o_lag
from oracle import pearson as o_pear
from oracle import regression as o_reg
from tests import host_device as hd
from tests import parity_log

pytestmark = pytest.mark.gpu

LAMB = 0.1
# Weights: 1e-5 max-norm relative; element-wise (entries above 1e-3 of the largest) 1e-4 -- an entry at
# the cut-off carries the max-norm distance (~1e-7 at K = 2048) times 1e3 of its own size.
W_ELEM = 1e-4


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _batches(x, y, batch, perm=None, key='input_1', x2=None):
  """(dict, y) minibatches of `batch` rows (None: one of everything), rows permuted first."""
  if perm is not None:
    x = x[perm]
    y = y[perm] if y is not None else None
    x2 = x2[perm] if x2 is not None else None
  n = x.shape[0]
  batch = batch or n
  out = []
  for s in range(0, n, batch):
    feats = {key: x[s:s + batch]}
    if x2 is not None:
      feats['input_2'] = x2[s:s + batch]
    out.append((feats, y[s:s + batch] if y is not None else None))
  return out


# --------------------------------------------------------------------------- 1. moments, C-ABI level
WIDE_MOMENTS = [
    # K, c2, d, rows of each minibatch (the last one shorter where it differs), strided input
    (130, 0, 1, (2049, 65), False),
    (191, 1, 0, (64, 1, 63), False),
    (192, 0, 4, (2048,), True),
    (193, 8, 0, (65, 2047), True),
    (255, 0, 5, (1, 2049), False),
    (256, 31, 0, (2048, 65), False),
    (257, 32, 0, (2049, 64), True),
    (513, 65, 0, (20000, 2047), False),
    (513, 0, 64, (2048, 63), True),
    (1000, 0, 1, (2048, 999), True),
    (2049, 0, 1, (2049, 2048, 1), True),
    (2553, 31, 0, (2048, 500), True),
]


def _wide_case(h, k, c2, d, rows, strided, seed):
  """Host float32 minibatches and their device copies; strided: a column slice t[:, 1:K + 1] of a
  wider device tensor (row stride K + 3, base 4 bytes past a 16-byte boundary)."""
  import torch
  rng = np.random.default_rng(seed)
  mbs = []
  for r in rows:
    x = rng.standard_normal((r, k)).astype(np.float32)
    x2 = rng.standard_normal((r, c2)).astype(np.float32) if c2 else None
    y = rng.standard_normal((r, d)).astype(np.float32) if d else None
    if strided:
      wide = torch.zeros((r, k + 3), dtype=torch.float32, device=h.device)
      wide[:, 1:k + 1] = torch.from_numpy(x).to(h.device)
      xd = wide[:, 1:k + 1]
      assert xd.stride(0) == k + 3 and (r == 1 or not xd.is_contiguous())
    else:
      xd = h.to_device(x)
    mbs.append((x, x2, y, xd, h.to_device(x2) if c2 else None, h.to_device(y) if d else None))
  return mbs


def _wide_truth(mbs, c2, d):
  x = np.concatenate([m[0] for m in mbs]).astype(np.float64)
  x1 = np.hstack((x, np.ones((x.shape[0], 1))))
  t = {'xtx': x1.T @ x1}
  if d:
    y = np.concatenate([m[2] for m in mbs]).astype(np.float64)
    t['xty'], t['yy'] = x1.T @ y, np.sum(y * y, axis=0)
  if c2:
    x2 = np.concatenate([m[1] for m in mbs]).astype(np.float64)
    t['x2tx2'], t['xtx2'], t['sum_x2'] = x2.T @ x2, x.T @ x2, x2.sum(axis=0)
  return t


def _wide_stats(dev, h, mbs, k, c2, d):
  st = dev.LagStats(k, 0, 0, c2, 0, 0, d, handle=h)
  for _, _, _, xd, x2d, yd in mbs:
    st.accumulate(xd, x2d, yd)
  return st


def _wide_errors(st, t, c2, d):
  m = st.moments(want_cca=bool(c2))
  xtx = m['xtx'].cpu().numpy()
  np.testing.assert_array_equal(xtx, xtx.T)
  errs = {'xtx': hd.moment_rel(xtx, t['xtx'])}
  gd = np.diag(t['xtx'])
  if d:
    errs['xty'] = hd.moment_rel(m['xty'].cpu().numpy(), t['xty'], gd, t['yy'])
  if c2:
    g2 = np.diag(t['x2tx2'])
    errs['x2tx2'] = hd.moment_rel(m['x2tx2'].cpu().numpy(), t['x2tx2'])
    errs['xtx2'] = hd.moment_rel(m['xtx2'].cpu().numpy(), t['xtx2'], gd[:-1], g2)
    errs['sum_x2'] = float(np.max(np.abs(m['sum_x2'].cpu().numpy() - t['sum_x2']) /
                                  np.sqrt(gd[-1] * g2)))
  return xtx, m, errs


@pytest.mark.parametrize('k,c2,d,rows,strided', WIDE_MOMENTS)
def test_wide_context_free_moments_match_dense_float64(dev, k, c2, d, rows, strided):
  """LagStats(K, 0, 0, c2, 0, 0, d) over context-free minibatches -- what _iterable_stats builds
  from already-lagged input -- against dense float64 products: 64-column tile edges, odd widths
  (scalar loads), strided and misaligned input, 1 .. 20 000 rows a call, short last minibatches."""
  h = dev.default_handle()
  mbs = _wide_case(h, k, c2, d, rows, strided, seed=k * 7 + c2 + d)
  st = _wide_stats(dev, h, mbs, k, c2, d)
  frames, files = st.counts()
  assert frames == sum(rows) and files == len(rows)
  t = _wide_truth(mbs, c2, d)
  xtx, _, errs = _wide_errors(st, t, c2, d)
  parity_log.record('prelagged_moments_K%d_c2%d_d%d' % (k, c2, d), rows=sum(rows), strided=strided,
                    maxnorm_rel=hd.maxnorm_rel(xtx, t['xtx']), **{'elem_' + n: v for n, v in errs.items()})
  for name, err in errs.items():
    assert err < 2e-6, (name, err)


def test_accumulate_modes_do_not_change_wide_context_free_moments(dev):
  """The three accumulate modes only choose among the <= 64-channel kernels: at K = 1000 without
  context they run the same float32 kernel, so the moments are bit for bit the same."""
  h = dev.default_handle()
  k, rows = 1000, (2049, 700)
  mbs = _wide_case(h, k, 0, 1, rows, True, seed=77)
  t = _wide_truth(mbs, 0, 1)
  got = {}
  try:
    for mode in ('f16x2', 'bf16x3', 'f32'):
      h.set_accumulate_mode(mode)
      xtx, m, errs = _wide_errors(_wide_stats(dev, h, mbs, k, 0, 1), t, 0, 1)
      got[mode] = (xtx, m['xty'].cpu().numpy())
      assert max(errs.values()) < 2e-6, (mode, errs)
  finally:
    h.set_accumulate_mode('f16x2')
  for mode in ('bf16x3', 'f32'):
    np.testing.assert_array_equal(got[mode][0], got['f16x2'][0])
    np.testing.assert_array_equal(got[mode][1], got['f16x2'][1])


# --------------------------------------------------------------------------- 2. public entry points
N_REC, C_REC, L_REC = 20000, 64, 32          # 64 channels x 32 lags = 2048 lagged columns (+ ones: 2049)


@pytest.fixture(scope='module')
def rec():
  """One 20 000-frame, 64-channel recording, its lag matrix with 31 frames of post-context (the
  C2 layout) and a TRF target; the float64 moments of [xl | 1] and y are computed ONCE (168 GFLOP)
  and every 16-channel case reads its sub-block."""
  rng = np.random.default_rng(2049)
  raw = rng.standard_normal((N_REC, C_REC)).astype(np.float32)
  xl = o_lag.lag_matrix(raw, 0, L_REC - 1)
  w_true = rng.standard_normal((C_REC * L_REC, 1)) * 0.05
  y = (xl.astype(np.float64) @ w_true + 0.5 * rng.standard_normal((N_REC, 1))).astype(np.float32)
  g, gxy = hd.gram64(xl, y)
  cols16 = np.array([l * C_REC + c for l in range(L_REC) for c in range(16)] + [C_REC * L_REC])
  return dict(raw=raw, xl=xl, y=y, g=g, gxy=gxy, cols16=cols16, perm=rng.permutation(N_REC))


def _view(rec, width):
  """(lagged x, G, Gxy) of the 64-channel recording (2048) or of its first 16 channels (512)."""
  if width == C_REC * L_REC:
    return rec['xl'], rec['g'], rec['gxy']
  c = rec['cols16']
  return rec['xl'][:, c[:-1]], rec['g'][np.ix_(c, c)], rec['gxy'][c]


def _spec_dataset(raw, y, batch=1000):
  from telluride_decoding_amd import brain_data
  att = np.zeros((raw.shape[0], 1), np.float32)
  return brain_data.Dataset([(raw, raw[:, :1], y, att)], batch, post_context=L_REC - 1)


def _record_weights(case, w, b, w64, b64, **extra):
  err = hd.maxnorm_rel(np.vstack((w, np.reshape(b, (1, -1)))), np.vstack((w64, b64)))
  elem = hd.weight_rel(w, w64)
  parity_log.record(case, maxnorm_rel=err, elem_rel=elem, **extra)
  return err, elem


def test_ridge_from_moments_is_the_oracle(rec):
  """The float64 truth of this file solves the summed moments (one dense product shared by many
  cases); on the 512-column view it is oracle/regression itself, minibatch loop and all."""
  xl, g, gxy = _view(rec, 512)
  w64, b64 = hd.ridge_from_moments(g, gxy, N_REC, LAMB)
  f64 = [({'input_1': bx['input_1'].astype(np.float64)}, by.astype(np.float64))
         for bx, by in _batches(xl, rec['y'], 1000)]
  w, b, _, _, _ = o_reg.linear_regressor_from_batches(f64, lamb=LAMB)
  assert hd.maxnorm_rel(w, w64) < 1e-10 and hd.maxnorm_rel(b, b64) < 1e-10


@pytest.mark.parametrize('width,entry,batch,shuffled', [
    (2048, 'function', 100, True), (2048, 'function', 1000, False), (2048, 'function', None, True),
    (2048, 'model', 1000, True),
    (512, 'function', 100, False), (512, 'function', 1000, True), (512, 'function', None, False),
    (512, 'model', 100, True)])
def test_ridge_fit_of_lagged_minibatches_matches_float64(dev, rec, width, entry, batch, shuffled):
  """calculate_linear_regressor_parameters_from_dataset(iterable) and BrainModelLinearRegression.fit
  (iterable) on already-lagged minibatches of 100, 1000 or all 20 000 rows, the (x, y) rows in
  recording order or globally permuted, against the float64 ridge solution."""
  from telluride_decoding_amd import brain_model
  xl, g, gxy = _view(rec, width)
  w64, b64 = hd.ridge_from_moments(g, gxy, N_REC, LAMB)
  batches = _batches(xl, rec['y'], batch, rec['perm'] if shuffled else None)
  if entry == 'function':
    w, b, _, _, _ = brain_model.calculate_linear_regressor_parameters_from_dataset(batches, lamb=LAMB)
  else:
    model = brain_model.BrainModelLinearRegression(_spec_dataset(rec['raw'][:, :width // L_REC], rec['y']),
                                                   regularization_lambda=LAMB)
    assert model.fit(batches) == {}
    w, b = model.w_estimate, model.b_estimate
  err, elem = _record_weights('prelagged_ridge_K%d_%s_b%s%s' % (width, entry, batch or 'all',
                                                                 '_shuffled' if shuffled else ''),
                              w, b, w64, b64)
  assert err < 1e-5 and elem < W_ELEM, (err, elem)


def test_forward_model_of_lagged_envelope_matches_oracle(dev):
  """A forward model: 33 lags of an envelope (K = 33) against 64 EEG outputs (d = 64), shuffled
  1000-row minibatches, against oracle/regression in float64."""
  from telluride_decoding_amd import brain_model
  rng = np.random.default_rng(64)
  n = N_REC
  env = np.abs(np.convolve(rng.standard_normal(n + 40), np.ones(8) / 8, 'same'))[:n, None]
  xl = o_lag.lag_matrix(env.astype(np.float32), 0, 32)
  trf = rng.standard_normal((33, 64)) * np.exp(-np.arange(33) / 8.0)[:, None]
  y = (xl @ trf + rng.standard_normal((n, 64))).astype(np.float32)
  batches = _batches(xl, y, 1000, rng.permutation(n))
  f64 = [({'input_1': bx['input_1'].astype(np.float64)}, by.astype(np.float64)) for bx, by in batches]
  w64, b64, _, _, _ = o_reg.linear_regressor_from_batches(f64, lamb=LAMB)
  w, b, _, _, _ = brain_model.calculate_linear_regressor_parameters_from_dataset(batches, lamb=LAMB)
  assert w.shape == (33, 64) and b.shape == (1, 64)
  err, elem = _record_weights('prelagged_forward_K33_d64', w, b, w64, b64)
  assert err < 1e-5 and elem < W_ELEM, (err, elem)


def test_shrinkage_branches_of_lagged_minibatches_match_oracle(dev, rec):
  """use_ridge=False at a fixed lambda = 0.3, and Ledoit-Wolf (lamb = -1, use_ridge = False) at
  K = 512: the shrinkage to 1e-6 relative; the weights to 1e-5 of float64 -- or, if the estimate is
  too ill-conditioned for that, within the reference's own float32 distance + 1e-5 (recorded)."""
  from telluride_decoding_amd import brain_model
  xl, _, _ = _view(rec, 512)
  batches = _batches(xl, rec['y'], 1000)
  f64 = [({'input_1': bx['input_1'].astype(np.float64)}, by.astype(np.float64)) for bx, by in batches]
  w64, b64, _, _, sh64 = o_reg.linear_regressor_from_batches(f64, lamb=0.3, use_ridge=False)
  w, b, _, _, sh = brain_model.calculate_linear_regressor_parameters_from_dataset(batches, lamb=0.3,
                                                                                   use_ridge=False)
  assert sh == sh64 == 0.3
  err, elem = _record_weights('prelagged_shrink_fixed_K512', w, b, w64, b64)
  assert err < 1e-5 and elem < W_ELEM, (err, elem)

  w64, b64, _, _, sh64 = o_reg.linear_regressor_from_batches(f64, lamb=-1, use_ridge=False)
  w32, b32, _, _, _ = o_reg.linear_regressor_from_batches(batches, lamb=-1, use_ridge=False)
  w, b, _, _, sh = brain_model.calculate_linear_regressor_parameters_from_dataset(batches, lamb=-1,
                                                                                   use_ridge=False)
  sh_rel = abs(sh - sh64) / abs(sh64)
  ref32 = hd.maxnorm_rel(np.vstack((w32, b32)), np.vstack((w64, b64)))
  err = hd.maxnorm_rel(np.vstack((w, b)), np.vstack((w64, b64)))
  bound = 'absolute' if err < 1e-5 else 'reference_fp32'
  _record_weights('prelagged_ledoit_wolf_K512', w, b, w64, b64, shrinkage=sh64, shrinkage_rel=sh_rel,
                  reference_fp32_rel=ref32, bound=bound)
  assert sh_rel < 1e-6, (sh, sh64)
  assert err < 1e-5 or err < ref32 + 1e-5, (err, ref32)


def test_prediction_and_evaluate_of_lagged_minibatches(dev, rec):
  """model({'input_1': lagged}) at K = 2048 (the lane-per-channel FIR path, 32 passes of 64
  channels accumulating into the output) against X W + b in float64 with the model's weights, and
  model.evaluate(iterable) against the Keras-style per-minibatch mean of the mse and of the first
  column's Pearson correlation, computed on the host in float64."""
  from telluride_decoding_amd import brain_model
  xl, y = rec['xl'], rec['y']
  batches = _batches(xl, y, 1000)
  model = brain_model.BrainModelLinearRegression(_spec_dataset(rec['raw'], y), regularization_lambda=LAMB)
  model.fit(batches)
  w, b = np.asarray(model.w_estimate, np.float64), np.asarray(model.b_estimate, np.float64)
  rows = slice(3000, 7001)
  pred = model({'input_1': xl[rows]})
  want = o_reg.dense_forward(xl[rows].astype(np.float64), w, b)
  err = hd.maxnorm_rel(pred, want)
  got = model.evaluate(batches)
  preds = [o_reg.dense_forward(bx['input_1'].astype(np.float64), w, b) for bx, _ in batches]
  truths = [by.astype(np.float64) for _, by in batches]
  loss = float(np.mean([np.mean((t - p) ** 2) for t, p in zip(truths, preds)]))
  r = float(o_pear.evaluate_mean_over_batches(o_pear.pearson_correlation_first, preds, truths))
  loss_rel, r_abs = abs(got['loss'] - loss) / loss, abs(got['pearson_correlation_first'] - r)
  parity_log.record('prelagged_predict_evaluate_K2048', maxnorm_rel=err, loss_rel=loss_rel, r_abs=r_abs)
  assert err < 1e-5, err
  assert loss_rel < 1e-5 and r_abs < 1e-5, (got, loss, r)


def test_lagged_statistics_are_invariant_to_order_batching_and_route(dev, rec):
  """The moments of the 2048-column lagged recording are the same -- 2e-6 element-wise, and each
  within 2e-6 of float64 -- whether its rows come shuffled or in order, in minibatches of 100, 1000 or
  all at once, or as the raw 64-channel recording with 31 frames of post-context through the Dataset
  route (the float16 x 2 split kernel against the float32 context-free one); their weights agree to
  1e-5."""
  from telluride_decoding_amd import brain_model
  xl, y, g, gxy = rec['xl'], rec['y'], rec['g'], rec['gxy']
  gd, yy = np.diag(g), float(np.sum(y.astype(np.float64) ** 2))
  w64, b64 = hd.ridge_from_moments(g, gxy, N_REC, LAMB)
  routes = {}
  for name, batch, perm in (('b100_ordered', 100, None), ('b1000_shuffled', 1000, rec['perm']),
                            ('all_shuffled', None, rec['perm'])):
    st, _, _ = brain_model._iterable_stats(_batches(xl, y, batch, perm))
    routes[name] = st
  routes['dataset'] = brain_model._dataset_stats(_spec_dataset(rec['raw'], y))
  mom, wts = {}, {}
  for name, st in routes.items():
    assert st.counts()[0] == N_REC
    m = st.moments()
    mom[name] = (m['xtx'].cpu().numpy(), m['xty'].cpu().numpy())
    wd, bd = st.ridge_solve([LAMB])
    wts[name] = (wd.cpu().numpy()[0], bd.cpu().numpy())
    e_g = hd.moment_rel(mom[name][0], g)
    e_y = hd.moment_rel(mom[name][1], gxy, gd, [yy])
    err, elem = _record_weights('prelagged_route_%s_K2048' % name, wts[name][0], wts[name][1], w64, b64,
                                elem_xtx=e_g, elem_xty=e_y, maxnorm_xtx=hd.maxnorm_rel(mom[name][0], g))
    assert e_g < 2e-6 and e_y < 2e-6, (name, e_g, e_y)
    assert err < 1e-5 and elem < W_ELEM, (name, err, elem)
  base = mom['b100_ordered']
  for name in ('b1000_shuffled', 'all_shuffled', 'dataset'):
    assert hd.moment_rel(mom[name][0], base[0], gd, gd) < 2e-6, name
    assert hd.moment_rel(mom[name][1], base[1], gd, [yy]) < 2e-6, name
    assert hd.maxnorm_rel(np.vstack((wts[name][0], wts[name][1])),
                          np.vstack((wts['b100_ordered'][0], wts['b100_ordered'][1]))) < 1e-5, name


# --------------------------------------------------------------------------- CCA at the codelab's width
N_CCA, C_CCA, L_CCA, L_ENV = 4000, 69, 37, 31         # K1 = 69 x 37 = 2553, K2 = 31


@pytest.fixture(scope='module')
def cca_rec():
  rng = np.random.default_rng(2553)
  src = rng.standard_normal((N_CCA, 4))
  mix = rng.standard_normal((4, C_CCA)) * np.array([1.0, 0.6, 0.3, 0.1])[:, None]
  raw = (src @ mix + rng.standard_normal((N_CCA, C_CCA))).astype(np.float32)
  env = (src[:, :1] + 0.5 * rng.standard_normal((N_CCA, 1))).astype(np.float32)
  return dict(raw=raw, env=env, xl=o_lag.lag_matrix(raw, 0, L_CCA - 1),
              el=o_lag.lag_matrix(env, 0, L_ENV - 1), perm=rng.permutation(N_CCA))


def _cca_compare(case, got, want):
  ra, rb, mx, my, e = want
  gx, gy, gmx, gmy, ge = (np.asarray(a, np.float64) for a in got)
  dim = e.size
  e_rel = float(np.max(np.abs(ge - e) / e))
  sign = np.sign(np.sum(gx * ra, axis=0))
  assert np.all(sign != 0)
  gap = np.min(np.abs(np.diff(np.concatenate((e, [0.0]))))) if dim > 1 else 1.0
  tol = 2e-6 / max(gap, 1e-3)
  rot_x, rot_y = hd.maxnorm_rel(gx * sign, ra), hd.maxnorm_rel(gy * sign, rb)
  parity_log.record(case, e_rel=e_rel, rot_x_maxnorm=rot_x, rot_y_maxnorm=rot_y, gap=gap, rot_tol=tol,
                    rot_x_elem=hd.weight_rel(gx * sign, ra), rot_y_elem=hd.weight_rel(gy * sign, rb))
  np.testing.assert_allclose(ge, e, rtol=1e-5)
  assert rot_x < tol and rot_y < tol, (rot_x, rot_y, tol)
  np.testing.assert_allclose(gmx, mx, atol=1e-6)
  np.testing.assert_allclose(gmy, my, atol=1e-6)
  return sign


@pytest.mark.parametrize('case,batch,count,shuffled', [
    ('shuffled', 400, 0, True), ('uneven_last', 700, 0, False), ('mini_batch_count', 400, 4, True)])
def test_cca_of_lagged_minibatches_at_codelab_width(dev, cca_rec, case, batch, count, shuffled):
  """cca.calculate_cca_parameters_from_dataset(iterable, dim=5) at K1 = 2553 against K2 = 31:
  rows shuffled; an uneven last minibatch (its row count enters the (num_mini_batches n_row - 1)
  denominator, cca.py:339); mini_batch_count below the number of minibatches."""
  from telluride_decoding_amd import cca
  batches = _batches(cca_rec['xl'], None, batch, cca_rec['perm'] if shuffled else None, x2=cca_rec['el'])
  f64 = [({'input_1': bx['input_1'].astype(np.float64), 'input_2': bx['input_2'].astype(np.float64)}, None)
         for bx, _ in batches]
  # (np.linalg.eig of the reference may return complex arrays with zero imaginary parts)
  want = tuple(np.real(a) for a in o_cca.cca_parameters_from_batches(f64, 5, regularization=0.1,
                                                                      mini_batch_count=count))
  got = cca.calculate_cca_parameters_from_dataset(batches, 5, regularization=0.1, mini_batch_count=count)
  _cca_compare('prelagged_cca_K2553_%s' % case, got, want)


def test_cca_model_call_and_evaluate_on_lagged_minibatches(dev, cca_rec):
  """BrainModelCCA.fit / call / evaluate on dict minibatches at K1 = 2553, K2 = 31 against
  oracle/cca's transform with the oracle's own rotations (1e-4: DESIGN section 5)."""
  from telluride_decoding_amd import brain_data, cca
  xl, el = cca_rec['xl'], cca_rec['el']
  batches = _batches(xl, None, 400, cca_rec['perm'], x2=el)
  att = np.zeros((N_CCA, 1), np.float32)
  spec = brain_data.Dataset([(cca_rec['raw'], cca_rec['env'], att, att)], 400, post_context=L_CCA - 1,
                            in2_post_context=L_ENV - 1)
  model = cca.BrainModelCCA(spec, cca_dims=5, regularization_lambda=0.1)
  assert model.fit(batches) == {}
  f64 = [({'input_1': bx['input_1'].astype(np.float64), 'input_2': bx['input_2'].astype(np.float64)}, None)
         for bx, _ in batches]
  want = tuple(np.real(a) for a in o_cca.cca_parameters_from_batches(f64, 5, regularization=0.1,
                                                                      mini_batch_count=0))
  ra, rb, mx, my, _ = want
  sign = _cca_compare('prelagged_cca_model_K2553',
                      (model.rot_x, model.rot_y, model.mean_x, model.mean_y, model.eigenvalues), want)
  rows = slice(1000, 2000)
  out = np.asarray(model({'input_1': xl[rows], 'input_2': el[rows]}), np.float64)
  ref = o_cca.cca_transform(xl[rows].astype(np.float64), el[rows].astype(np.float64), mx, my, ra, rb)
  err = hd.maxnorm_rel(out * np.concatenate((sign, sign)), ref)
  got = model.evaluate(batches)
  zs = [o_cca.cca_transform(bx['input_1'], bx['input_2'], mx, my, ra, rb) for bx, _ in f64]
  r = float(np.mean([o_pear.pearson_correlation(z[:, :5], z[:, 5:])[0] for z in zs]))
  r_abs = abs(got['cca_pearson_correlation_first'] - r)
  parity_log.record('prelagged_cca_transform_evaluate_K2553', maxnorm_rel=err, r_abs=r_abs)
  assert err < 1e-4, err
  assert r_abs < 1e-4 and got['loss'] == got['cca_pearson_correlation_first'], (got, r)


# --------------------------------------------------------------------------- 3. DC offsets
_DC_REF = {}


def _dc_case(rec, dc, width):
  """(raw + offsets, lagged view, float64 W / b, the reference's own float32 W / b).  Offsets per
  channel dc * U(1, 2) sigma (the recording has unit variance); the float64 moments follow from the
  zero-offset ones (host_device.offset_moments), the reference's arithmetic is oracle/regression on
  float32 minibatches of 1000 rows (np.matmul per minibatch, float32 sums: brain_model.py:437-439)."""
  key = (dc, width)
  if key not in _DC_REF:
    rng = np.random.default_rng(int(dc))
    off = dc * rng.uniform(1.0, 2.0, C_REC)
    raw = (rec['raw'] + off).astype(np.float32)
    g, gxy = hd.offset_moments(rec['g'], rec['gxy'], rec['xl'], rec['y'], off, 0, L_REC - 1)
    if width != C_REC * L_REC:
      c = rec['cols16']
      g, gxy, raw = g[np.ix_(c, c)], gxy[c], raw[:, :width // L_REC]
    w64, b64 = hd.ridge_from_moments(g, gxy, N_REC, LAMB)
    xl = o_lag.lag_matrix(raw, 0, L_REC - 1)
    w32, b32, _, _, _ = o_reg.linear_regressor_from_batches(_batches(xl, rec['y'], 1000), lamb=LAMB)
    ref32 = hd.maxnorm_rel(np.vstack((w32, b32)), np.vstack((w64, b64)))
    _DC_REF[key] = (raw, xl, g, w64, b64, ref32)
  return _DC_REF[key]


def _dc_check(case, st, g, w, b, w64, b64, ref32, dc, width):
  """The moments to 2e-6 element-wise (the kernels do what td_common.h says); the weights at most
  a quarter of the reference's own float32 distance, and within 1e-5 at 3 sigma on the 512-column
  view.  (At 2048 columns 3 sigma costs 1.2 .. 1.8e-5 in every accumulate mode: the conditioning of
  uncentred moments)"""
  xtx = st.moments(want_xty=False)['xtx'].cpu().numpy()
  e_g = hd.moment_rel(xtx, g)
  err, elem = _record_weights(case, w, b, w64, b64, dc_sigma=dc, reference_fp32_rel=ref32, elem_xtx=e_g,
                              maxnorm_xtx=hd.maxnorm_rel(xtx, g))
  assert e_g < 2e-6, e_g
  assert err <= 0.25 * ref32, (err, ref32)
  if dc <= 3 and width == 512:
    assert err < 1e-5, (err, ref32)


@pytest.mark.parametrize('dc', [3, 10, 30])
@pytest.mark.parametrize('mode', ['f16x2', 'bf16x3', 'f32'])
def test_dc_offset_dataset_route(dev, rec, dc, mode):
  """Uncentred moments of channels N(0, 1) + dc U(1, 2) sigma through the Dataset route (64
  channels x 32 lags: the float16 x 2 split kernel by default) in each accumulate mode: within 1e-5
  of float64 at 3 sigma; at 10 and 30 sigma at most a quarter of the reference's own float32
  distance."""
  from telluride_decoding_amd import brain_model
  raw, _, g, w64, b64, ref32 = _dc_case(rec, dc, C_REC * L_REC)
  h = dev.default_handle()
  try:
    h.set_accumulate_mode(mode)
    ds = _spec_dataset(raw, rec['y'])
    w, b, _, _, _ = brain_model.calculate_linear_regressor_parameters_from_dataset(ds, lamb=LAMB)
    st = brain_model._dataset_stats(ds)
  finally:
    h.set_accumulate_mode('f16x2')
  _dc_check('prelagged_dc%d_dataset_K2048_%s' % (dc, mode), st, g, w, b, w64, b64, ref32, dc, 2048)


@pytest.mark.parametrize('dc', [3, 10, 30])
@pytest.mark.parametrize('width', [512, 2048])
def test_dc_offset_iterable_route(dev, rec, dc, width):
  """The same offsets handed over already lagged (the float32 context-free kernel), minibatches
  of 1000 rows: 16 channels x 32 lags (K = 512), and the 2048 columns of the Dataset route above."""
  from telluride_decoding_amd import brain_model
  _, xl, g, w64, b64, ref32 = _dc_case(rec, dc, width)
  batches = _batches(xl, rec['y'], 1000)
  w, b, _, _, _ = brain_model.calculate_linear_regressor_parameters_from_dataset(batches, lamb=LAMB)
  st, _, _ = brain_model._iterable_stats(batches)
  _dc_check('prelagged_dc%d_iterable_K%d' % (dc, width), st, g, w, b, w64, b64, ref32, dc, width)


# --------------------------------------------------------------------------- 4. scratch of long wide calls
def test_one_long_wide_call_equals_slab_sized_calls_in_bounded_scratch(dev):
  """One 131 072-row call at K = 2049 (64 slabs of 2048 rows, 143 MB of partial sums each) gives the
  moments of sixty-four 2048-row calls to 1e-12, and the handle's scratch stays under the cap of
  td_lagcov (256 MB, x 1.25 growth) instead of holding all 64 slabs (9 GB)."""
  import torch
  h = dev.Handle()                  # a handle of its own: its scratch starts empty
  k, rows, slab = 2049, 131072, 2048
  gen = torch.Generator(device=h.device)
  gen.manual_seed(2049)
  x = torch.randn((rows, k), generator=gen, device=h.device, dtype=torch.float32)
  one = dev.LagStats(k, handle=h)
  one.accumulate(x)
  m1 = one.moments(want_xty=False)['xtx'].cpu().numpy()
  h.synchronize()
  scratch = h.scratch_bytes()
  many = dev.LagStats(k, handle=h)
  for s in range(0, rows, slab):
    many.accumulate(x[s:s + slab])
  m64 = many.moments(want_xty=False)['xtx'].cpu().numpy()
  assert one.counts() == (rows, 1) and many.counts() == (rows, rows // slab)
  err = hd.maxnorm_rel(m1, m64)
  parity_log.record('prelagged_long_call_K2049', rows=rows, maxnorm_rel=err, scratch_mb=scratch / 2.0 ** 20)
  assert err < 1e-12, err
  assert scratch <= (256 << 20) * 5 // 4, scratch
