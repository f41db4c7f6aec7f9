"""GPU parity tests of the fit path (A1-A3): lagged statistics, moments, ridge.

Every check calls the HIP kernels through the C-ABI and compares with the CPU
oracle (oracle/) on the same seeded inputs, or with the golden fixtures produced
by the reference itself.
"""
import numpy as np
import pytest

from oracle import lag as o_lag
from oracle import regression as o_reg
from tests import host_device as hd
from tests import parity_log
from tests.conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _dense_moments(files, pre, post, pre2, post2, input_offset, rows_used_last, dt=np.float64):
  """Literal reference arithmetic in float64: materialise the lag matrices."""
  xs, x2s, ys = [], [], []
  for i, (x, x2, y) in enumerate(files):
    a = np.zeros((x.shape[0], 1), np.float32)
    xl, x2l, yl, _ = o_lag.window_streams(x.astype(dt), x2.astype(dt), y.astype(dt), a,
                                          pre=pre, post=post, pre2=pre2, post2=post2,
                                          input_offset=input_offset)
    if i == len(files) - 1 and rows_used_last is not None:
      xl, x2l, yl = xl[:rows_used_last], x2l[:rows_used_last], yl[:rows_used_last]
    xs.append(xl); x2s.append(x2l); ys.append(yl)
  X = np.concatenate(xs); X2 = np.concatenate(x2s); Y = np.concatenate(ys)
  X1 = np.hstack((X, np.ones((X.shape[0], 1), dt)))
  return dict(xtx=X1.T @ X1, xty=X1.T @ Y, x2tx2=X2.T @ X2, xtx2=X.T @ X2,
              sum_x2=X2.sum(axis=0), n=X.shape[0])


def _rel(a, b):
  return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


@pytest.mark.parametrize('c1,pre,post,c2,pre2,post2,d,off,lens,drop', [
    (5, 2, 3, 3, 1, 2, 1, 0, (700, 333, 1021), 0),
    (5, 2, 3, 3, 1, 2, 2, 0, (700, 333, 1021), 57),
    (16, 0, 7, 0, 0, 0, 1, 0, (2000, 1500), 0),
    (16, 3, 0, 0, 0, 0, 1, 2, (900, 901), 13),
    (7, 1, 4, 2, 2, 0, 1, -3, (640, 129), 5),
    (64, 0, 31, 0, 0, 0, 1, 0, (5000, 4096, 3000), 96),
    (70, 4, 4, 9, 0, 3, 3, 0, (1500, 800), 0),       # more than one channel tile
    (3, 0, 0, 2, 0, 0, 1, 0, (1000,), 0),            # no lags at all
    (4, 5, 5, 0, 0, 0, 1, 0, (8, 3, 1200), 0),       # files shorter than the context
    # CCA without context and without targets: the one-pass Gram kernel (td_gram)
    (64, 0, 0, 8, 0, 0, 0, 0, (3000, 0, 2177, 130), 0),
    (10, 0, 0, 3, 0, 0, 0, 2, (1500, 700), 41),      # scalar-load variant, input_offset > 0
    (61, 0, 0, 31, 0, 0, 0, -3, (5000, 129), 7),     # widest x2 tile, input_offset < 0
    (32, 0, 0, 16, 0, 0, 0, 0, (100, 20000), 0),
    (65, 0, 0, 8, 0, 0, 0, 0, (1500, 700), 0),       # too wide for it: the lag kernels
    # the bf16x3 accumulate kernel (33..64 channels, <= 32 lags): channel counts that need
    # masks / scalar loads, files around the 128-sample tile and the 2048-sample slab, cut tiles
    (37, 3, 8, 0, 0, 0, 1, 0, (700, 333, 1021, 5), 0),
    (48, 0, 15, 0, 0, 0, 2, 1, (128, 129, 127, 160, 2049), 0),
    (63, 5, 2, 0, 0, 0, 1, -2, (4097, 64), 31),
    (33, 0, 4, 0, 0, 0, 1, 0, (10, 3000), 0),
    (64, 16, 15, 0, 0, 0, 1, 0, (2048, 2048, 100), 0),
    (64, 0, 8, 0, 0, 0, 1, 0, (6000, 1), 0),
    # the float16 kernel with the target column riding along (one target, no pre-context):
    # offsets of either sign, recordings shorter than the lag span, a dropped remainder that
    # leaves real rows behind the summed range (they pair with the last targets)
    (40, 0, 20, 0, 0, 0, 1, 2, (130, 129, 2050, 131), 77),
    (64, 0, 31, 0, 0, 0, 1, -3, (4097, 640), 5),
    (57, 0, 31, 0, 0, 0, 1, 0, (17, 9000, 400), 130),
    # 65 .. 128 channels: every pair of 32-channel tiles gathered into a 64-channel copy of its
    # own for the split kernel (3 passes up to 96 channels, 6 up to 128)
    (69, 0, 36, 0, 0, 0, 1, 0, (2500, 700), 0),
    (90, 10, 30, 0, 0, 0, 1, 2, (700, 129, 2500), 9),
    (97, 0, 3, 0, 0, 0, 1, -2, (300, 5, 1400), 0),
    (100, 2, 9, 0, 0, 0, 2, 1, (1800, 129, 640), 13),
    (128, 0, 31, 0, 0, 0, 1, 0, (3000,), 0),
    (65, 1, 2, 0, 0, 0, 1, 0, (900, 901), 0),
    # lagged CCA with a narrow second view (<= 8 columns) against a wide first one: the
    # cross-covariance runs with the operands swapped (skinny kernel + reversed, transposed add);
    # offsets of either sign, a dropped remainder, recordings shorter than the lag span, the
    # codelab's 69 x 1 channels
    (69, 0, 36, 1, 0, 30, 0, 0, (2500, 700), 0),
    (12, 2, 3, 3, 4, 1, 0, 2, (900, 40, 1300), 57),
    (33, 0, 8, 8, 3, 3, 2, -3, (1500, 5, 700), 11),
    (20, 5, 0, 2, 0, 6, 0, 0, (64, 3000), 0),
    # a one-column second view: its auto- and cross-covariance as a "target column" on the
    # matrix-core targets kernel in windows of 32 lags (td_lagcov_column), windows without lag 0
    (20, 3, 4, 1, 5, 40, 0, 2, (900, 40, 1300), 57),
    (33, 0, 8, 1, 3, 3, 1, -3, (1500, 5, 700), 11),
    (64, 0, 63, 1, 31, 0, 0, 0, (4000, 129), 0),
    (9, 0, 0, 1, 0, 33, 0, 0, (2600,), 0),
    # both operands narrow (<= 8 channels, >= 8 lags): the VALU kernel with a row of outputs per
    # thread -- auto- and cross-covariances of a lagged CCA's narrow views, a narrow regression
    (8, 3, 12, 8, 7, 8, 2, 1, (900, 40, 1300), 57),
    (6, 0, 40, 0, 0, 0, 1, 0, (3000, 64), 0),
    (3, 0, 7, 2, 9, 0, 0, -2, (500, 700), 0),
    (64, 0, 20, 8, 7, 8, 0, 0, (2500, 2049), 0),
    # more than four target columns: a narrow x against wide targets with the operands swapped
    # (a forward model), 5 .. 16 columns on the matrix-core targets kernel four at a time, the
    # general kernel beyond; offsets of either sign, dropped remainders, short recordings
    (6, 2, 9, 0, 0, 0, 12, 1, (900, 40, 1300), 57),
    (2, 0, 40, 0, 0, 0, 70, -3, (1500, 5, 700), 0),
    (64, 0, 31, 0, 0, 0, 8, -2, (3000, 700), 0),
    (40, 3, 8, 0, 0, 0, 16, 0, (500, 5, 2000), 13),
    (12, 1, 1, 0, 0, 0, 20, 2, (800, 300), 0),
    # boundaries: 129 channels (three 64-channel tiles of the general kernels), 96 channels exactly,
    # 65 lags (one past the split kernel's 64), K + 1 a multiple of 64
    (129, 0, 2, 0, 0, 0, 1, 0, (700, 300), 0),
    (96, 1, 1, 0, 0, 0, 2, -1, (900, 200), 0),
    (34, 32, 32, 0, 0, 0, 1, 0, (1500, 400), 0),
    (21, 0, 2, 0, 0, 0, 1, 0, (800,), 0),
    # 33 .. 64 lags: the 192-row geometry of the same kernel
    (64, 40, 20, 0, 0, 0, 1, 0, (3000, 260, 129), 0),
    (44, 0, 32, 0, 0, 0, 1, 3, (2500, 2049), 17),
    (64, 31, 32, 0, 0, 0, 1, 0, (191, 192, 193, 5000), 0),
    # 9 .. 32 channels with at least 5 lags, 65 .. 128 channels: the float16 kernel on VIRTUAL images
    # (shifted copies of a narrow block of channels fill a 32-channel tile): whole tiles, copies on
    # both sides (<= 16 channels), dropped remainders (rows behind the summed range), offsets,
    # recordings shorter than the copies' shifts, 33 .. 64 lags, a narrow third block (65 .. 80)
    (32, 0, 31, 0, 0, 0, 1, 0, (5000, 4096, 300), 96),
    (16, 0, 31, 0, 0, 0, 1, 0, (3000, 129, 2049), 57),
    (16, 8, 8, 0, 0, 0, 2, -2, (700, 12, 1500), 0),
    (10, 0, 15, 0, 0, 0, 1, 1, (7, 2600), 33),
    (24, 4, 20, 0, 0, 0, 1, 0, (1300, 127, 128), 0),
    (12, 0, 63, 0, 0, 0, 1, 0, (2100, 40), 0),
    (28, 20, 20, 0, 0, 0, 1, 0, (1500, 400), 5),
    (9, 2, 2, 0, 0, 0, 1, 0, (900, 3), 0),
    (69, 0, 36, 0, 0, 0, 1, 1, (2500, 20, 700), 130),
    (72, 0, 31, 0, 0, 0, 1, 0, (3000, 129), 0),
    (80, 16, 15, 0, 0, 0, 1, 0, (2600,), 7),
    (112, 0, 15, 0, 0, 0, 1, 0, (1400, 300), 0),
    (20, 0, 11, 8, 3, 3, 0, 0, (1500, 5, 700), 11),
    # <= 16 channels x <= 16 lags: ONE streaming kernel for matrix and targets (float32 16 x 16 x 4 matrix
    # instruction, lagcov_narrow16_kernel): the C1 shape, odd channel counts, 2 .. 4 targets, a pre-context
    # (the targets' lags start before 0), offsets of either sign, a recording shorter than the context,
    # dropped remainders, one lag, one channel, both lag-group layouts (<= 8 and 9 .. 16 lags)
    (16, 0, 3, 0, 0, 0, 1, 0, (5000, 4096, 300), 96),
    (13, 2, 5, 0, 0, 0, 3, -2, (700, 5, 1300), 31),
    (1, 0, 15, 0, 0, 0, 4, 1, (900, 40), 0),
    (9, 7, 8, 0, 0, 0, 2, 0, (130, 129, 2050), 77),
    (16, 0, 0, 0, 0, 0, 1, 0, (1000, 7), 0),
    (5, 1, 1, 0, 0, 0, 2, 3, (64, 65, 63, 9), 0),
])
def test_moments_match_dense_lag_matrix(dev, c1, pre, post, c2, pre2, post2, d, off, lens, drop):
  rng = np.random.default_rng(1234 + c1 + pre * 7 + post)
  files = []
  for n in lens:
    x = rng.standard_normal((n, c1)).astype(np.float32)
    x2 = rng.standard_normal((n, max(c2, 1))).astype(np.float32)
    y = rng.standard_normal((n, max(d, 1))).astype(np.float32)[:, :d]
    files.append((x, x2, y))
  zipped_last = lens[-1] - abs(off)
  used_last = zipped_last - drop if drop else None
  ref = _dense_moments(files, pre, post, pre2 if c2 else 0, post2 if c2 else 0, off, used_last)

  h = dev.default_handle()
  st = dev.LagStats(c1, pre, post, c2, pre2, post2, d)
  offs = np.concatenate(([0], np.cumsum(lens)))
  xd = h.to_device(np.concatenate([f[0] for f in files]))
  x2d = h.to_device(np.concatenate([f[1] for f in files])) if c2 else None
  yd = h.to_device(np.concatenate([f[2] for f in files])) if d else None
  rows_used = None
  if drop:
    rows_used = [n - abs(off) for n in lens]
    rows_used[-1] = used_last
  st.accumulate(xd, x2d, yd, offs, input_offset=off, rows_used=rows_used)
  frames, nfiles = st.counts()
  assert frames == ref['n'] and nfiles == len(lens)
  m = st.moments(want_cca=bool(c2))
  # float32 products accumulated in f32 chains of <= 16k samples, then float64:
  # well inside 1e-5 of the exact float64 moments.
  assert _rel(m['xtx'].cpu().numpy(), ref['xtx']) < 2e-6
  if d:
    assert _rel(m['xty'].cpu().numpy(), ref['xty']) < 2e-6
  if c2:
    assert _rel(m['x2tx2'].cpu().numpy(), ref['x2tx2']) < 2e-6
    assert _rel(m['xtx2'].cpu().numpy(), ref['xtx2']) < 2e-6
    assert _rel(m['sum_x2'].cpu().numpy(), ref['sum_x2']) < 2e-6
  xtx = m['xtx'].cpu().numpy()
  np.testing.assert_array_equal(xtx, xtx.T)       # symmetric by construction


def test_accumulate_is_additive_and_packable(dev):
  """Files added in two calls, combined from parts, or sent through the packed
  all-reduce buffer give the same statistics."""
  rng = np.random.default_rng(5)
  c1, pre, post, d = 8, 2, 5, 1
  lens = (400, 777, 512, 300)
  xs = [rng.standard_normal((n, c1)).astype(np.float32) for n in lens]
  ys = [rng.standard_normal((n, d)).astype(np.float32) for n in lens]
  h = dev.default_handle()

  def stats_of(idx):
    st = dev.LagStats(c1, pre, post, d=d)
    offs = np.concatenate(([0], np.cumsum([lens[i] for i in idx])))
    st.accumulate(h.to_device(np.concatenate([xs[i] for i in idx])), None,
                  h.to_device(np.concatenate([ys[i] for i in idx])), offs)
    return st

  whole = stats_of([0, 1, 2, 3])
  ref = whole.moments()['xtx'].cpu().numpy()
  two = stats_of([0, 1])
  offs = np.concatenate(([0], np.cumsum(lens[2:])))
  two.accumulate(h.to_device(np.concatenate(xs[2:])), None, h.to_device(np.concatenate(ys[2:])), offs)
  np.testing.assert_allclose(two.moments()['xtx'].cpu().numpy(), ref, rtol=1e-12, atol=1e-9)

  a, b = stats_of([0, 1]), stats_of([2, 3])
  comb = a.like().combine([a, b])
  np.testing.assert_allclose(comb.moments()['xtx'].cpu().numpy(), ref, rtol=1e-12, atol=1e-9)
  assert comb.counts() == whole.counts()

  # what two ranks would all-reduce: sum of packed buffers == concatenation
  buf = a.pack(4, 0) + b.pack(4, 2)
  merged = a.like()
  merged.unpack(buf, 4)
  np.testing.assert_allclose(merged.moments()['xtx'].cpu().numpy(), ref, rtol=1e-12, atol=1e-9)
  assert merged.counts() == whole.counts()


# cases whose reference (float32) output is further than 3e-6 from the same algorithm in float64
# (|ref32 - ref64| in profiles/r02_parity.json): more lags on low-pass data, lambda = 0
ILL_CONDITIONED_C1 = ('c1_pre2post2', 'c1_lam0', 'c1_offp2')
C1_CASES = ['c1_nolag', 'c1_post3', 'c1_pre2post2', 'c1_lam0', 'c1_lam10', 'c1_offp2', 'c1_offm3']


@pytest.mark.parametrize('name', C1_CASES)
def test_ridge_matches_reference_golden(dev, name):
  """TRF weights against the reference's own output (float32 path there):
  within 1e-5 relative, the tolerance BASELINE.json's north_star states."""
  g = golden('g2_ridge')
  nf, pre, post, batch, off = (int(v) for v in g[name + '_cfg'])
  lamb = float(g[name + '_lamb'])
  h = dev.default_handle()
  eeg = [g['c1_eeg%d' % i] for i in range(nf)]
  env = [g['c1_env%d' % i][:, 0:1] for i in range(nf)]
  lens = [e.shape[0] for e in eeg]
  zipped = [n - abs(off) for n in lens]
  total = sum(zipped)
  rows_used = list(zipped)
  rows_used[-1] -= total % batch          # batch(drop_remainder=True)
  st = dev.LagStats(16, pre, post, d=1)
  st.accumulate(h.to_device(np.concatenate(eeg)), None, h.to_device(np.concatenate(env)),
                np.concatenate(([0], np.cumsum(lens))), input_offset=off, rows_used=rows_used)
  w, b = st.ridge_solve([lamb])
  w, b = w.cpu().numpy()[0].astype(np.float64), b.cpu().numpy().astype(np.float64)
  w32, b32 = g[name + '_w'].astype(np.float64), g[name + '_b'].astype(np.float64)
  # The reference runs in float32 end to end, so its own rounding noise is part
  # of the distance.  Report all three ("Hard parts"): the same
  # algorithm in float64 is the arbiter.
  files = []
  for i in range(nf):
    e64 = g['c1_eeg%d' % i].astype(np.float64)
    v64 = g['c1_env%d' % i].astype(np.float64)
    files.append((e64, v64[:, 1:2], v64[:, 0:1], np.zeros((e64.shape[0], 1))))
  w64, b64, _, _, _ = o_reg.linear_regressor_from_batches(
      o_lag.minibatches(files, batch, pre=pre, post=post, input_offset=off), lamb=lamb)
  scale = np.max(np.abs(w64))
  d_gpu_64 = max(np.max(np.abs(w - w64)), np.max(np.abs(b - b64))) / scale
  d_32_64 = max(np.max(np.abs(w32 - w64)), np.max(np.abs(b32 - b64))) / scale
  d_gpu_32 = max(np.max(np.abs(w - w32)), np.max(np.abs(b - b32))) / scale
  print('%s: |gpu-ref64| %.2e  |ref32-ref64| %.2e  |gpu-ref32| %.2e' %
        (name, d_gpu_64, d_32_64, d_gpu_32))
  parity_log.record('ridge_golden_' + name, gpu_ref64=d_gpu_64, ref32_ref64=d_32_64,
                    gpu_ref32=d_gpu_32, strict=bool(d_gpu_32 < 1e-5))
  # north_star: TRF weights within 1e-5 relative of the reference's float32 output.  STRICT for
  # every case, except the named ones where the reference's own float32 rounding (its distance
  # from the same algorithm in float64) is itself above 3e-6 -- there the bar is 1e-5 against
  # exact arithmetic and 1e-5 + the reference's own error against the reference.
  assert d_gpu_64 < 1e-5
  if d_32_64 < 3e-6 or name not in ILL_CONDITIONED_C1:
    assert d_gpu_32 < 1e-5
  else:
    assert d_32_64 > 3e-6
    assert d_gpu_32 < 1e-5 + 1.01 * d_32_64


def test_ridge_lambda_batch_and_spd_failure(dev):
  rng = np.random.default_rng(9)
  n, c = 3000, 6
  x = rng.standard_normal((n, c)).astype(np.float32)
  x[:, 5] = x[:, 4]                       # exactly collinear channels
  y = (x[:, :1] * 2 + 1).astype(np.float32)
  h = dev.default_handle()
  st = dev.LagStats(c, 0, 2, d=1)
  st.accumulate(h.to_device(x), None, h.to_device(y))
  lams = [1e-3, 0.1, 10.0]
  w, b = st.ridge_solve(lams)
  batches = list(o_lag.minibatches([(x.astype(np.float64), x[:, :1], y.astype(np.float64),
                                     np.zeros((n, 1)))], n, pre=0, post=2))
  for i, lam in enumerate(lams):
    wr, br, _, _, _ = o_reg.linear_regressor_from_batches(batches, lamb=lam)
    np.testing.assert_allclose(w[i].cpu().numpy(), wr, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(b[i].cpu().numpy(), br[0], rtol=2e-4, atol=2e-5)
  with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
    st.ridge_solve([0.0])


@pytest.mark.parametrize('c,pre,post,d,n', [(7, 1, 3, 12, 2500), (3, 0, 4, 70, 3000), (20, 0, 5, 64, 4000)])
def test_ridge_with_wide_targets(dev, c, pre, post, d, n):
  """More outputs than the batched solver's 8 right-hand sides (a forward model: the targets are
  the EEG channels; the reference has no limit, brain_model.py:384-481): the same float64 Cholesky
  through td_chol_factor / td_chol_back, against the reference algorithm on the dense lag matrix."""
  rng = np.random.default_rng(100 + d)
  x = rng.standard_normal((n, c)).astype(np.float32)
  mix = rng.standard_normal((c, d))
  y = (x @ mix + 0.3 * rng.standard_normal((n, d)) + rng.standard_normal((1, d))).astype(np.float32)
  h = dev.default_handle()
  st = dev.LagStats(c, pre, post, d=d)
  st.accumulate(h.to_device(x), None, h.to_device(y))
  lams = [1e-3, 0.1]
  w, b = st.ridge_solve(lams)
  k = c * (pre + 1 + post)
  assert tuple(w.shape) == (2, k, d) and tuple(b.shape) == (2, d)
  batches = list(o_lag.minibatches([(x.astype(np.float64), x[:, :1], y.astype(np.float64),
                                     np.zeros((n, 1)))], n, pre=pre, post=post))
  for i, lam in enumerate(lams):
    wr, br, _, _, _ = o_reg.linear_regressor_from_batches(batches, lamb=lam)
    np.testing.assert_allclose(w[i].cpu().numpy(), wr, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(b[i].cpu().numpy(), br[0], rtol=2e-4, atol=2e-5)
  # the asynchronous and the batched entry points take the same route
  w2, b2, flag = st.ridge_solve_async(lams)
  h.synchronize()
  assert flag() == 0
  np.testing.assert_array_equal(w2.cpu().numpy(), w.cpu().numpy())
  w3, b3 = dev.LagStats.ridge_solve_multi([st, st], lams)
  np.testing.assert_array_equal(w3[1].cpu().numpy(), w.cpu().numpy())
  np.testing.assert_array_equal(b3[0].cpu().numpy(), b.cpu().numpy())
  zero = dev.LagStats(c, pre, post, d=d)
  zero.accumulate(h.to_device(np.zeros((400, c), np.float32)), None, h.to_device(np.zeros((400, d), np.float32)))
  with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
    zero.ridge_solve([0.0])


@pytest.mark.parametrize('c,post,d', [(21, 2, 1), (9, 6, 8), (9, 6, 9), (127, 0, 3), (64, 1, 2), (3, 20, 16)])
def test_ridge_at_size_boundaries(dev, c, post, d):
  """K + 1 at and next to multiples of the solver's 64-wide blocks, 8 and 9 outputs (the batched
  solver's limit and the first wide case): against a float64 solve of the dense system."""
  rng = np.random.default_rng(c * 100 + post * 10 + d)
  n = 3000
  x = rng.standard_normal((n, c)).astype(np.float32)
  xp = np.vstack([x.astype(np.float64), np.zeros((post, c))])
  lagged = np.hstack([xp[l:l + n] for l in range(post + 1)])
  y = (lagged[:, :d] * 0.7 + 0.2 * rng.standard_normal((n, d)) + 1.0).astype(np.float32)
  h = dev.default_handle()
  st = dev.LagStats(c, 0, post, d=d)
  st.accumulate(h.to_device(x), None, h.to_device(y))
  w, b = st.ridge_solve([0.05])
  x1 = np.hstack([lagged, np.ones((n, 1))])
  sol = np.linalg.solve(x1.T @ x1 / n + 0.05 * np.eye(x1.shape[1]), x1.T @ y.astype(np.float64) / n)
  np.testing.assert_allclose(w[0].cpu().numpy(), sol[:-1], rtol=2e-4, atol=2e-5)
  np.testing.assert_allclose(b[0].cpu().numpy(), sol[-1], rtol=2e-4, atol=2e-5)


def test_spd_solve_sizes(dev):
  """The padding's scale.  (The sizes -- partial panels, several right-hand sides, batches -- are rows of
  tests/chol_edges.py: SPD_SIZE_LOOP in SPD_CASES, held by tests/test_gpu_chol_edges.py to a backward error of
  8 x LAPACK's instead of rtol 1e-9.)"""
  import ctypes
  import torch
  h = dev.default_handle()
  rng = np.random.default_rng(11)
  # The identity padding (n is rounded up to whole 64 x 64 tiles) sits on the system's own
  # scale: a system whose diagonal is ~1e15 (a huge ridge lambda) or ~1e-20 is as solvable as
  # np.linalg.solve finds it -- with a fixed 1.0 on the padding's diagonal the first had its
  # padding reported as "not positive definite", the second its tolerance set by the padding.
  for scale in (1e15, 1e-20):
    n, nrhs = 70, 2
    a = rng.standard_normal((1, n, n + 8))
    a = (a @ a.transpose(0, 2, 1) + 0.5 * np.eye(n)) * scale
    rhs = rng.standard_normal((1, n, nrhs))
    want = np.linalg.solve(a, rhs)
    ad = torch.from_numpy(a.copy()).cuda()
    rd = torch.from_numpy(rhs.copy()).cuda()
    h.check(h.lib.td_spd_solve(h.ptr, ctypes.c_void_p(ad.data_ptr()),
                               ctypes.c_void_p(rd.data_ptr()), n, nrhs, 1))
    np.testing.assert_allclose(rd.cpu().numpy(), want, rtol=1e-9, atol=1e-11 / scale)


def test_c2_shape_fit_against_float64_oracle(dev):
  """64 ch x 32 lags (K = 2048 + bias) on a 60k-sample slice of the C2 workload:
  weights against the exact float64 normal equations."""
  from telluride_decoding_amd import synth
  trials = synth.make_trials(2, 6, 10000, 64)
  eeg = np.concatenate([t[0] for t in trials])
  env = np.concatenate([t[1][:, 0:1] for t in trials])
  offs = np.arange(7) * 10000
  h = dev.default_handle()
  st = dev.LagStats(64, 0, 31, d=1)
  st.accumulate(h.to_device(eeg), None, h.to_device(env), offs)
  w, b = st.ridge_solve([0.1])
  w = w.cpu().numpy()[0]
  # float64 oracle on the materialised lag matrix (the reference's arithmetic)
  X = np.concatenate([o_lag.lag_matrix(t[0].astype(np.float64), 0, 31) for t in trials])
  X1 = np.hstack((X, np.ones((X.shape[0], 1))))
  cov = X1.T @ X1 / X1.shape[0] + 0.1 * np.eye(2049)
  sol = np.linalg.solve(cov, X1.T @ env.astype(np.float64) / X1.shape[0])
  # the reference's float32 arithmetic (batch 1000, the survey's C2 batch size)
  files = [(t[0], t[1][:, 1:2], t[1][:, 0:1], t[2]) for t in trials]
  w32, b32, _, _, _ = o_reg.linear_regressor_from_batches(
      o_lag.minibatches(files, 1000, pre=0, post=31), lamb=0.1)
  norm = np.linalg.norm(sol[:-1])
  d_gpu_64 = np.linalg.norm(w - sol[:-1]) / norm
  d_32_64 = np.linalg.norm(w32 - sol[:-1]) / norm
  d_gpu_32 = np.linalg.norm(w - w32) / norm
  print('C2 shape, 60k samples: |gpu-ref64| %.2e  |ref32-ref64| %.2e  |gpu-ref32| %.2e' %
        (d_gpu_64, d_32_64, d_gpu_32))
  parity_log.record('ridge_c2_shape_60k_lowpass', gpu_ref64=d_gpu_64, ref32_ref64=d_32_64,
                    gpu_ref32=d_gpu_32, strict=bool(d_gpu_32 < 1e-5))
  # K = 2049 on 60k LOW-PASS samples is ill-conditioned (the reference's own float32 output is
  # ~1e-4 from exact arithmetic): the bar is 1e-5 against exact arithmetic and the reference's
  # own distance against the reference.  The well-conditioned strict case is the next test.
  assert d_gpu_64 < 1e-5
  assert d_32_64 > 3e-6
  assert d_gpu_32 < 1e-5 + 1.01 * d_32_64
  assert abs(float(b.cpu().numpy()[0, 0]) - sol[-1, 0]) < 1e-5 * max(1.0, np.max(np.abs(sol)))


def test_c2_shape_fit_strict_against_float32_reference(dev):
  """SURVEY 7 "Hard parts": the pass/fail number on a well-conditioned synthetic -- C2 shape
  (64 ch x 32 lags, K = 2049) on 200k samples of white-ish EEG, lambda = 0.1 -- is the STRICT
  north_star bound |gpu - ref32| < 1e-5 relative against the reference's float32 arithmetic
  (materialised lag matrix, per-minibatch float32 x^T x, float32 solve)."""
  rng = np.random.default_rng(2024)
  n_files, n, c, post = 4, 50000, 64, 31
  trf = (rng.standard_normal((post + 1, c)) * np.exp(-np.arange(post + 1) / 8.0)[:, None]).astype(np.float32)
  files = []
  for _ in range(n_files):
    eeg = rng.standard_normal((n, c)).astype(np.float32)
    lagged = o_lag.lag_matrix(eeg, 0, post)
    env = (lagged @ trf.reshape(-1, 1) / 8.0 + 0.5 * rng.standard_normal((n, 1))).astype(np.float32)
    files.append((eeg, env, env, np.zeros((n, 1), np.float32)))
    del lagged
  h = dev.default_handle()
  st = dev.LagStats(c, 0, post, d=1)
  st.accumulate(h.to_device(np.concatenate([f[0] for f in files])), None,
                h.to_device(np.concatenate([f[2] for f in files])), np.arange(n_files + 1) * n)
  w, b = st.ridge_solve([0.1])
  w, b = w.cpu().numpy()[0].astype(np.float64), b.cpu().numpy().astype(np.float64)
  # the reference's arithmetic in float32 and the same in float64, batch 1000
  # (file lengths are multiples of the batch size: batching file by file = batching the stream)
  def batches(dtype):
    for f in files:
      yield from o_lag.minibatches([tuple(a.astype(dtype) for a in f)], 1000, pre=0, post=post)
  w32, b32, _, _, _ = o_reg.linear_regressor_from_batches(batches(np.float32), lamb=0.1)
  assert w32.dtype == np.float32
  w64, b64, _, _, _ = o_reg.linear_regressor_from_batches(batches(np.float64), lamb=0.1)
  scale = np.max(np.abs(w64))
  d_gpu_64 = max(np.max(np.abs(w - w64)), np.max(np.abs(b - b64))) / scale
  d_32_64 = max(np.max(np.abs(w32 - w64)), np.max(np.abs(b32 - b64))) / scale
  d_gpu_32 = max(np.max(np.abs(w - w32)), np.max(np.abs(b - b32))) / scale
  print('C2 shape, 200k white samples: |gpu-ref64| %.2e  |ref32-ref64| %.2e  |gpu-ref32| %.2e' %
        (d_gpu_64, d_32_64, d_gpu_32))
  parity_log.record('ridge_c2_shape_200k_white', gpu_ref64=d_gpu_64, ref32_ref64=d_32_64,
                    gpu_ref32=d_gpu_32, strict=bool(d_gpu_32 < 1e-5))
  assert d_gpu_32 < 1e-5          # north_star, strict
  assert d_gpu_64 < 1e-5


@pytest.mark.gpu
def test_pipelined_fits_equal_serial_fits(dev):
  """pipeline.FitPipeline (accumulate of fit i+1 under the solve of fit i, two streams,
  double-buffered statistics, results handed out two submits later) returns, fit by fit,
  exactly what back-to-back fits return; a singular fit raises when its result is due."""
  import torch
  from telluride_decoding_amd import pipeline
  rng = np.random.default_rng(21)
  h = dev.default_handle()
  c, pre, post, n = 16, 1, 6, 6000
  offs = np.array([0, 2500, 6000], np.int64)
  data = []
  for i in range(5):
    x = rng.standard_normal((n, c)).astype(np.float32)
    y = (x[:, :1] * (i + 1) + 0.1 * rng.standard_normal((n, 1))).astype(np.float32)
    data.append((h.to_device(x), h.to_device(y)))
  torch.cuda.synchronize()
  want = []
  st = dev.LagStats(c, pre, post, d=1)
  for x, y in data:
    st.reset()
    st.accumulate(x, None, y, offs)
    w, b = st.ridge_solve([0.1, 1.0])
    want.append((w.cpu().numpy(), b.cpu().numpy()))
  # a singular fit (all-zero recording, lambda = 0) is reported when its result is due: with n
  # solve streams submit(k) hands out fit k - (n + 1)
  zx = torch.zeros(n, c, device='cuda'); zy = torch.zeros(n, 1, device='cuda')
  for streams in (1, 2):
    pipe = pipeline.FitPipeline(c, pre, post, d=1, solve_streams=streams)
    assert pipe.submit(zx, zy, offs, [0.0]) is None
    for k in range(streams):
      assert pipe.submit(data[k][0], data[k][1], offs, [0.1, 1.0]) is None
    with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
      pipe.submit(data[streams][0], data[streams][1], offs, [0.1, 1.0])      # hands out fit 0
    rest = pipe.flush()
    assert len(rest) == streams + 1
    for k in range(streams + 1):
      np.testing.assert_array_equal(rest[k][0].cpu().numpy(), want[k][0])
    # a singular LAST fit (solved synchronously by flush's latency solver) is reported in order too:
    # the earlier fits' solutions are not lost, and a second flush does not solve it again
    assert pipe.submit(data[0][0], data[0][1], offs, [0.1, 1.0]) is None
    assert pipe.submit(zx, zy, offs, [0.0]) is None
    with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
      pipe.flush()
    assert pipe.pending is None
    kept = pipe.flush()
    assert len(kept) == 1 and pipe.flush() == []
    np.testing.assert_array_equal(kept[0][0].cpu().numpy(), want[0][0])
    del pipe
  # both placements of the y^T x part: on the solve stream (default) and on the accumulate stream
  for on_solve in (True, False):
    pipe = pipeline.FitPipeline(c, pre, post, d=1, targets_on_solve=on_solve)
    got = []
    for x, y in data:
      r = pipe.submit(x, y, offs, [0.1, 1.0])
      if r is not None:
        got.append(r)
    got.extend(pipe.flush())
    assert pipe.flush() == []
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for (w, b), (w0, b0) in zip(got, want):
      np.testing.assert_array_equal(w.cpu().numpy(), w0)
      np.testing.assert_array_equal(b.cpu().numpy(), b0)


def _lag_block_f64(torch, x, offs, a, b, rows_used=None):
  """sum over files of sum_t x~[t+a]^T x~[t+b] in float64 (x~ zero outside the file), the
  (signed lag a, signed lag b) block of X^T X, by direct shifted-slice products."""
  c = x.shape[1]
  out = torch.zeros((c, c), dtype=torch.float64, device=x.device)
  for f in range(len(offs) - 1):
    xf = x[offs[f]:offs[f + 1]].double()
    n = xf.shape[0]
    t_lo = max(0, -a, -b)
    t_hi = min(n if rows_used is None else rows_used[f], n - a, n - b)
    if t_hi > t_lo:
      out += xf[t_lo + a:t_hi + a].T @ xf[t_lo + b:t_hi + b]
  return out


def test_narrow16_long_input_keeps_float32_chains_short(dev):
  """The <= 16-channel streaming accumulate on 2e7 samples (one recording): a wave's sums are one float32
  accumulation chain, capped at 2048 samples by giving long inputs more workgroups -- selected blocks of the
  moments against direct float64 shifted products to 2e-7 of the diagonal, like every other kernel."""
  import torch
  h = dev.default_handle()
  torch.manual_seed(11)
  n, c, post = 20000000, 8, 7
  x = torch.randn(n, c, device='cuda')
  x += 0.4 * torch.roll(x, 1, 0) + 1.5            # correlated in time, not zero-mean: every product counts
  y = (x[:, 2:3] * 0.7 + torch.randn(n, 1, device='cuda'))
  offs = np.array([0, n], np.int64)
  st = dev.LagStats(c, 0, post, d=1)
  st.accumulate(x, None, y, offs)
  m = st.moments()
  xtx, xty = m['xtx'], m['xty']
  scale = float(xtx.abs().max())
  for (la, lb) in ((0, 0), (0, 7), (3, 5)):
    want = _lag_block_f64(torch, x, offs, la, lb)
    got = xtx[la * c:(la + 1) * c, lb * c:(lb + 1) * c]
    assert float((got - want).abs().max()) / scale < 2e-7, (la, lb)
  wy = x[3:].double().T @ y[:n - 3, 0].double()
  assert float((xty[3 * c:4 * c, 0] - wy).abs().max()) / float(xty.abs().max()) < 2e-7


def test_c2_full_size_moments_properties(dev):
  """BASELINE config C2 at full size (64 ch x 1e6 samples, 32 lags, 10 recordings): selected
  blocks of the 2049 x 2049 moment matrix against direct float64 shifted products, exact
  structural properties, additivity over recordings, and a solve whose residual is small."""
  import torch
  h = dev.default_handle()
  torch.manual_seed(5)
  n, c, pre, post = 1000000, 64, 0, 31
  x = torch.randn(n, c, device='cuda')
  x += 0.3 * torch.roll(x, 1, 0) + 0.2 * torch.roll(x, 7, 1)         # temporal and spatial correlation
  y = (x[:, 3:4] * 0.7 + torch.roll(x[:, 10:11], -5, 0) * 0.4 + 0.5 * torch.randn(n, 1, device='cuda'))
  offs = np.arange(11, dtype=np.int64) * 100000
  st = dev.LagStats(c, pre, post, d=1)
  st.accumulate(x, None, y, offs)
  assert st.counts() == (n, 10)
  m = st.moments()
  xtx, xty = m['xtx'], m['xty']
  k = c * 32
  assert torch.equal(xtx, xtx.T)
  assert float(xtx[k, k]) == n
  scale = float(xtx.abs().max())
  for (la, lb) in ((0, 0), (0, 31), (3, 17), (31, 31), (12, 13)):
    want = _lag_block_f64(torch, x, offs, la - pre, lb - pre)
    got = xtx[la * c:(la + 1) * c, lb * c:(lb + 1) * c]
    assert float((got - want).abs().max()) / scale < 2e-7, (la, lb)
  # bias row = lagged column sums, Xty = lagged cross products with y
  for l in (0, 9, 31):
    want = torch.zeros(c, dtype=torch.float64, device='cuda')
    wy = torch.zeros(c, dtype=torch.float64, device='cuda')
    for f in range(10):
      xf = x[offs[f]:offs[f + 1]].double(); yf = y[offs[f]:offs[f + 1], 0].double()
      a = l - pre
      want += xf[a:].sum(0)
      wy += xf[a:].T @ yf[:xf.shape[0] - a]
    assert float((xtx[k, l * c:(l + 1) * c] - want).abs().max()) < 1e-6 * n ** 0.5
    assert float((xty[l * c:(l + 1) * c, 0] - wy).abs().max()) / float(xty.abs().max()) < 2e-7
  # additivity: two halves of the recordings, combined
  a_st, b_st = st.like(), st.like()
  a_st.accumulate(x[:400000], None, y[:400000], offs[:5])
  b_st.accumulate(x[400000:], None, y[400000:], offs[4:] - 400000)
  both = st.like().combine([a_st, b_st])
  m2 = both.moments()
  assert float((m2['xtx'] - xtx).abs().max()) / scale < 1e-7
  # the solve: residual of (XtX/n + lam I) w = Xty/n in float64
  lam = 0.1
  w, b = st.ridge_solve([lam])
  sol = torch.cat([w[0, :, 0].double(), b[0].double()])
  cov = xtx / n + lam * torch.eye(k + 1, dtype=torch.float64, device='cuda')
  res = cov @ sol - xty[:, 0] / n
  assert float(res.abs().max()) / float((xty[:, 0] / n).abs().max()) < 1e-5    # f32 output rounding


def test_long_recording_keeps_the_float32_chains_short(dev):
  """3e6 samples in ONE recording: the lag kernel's workgroups walk their slabs, and a partial
  slab is a float32 sum -- at most four work items long whatever the input's length (every CU
  walking all of its items left the sums of squares of a 4e7-sample call 3e-7 off)."""
  import torch
  h = dev.default_handle()
  torch.manual_seed(11)
  n, c = 3000000, 64
  x = torch.randn(n, c, device='cuda')
  y = torch.randn(n, 1, device='cuda')
  st = dev.LagStats(c, 0, 31, d=1)
  st.accumulate(x, None, y, np.array([0, n], np.int64))
  xtx = st.moments()['xtx']
  want = (x.double() ** 2).sum(0)
  got = torch.diagonal(xtx)[:c]
  assert float(((got - want) / want).abs().max()) < 1.5e-7
  lag5 = (x[:-5].double() * x[5:].double()).sum(0)             # diagonal of the lag-5 block
  got5 = torch.diagonal(xtx[:c, 5 * c:6 * c])
  assert float((got5 - lag5).abs().max()) / float(want.max()) < 2e-8


def test_c3_full_size_cca_moments(dev):
  """BASELINE config C3 at full size (64-ch EEG vs 8-band envelope, 1e6 samples, no lags):
  every CCA moment against a direct float64 product."""
  import torch
  torch.manual_seed(6)
  n = 1000000
  x = torch.randn(n, 64, device='cuda')
  x2 = torch.randn(n, 8, device='cuda') + 0.5 * x[:, :8]
  st = dev.LagStats(64, 0, 0, 8, 0, 0, 0)
  st.accumulate(x, x2, None, np.array([0, 300000, 1000000], np.int64))
  m = st.moments(want_cca=True)
  xd, x2d = x.double(), x2.double()
  for got, want in ((m['xtx'][:64, :64], xd.T @ xd), (m['x2tx2'], x2d.T @ x2d), (m['xtx2'], xd.T @ x2d)):
    assert float((got - want).abs().max()) / float(want.abs().max()) < 2e-7
  # the column sums ride in the Gram matrix (ones column): float32 chains of <= 512 row quads
  # per wave, float64 above -- |error| ~ 1e-3 on sums of 1e6 unit-variance samples, i.e. 1e-9
  # of a sample per row, far below what the float32 products above carry
  assert float((m['sum_x2'] - x2d.sum(0)).abs().max()) < 5e-6 * n ** 0.5
  assert float((m['xtx'][64, :64] - xd.sum(0)).abs().max()) < 5e-6 * n ** 0.5


def test_c3_full_size_fit_and_transform_vs_oracle(dev):
  """BASELINE config C3 END TO END at full size (only its moments were tested, the dense
  stage and the transform at 1e6 ran in bench.py alone): 64-ch EEG against an 8-band envelope, 1e6
  frames in minibatches of 1000, reg = 0.1, 5 components -- cca.BrainModelCCA.fit (one-pass Gram
  kernel + td_cca_solve) and .predict (cca_project_stream_kernel) against the reference's procedure
  in float64 (oracle/cca.py: per-minibatch moments, eig, whitening, svd; cca.py:272-369): canonical
  correlations, rotations up to the joint sign of a component, and a seeded sample of 10 000 rows of the
  transform (cca.py:157-161)."""
  from oracle import cca as o_cca
  from telluride_decoding_amd import brain_data, cca
  rng = np.random.default_rng(33)
  n, c1, c2, dim, batch = 1000000, 64, 8, 5, 1000
  src = rng.standard_normal((n, c2)).astype(np.float32)
  mix = (rng.standard_normal((c2, c1)) * np.linspace(1.0, 0.1, c2)[:, None]).astype(np.float32)
  x = (src @ mix + rng.standard_normal((n, c1)).astype(np.float32)).astype(np.float32)
  x2 = (src + 0.5 * rng.standard_normal((n, c2)).astype(np.float32)).astype(np.float32) + 3.0
  bd = brain_data.TestBrainData('input_1', 'input_2', 100.0, final_batch_size=batch)
  bd.preserve_test_data(x, np.ones((n, 1), np.float32), x2)
  ds = bd.create_dataset('program_test', temporal_context=False)
  model = cca.BrainModelCCA(ds, cca_dims=dim, regularization_lambda=0.1)
  assert model.fit(ds) == {}
  x64, y64 = x.astype(np.float64), x2.astype(np.float64)
  batches = (({'input_1': x64[s:s + batch], 'input_2': y64[s:s + batch]}, None) for s in range(0, n, batch))
  ra, rb, mx, my, e = o_cca.cca_parameters_from_batches(batches, dim, regularization=0.1, mini_batch_count=0)
  np.testing.assert_allclose(model.eigenvalues, e, rtol=1e-5)       # (5.3e-7 measured)
  np.testing.assert_allclose(model.mean_x, mx, atol=2e-6)
  np.testing.assert_allclose(model.mean_y, my, atol=2e-6)
  sign = np.sign(np.sum(np.asarray(model.rot_x, np.float64) * ra, axis=0))
  assert np.all(sign != 0)
  # (a canonical DIRECTION moves by (moment rounding) / (gap to the neighbouring canonical correlations):
  # the last components here are 0.02 apart, so the float32-product moments' 1e-7 shows as ~2e-5 in
  # them -- the reference's own float32 accumulation as much; 1e-4 of the largest entry)
  np.testing.assert_allclose(np.asarray(model.rot_x) * sign, ra, atol=1e-4 * np.max(np.abs(ra)))
  np.testing.assert_allclose(np.asarray(model.rot_y) * sign, rb, atol=1e-4 * np.max(np.abs(rb)))
  out = model.predict(ds)
  assert out.shape == (n, 2 * dim)
  rows = np.sort(rng.choice(n, 10000, replace=False))
  # the transform kernel against float64 with the rotations the fit returned (isolates the kernel) ...
  same = o_cca.cca_transform(x64[rows], y64[rows], model.mean_x, model.mean_y,
                             np.asarray(model.rot_x, np.float64), np.asarray(model.rot_y, np.float64))
  assert float(np.max(np.abs(out[rows] - same)) / np.max(np.abs(same))) < 2e-6
  # ... and end to end against the oracle's own rotations
  want = o_cca.cca_transform(x64[rows], y64[rows], mx, my, ra, rb)
  got = out[rows].astype(np.float64) * np.concatenate((sign, sign))
  err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
  parity_log.record('c3_full_fit_transform', e_rel=float(np.max(np.abs(model.eigenvalues - e) / e)), transform_rel=err,
                    rot_x_maxnorm=hd.maxnorm_rel(np.asarray(model.rot_x) * sign, ra),
                    rot_x_elem=hd.weight_rel(np.asarray(model.rot_x) * sign, ra),
                    rot_y_elem=hd.weight_rel(np.asarray(model.rot_y) * sign, rb))
  assert err < 1e-4


def test_c5_full_subjects_sampled_folds_vs_oracle_refit(dev):
  """BASELINE config C5 with all 32 subjects and all 20 lambdas on a 20 000-frame slice of every
  subject (at full size the sweep was only compared with itself -- PCG against the direct
  solves; the oracle comparison was 5 files x 1 200 frames): three sampled (held-out subject, lambda)
  pairs refit FROM SCRATCH by the reference's procedure in float64 (oracle: lag matrix of the 31
  training subjects in minibatches of 1000, x^T x per minibatch, np.linalg.solve; held-out
  pearson_correlation_first per minibatch, Keras mean; regression.py:151-242, brain_model.py:422-481)
  against the sweep's entries."""
  from oracle import pearson as o_pear
  from telluride_decoding_amd import brain_data, regression, synth
  n_subj, n, c, pre, post, batch = 32, 20000, 64, 0, 31, 1000
  trials = synth.make_trials(9, n_subj, n, c)
  files = [(eeg, env, env[:, 0:1].astype(np.float32), att) for eeg, env, att in trials]
  ds = brain_data.Dataset(files, batch, pre_context=pre, post_context=post)
  lams = list(np.logspace(-6, 3, 20))
  got = regression.jackknife_over_regularizations(ds, lams)
  assert got['all_runs'].shape == (20, n_subj) and np.all(np.isfinite(got['all_runs']))
  f64 = [tuple(a.astype(np.float64) for a in f) for f in files]
  worst = worst_rel = 0.0
  for fold, li in ((0, 12), (17, 7), (31, 18)):            # lambda = 0.48, 2e-3, 336
    train = [f64[g] for g in range(n_subj) if g != fold]
    w, b, _, _, _ = o_reg.linear_regressor_from_batches(
        o_lag.minibatches(train, batch, pre=pre, post=post), lamb=lams[li])
    test_b = list(o_lag.minibatches([f64[fold]], batch, pre=pre, post=post))
    preds = [o_reg.dense_forward(bx['input_1'], w, b) for bx, _ in test_b]
    want = o_pear.evaluate_mean_over_batches(o_pear.pearson_correlation_first, preds, [by for _, by in test_b])
    err = abs(float(got['all_runs'][li, fold]) - float(want))
    worst = max(worst, err)
    worst_rel = max(worst_rel, err / abs(float(want)))
    assert err < 1e-5, (fold, lams[li], float(got['all_runs'][li, fold]), float(want))   # (7e-11 measured)
  # (the sweep's output is one correlation per (lambda, subject): the element-wise distance is the relative one)
  parity_log.record('c5_32_subjects_sampled_refits', max_abs_r_err=worst, pairs=3, elem_rel=worst_rel)


def test_loso_lambda_sweep_matches_refit_from_scratch(dev):
  """Row A10 (config C5's shape, small): regression.jackknife_over_regularizations -- one
  accumulate per file, fold = sum of the others, all lambdas in one batched solve -- against the
  reference's procedure restated with the oracle: refit from scratch for every (lambda, held-out
  file) (regression.py:151-242, 326-420) and score pearson_correlation_first per minibatch."""
  from oracle import pearson as o_pear
  from telluride_decoding_amd import brain_data, regression, synth
  c, pre, post, batch, n_files, n = 8, 1, 4, 100, 5, 1200
  trials = synth.make_trials(77, n_files, n, c)
  files = []
  for eeg, env, att in trials:
    files.append((eeg, env, env[:, 0:1].astype(np.float32), att))
  ds = brain_data.Dataset(files, batch, pre_context=pre, post_context=post)
  lambdas = [1e-3, 0.1, 10.0]
  got = regression.jackknife_over_regularizations(ds, lambdas)
  want = np.zeros((len(lambdas), n_files))
  f64 = [tuple(a.astype(np.float64) for a in f) for f in files]
  for li, lam in enumerate(lambdas):
    for f in range(n_files):
      train = [f64[g] for g in range(n_files) if g != f]
      w, b, _, _, _ = o_reg.linear_regressor_from_batches(
          o_lag.minibatches(train, batch, pre=pre, post=post), lamb=lam)
      test_b = list(o_lag.minibatches([f64[f]], batch, pre=pre, post=post))
      preds = [o_reg.dense_forward(bx['input_1'], w, b) for bx, _ in test_b]
      want[li, f] = o_pear.evaluate_mean_over_batches(o_pear.pearson_correlation_first, preds,
                                                      [by for _, by in test_b])
  np.testing.assert_allclose(got['all_runs'], want, rtol=1e-4, atol=2e-5)
  for li, lam in enumerate(lambdas):
    assert got[lam][0] == pytest.approx(want[li].mean(), abs=2e-5)
    assert got[lam][1] == pytest.approx(want[li].std(), abs=2e-5)


@pytest.mark.parametrize('off', [0, 2, -3])
def test_loso_sweep_ragged_files_and_offset(dev, off):
  """recordings whose lengths are not multiples of the batch size and a non-zero
  input_offset -- the fold's training stream drops only the remainder of the CONCATENATED
  stream (brain_data.py:369-370); 23 lambdas also cross the old 16-column limit of the
  window kernels.  HIP path against from-scratch oracle refits."""
  from telluride_decoding_amd import brain_data, regression
  from tests.test_cpu_host import _loso_case, _loso_refits
  files = _loso_case()
  batch, pre, post = 100, 1, 2
  lambdas = list(np.logspace(-4, 2, 23))
  ds = brain_data.Dataset(files, batch, pre, post, input_offset=off)
  got = regression.jackknife_over_regularizations(ds, lambdas)
  want = _loso_refits(files, batch, pre, post, off, lambdas)
  np.testing.assert_allclose(got['all_runs'], want, rtol=1e-4, atol=3e-5)


def test_loso_scores_every_model_on_its_own_on_the_device(dev):
  """VERDICT r2 #9 on the HIP path: a lambda whose float32 weights underflow to zero predicts
  a constant and scores exactly 0 -- without zeroing the other lambdas of its fold; a constant
  second output zeroes every model (all d outputs of a model enter the zero rule,
  brain_model.py:72-79)."""
  from telluride_decoding_amd import brain_data, regression
  from tests.test_cpu_host import _loso_case, _loso_refits
  files = _loso_case()
  batch, pre, post = 100, 1, 2
  lambdas = [1e-3, 1e60, 0.1]
  got = regression.jackknife_over_regularizations(brain_data.Dataset(files, batch, pre, post),
                                                  lambdas)
  want = _loso_refits(files, batch, pre, post, 0, [1e-3, 0.1])
  np.testing.assert_allclose(got['all_runs'][[0, 2]], want, rtol=1e-4, atol=3e-5)
  np.testing.assert_array_equal(got['all_runs'][1], np.zeros(len(files)))
  flat = [(f[0], f[1], np.concatenate((f[2][:, :1], np.zeros_like(f[2][:, :1])), axis=1), f[3])
          for f in files]
  got = regression.jackknife_over_regularizations(brain_data.Dataset(flat, batch, pre, post),
                                                  [1e-3, 0.1])
  np.testing.assert_array_equal(got['all_runs'], np.zeros((2, len(files))))


def test_accumulate_modes_agree(dev):
  """td_set_accumulate_mode: the float16 two-piece form (default), the bf16 three-piece form and
  the float32 matrix instruction give the same moments -- each well inside what the reference's
  own float32 np.matmul delivers (1e-6 on a 20k-sample sum); the bf16x3 form is the tightest."""
  rng = np.random.default_rng(12)
  h = dev.default_handle()
  n, c = 20000, 64
  x = (rng.standard_normal((n, c)) * np.logspace(-2, 3, c)).astype(np.float32)   # 5 decades of scale
  x[:, 5] += 40.0                                                                # a large offset
  y = (x[:, 3:4] * 0.7 + rng.standard_normal((n, 1))).astype(np.float32)
  xl = o_lag.lag_matrix(x.astype(np.float64), 0, 15)
  xl1 = np.hstack((xl, np.ones((n, 1))))
  want, want_y = xl1.T @ xl1, xl1.T @ y.astype(np.float64)
  scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
  errs = {}
  try:
    for mode in ('f16x2', 'bf16x3', 'f32'):
      h.set_accumulate_mode(mode)
      st = dev.LagStats(c, 0, 15, d=1)
      st.accumulate(h.to_device(x), None, h.to_device(y), [0, n])
      m = st.moments()
      errs[mode] = float(np.max(np.abs(m['xtx'].cpu().numpy() - want) / scale))
      ey = float(np.max(np.abs(m['xty'].cpu().numpy() - want_y) / np.sqrt(np.diag(want)[:, None] * (y.astype(np.float64) ** 2).sum())))
      assert errs[mode] < 2e-7 and ey < 2e-7, (mode, errs[mode], ey)
  finally:
    h.set_accumulate_mode('f16x2')
  assert errs['bf16x3'] <= errs['f16x2']
  with pytest.raises(KeyError):
    h.set_accumulate_mode('fp8')


def test_nan_in_one_channel_poisons_that_channel_only(dev):
  """A NaN (or an infinity) in the input must come out as float32 arithmetic would leave it:
  NaN in every moment that involves the channel, finite numbers elsewhere.  The float16 form
  clamps what it stages (a NaN does not survive v_med3); the channel's maximum remembers it and
  the float64 reduction puts it back."""
  rng = np.random.default_rng(13)
  h = dev.default_handle()
  n, c = 3000, 40
  x = rng.standard_normal((n, c)).astype(np.float32)
  y = rng.standard_normal((n, 1)).astype(np.float32)
  x[1234, 7] = np.nan
  x[77, 30] = np.inf
  st = dev.LagStats(c, 0, 3, d=1)
  st.accumulate(h.to_device(x), None, h.to_device(y), [0, n])
  m = st.moments()
  xtx, xty = m['xtx'].cpu().numpy(), m['xty'].cpu().numpy()
  bad = np.zeros(c * 4 + 1, bool)
  for lag in range(4):
    bad[lag * c + 7] = bad[lag * c + 30] = True
  assert np.all(~np.isfinite(xtx[bad][:, :])) and np.all(~np.isfinite(xtx[:, bad]))
  assert np.all(np.isfinite(xtx[~bad][:, ~bad]))
  assert np.all(~np.isfinite(xty[bad])) and np.all(np.isfinite(xty[~bad]))


def test_tfrecord_ingress_to_trf_fit(dev):
  """F3 end to end on real data: a slice of the reference's MEG recording (148 channels: three
  channel tiles) read by the dependency-free TFRecord parser, z-scored, ridge TRF envelope <-
  MEG with 2 lags (K = 296 < 400 frames), against the oracle on the materialised lag matrix."""
  import os
  from telluride_decoding_amd import brain_data, brain_model, tfrecord
  name = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'meg_subj01_400.tfrecords')
  assert tfrecord.count_tfrecords(name) == (400, False)
  feats = tfrecord.read_file(name, fields=['meg', 'envelope'], verify=True)
  assert feats['meg'].shape == (400, 148)
  x, x2, y, att = tfrecord.select_streams(feats, 'meg', 'envelope')
  x = ((x - x.mean(0)) / x.std(0)).astype(np.float32)
  y = ((y - y.mean(0)) / y.std(0)).astype(np.float32)
  ds = brain_data.Dataset([(x, x[:, :1], y, att)], 100, pre_context=0, post_context=1)
  model = brain_model.BrainModelLinearRegression(ds, regularization_lambda=1.0)
  model.fit(ds)
  f64 = [tuple(a.astype(np.float64) for a in ds.files[0])]
  w, b, _, _, _ = o_reg.linear_regressor_from_batches(
      o_lag.minibatches(f64, 100, pre=0, post=1), lamb=1.0)
  scale = np.max(np.abs(w))
  assert np.max(np.abs(model.w_estimate - w)) / scale < 1e-5
  assert abs(float(model.b_estimate[0]) - float(np.ravel(b)[0])) < 1e-6


def test_accumulate_in_two_parts_equals_one_call(dev):
  """td_stats_accumulate_parts: MAIN then TARGETS (second file batch included) gives bitwise the
  statistics of the single call."""
  rng = np.random.default_rng(31)
  h = dev.default_handle()
  c, pre, post = 16, 2, 5
  x = h.to_device(rng.standard_normal((3000, c)).astype(np.float32))
  y = h.to_device(rng.standard_normal((3000, 2)).astype(np.float32))
  offs1, offs2 = np.array([0, 1200, 2000], np.int64), np.array([0, 1000], np.int64)
  one = dev.LagStats(c, pre, post, d=2)
  one.accumulate(x[:2000], None, y[:2000], offs1)
  one.accumulate(x[2000:], None, y[2000:], offs2)
  two = dev.LagStats(c, pre, post, d=2)
  for xs, ys, offs in ((x[:2000], y[:2000], offs1), (x[2000:], y[2000:], offs2)):
    two.accumulate(xs, None, ys, offs, parts=1)
    two.accumulate(xs, None, ys, offs, parts=2)
  assert one.counts() == two.counts() == (3000, 3)
  m1, m2 = one.moments(), two.moments()
  np.testing.assert_array_equal(m1['xtx'].cpu().numpy(), m2['xtx'].cpu().numpy())
  np.testing.assert_array_equal(m1['xty'].cpu().numpy(), m2['xty'].cpu().numpy())


def test_single_rank_rccl_allreduce_round_trip(dev):
  """The multi-GPU exchange on real RCCL with a one-rank group: pack -> all-reduce (nccl) ->
  unpack leaves the statistics unchanged and the fit identical; the >1-rank protocol itself is
  covered by the two-process gloo test on CPU."""
  import os
  import torch
  import torch.distributed as dist
  from telluride_decoding_amd import distributed
  created = False
  if not dist.is_initialized():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29533')
    os.environ['TD_ALLREDUCE_ALWAYS'] = '1'        # call RCCL although the group has one rank
    dist.init_process_group('nccl', rank=0, world_size=1,
                            device_id=torch.device('cuda', torch.cuda.current_device()))
    created = True
  try:
    rng = np.random.default_rng(41)
    h = dev.default_handle()
    lens = [900, 1100, 700]
    x = h.to_device(rng.standard_normal((sum(lens), 16)).astype(np.float32))
    y = h.to_device(rng.standard_normal((sum(lens), 1)).astype(np.float32))
    offs = np.concatenate(([0], np.cumsum(lens)))
    st = dev.LagStats(16, 1, 6, d=1)
    st.accumulate(x, None, y, offs)
    w0, b0 = st.ridge_solve([0.1])
    m0 = st.moments()['xtx'].clone()
    plan = distributed.ShardPlan(lens, 1)
    distributed.allreduce_stats(st, plan, 0)
    assert st.counts() == (sum(lens), 3)
    np.testing.assert_array_equal(st.moments()['xtx'].cpu().numpy(), m0.cpu().numpy())
    w1, b1 = st.ridge_solve([0.1])
    np.testing.assert_array_equal(w1.cpu().numpy(), w0.cpu().numpy())
    np.testing.assert_array_equal(b1.cpu().numpy(), b0.cpu().numpy())
    # the pipelined form bench.py runs at N > 1: the exchange of fit i rides on the solve
    # stream (its own handle) while accumulate i + 1 runs; every fit equals the serial one
    from telluride_decoding_amd import pipeline
    pipe = pipeline.FitPipeline(
        16, 1, 6, d=1,
        allreduce=lambda s, hs: distributed.allreduce_stats(s, plan, 0, total_frames=sum(lens),
                                                            handle=hs))
    outs = []
    for _ in range(4):
      r = pipe.submit(x, y, offs, [0.1])
      if r is not None:
        outs.append(r)
    outs.extend(pipe.flush())
    assert len(outs) == 4
    for w2, b2 in outs:
      np.testing.assert_array_equal(w2.cpu().numpy(), w0.cpu().numpy())
      np.testing.assert_array_equal(b2.cpu().numpy(), b0.cpu().numpy())
    # the same exchange through torch.distributed's own all-reduce (the A/B switch)
    os.environ['TD_ALLREDUCE_TORCH'] = '1'
    try:
      distributed.allreduce_stats(st, plan, 0)
    finally:
      del os.environ['TD_ALLREDUCE_TORCH']
    np.testing.assert_array_equal(st.moments()['xtx'].cpu().numpy(), m0.cpu().numpy())
    assert distributed._comms, 'the C-ABI communicator was not used'
  finally:
    distributed.close_native_comms()
    if created:
      dist.destroy_process_group()


def test_c_abi_stats_allreduce_needs_no_torch_distributed(dev):
  """SURVEY 8b(3) `stats_allreduce(handle, rccl_comm)` as a C export: a binding
  without PyTorch makes the communicator itself (td_rccl_unique_id -> td_rccl_comm_create) and
  calls td_stats_allreduce on raw symbols; on one rank the sum over ranks is the identity, the
  boundary slots land where `file_slot` says, the frame count is taken from the buffer."""
  import ctypes
  rng = np.random.default_rng(43)
  h = dev.default_handle()
  lib = h.lib
  ident = (ctypes.c_char * 128)()
  assert lib.td_rccl_unique_id(h.ptr, ident) == 0, lib.td_last_error(h.ptr)
  comm = ctypes.c_void_p()
  assert lib.td_rccl_comm_create(h.ptr, 1, 0, ident, ctypes.byref(comm)) == 0, lib.td_last_error(h.ptr)
  n = ctypes.c_int(0)
  assert lib.td_rccl_comm_count(h.ptr, comm, ctypes.byref(n)) == 0 and n.value == 1
  try:
    lens = [800, 1000]
    x = h.to_device(rng.standard_normal((sum(lens), 40)).astype(np.float32))
    x2 = h.to_device(rng.standard_normal((sum(lens), 3)).astype(np.float32))
    y = h.to_device(rng.standard_normal((sum(lens), 2)).astype(np.float32))
    st = dev.LagStats(40, 0, 7, 3, 1, 1, 2)
    st.accumulate(x, x2, y, np.concatenate(([0], np.cumsum(lens))))
    want = {k: v.clone() for k, v in st.moments(want_cca=True).items() if v is not None}
    # two of four slots are this rank's (slots 1..2); frame count read back from the buffer
    assert lib.td_stats_allreduce(h.ptr, st.ptr, comm, 4, 1, -1) == 0, lib.td_last_error(h.ptr)
    assert st.counts() == (sum(lens), 4)
    # the statistics are unchanged where they were, and the two foreign slots are empty: the
    # moments (which sum the edge corrections over all four slots) are the same
    got = st.moments(want_cca=True)
    for k, v in want.items():
      np.testing.assert_array_equal(got[k].cpu().numpy(), v.cpu().numpy())
    # a raw buffer: in-place sum over one rank = identity
    buf = h.to_device(rng.standard_normal((1000, 1)), np.float64)
    ref = buf.clone()
    assert lib.td_allreduce_f64(h.ptr, ctypes.c_void_p(buf.data_ptr()), buf.numel(), comm) == 0
    h.synchronize()
    np.testing.assert_array_equal(buf.cpu().numpy(), ref.cpu().numpy())
    # errors: a slot range that does not fit, a NULL communicator
    assert lib.td_stats_allreduce(h.ptr, st.ptr, comm, 4, 3, -1) == -1
    assert lib.td_stats_allreduce(h.ptr, st.ptr, None, 4, 0, -1) == -1
  finally:
    assert lib.td_rccl_comm_destroy(h.ptr, comm) == 0


def _lw_moment_numpy(batches):
  """np.sum(sum_x2tx2) exactly as brain_model.py:429-443 accumulates it (float64)."""
  sum_x, n, tot = 0.0, 0, 0.0
  for x in batches:
    x = np.asarray(x, np.float64)
    n += x.shape[0]
    sum_x = sum_x + x.sum(axis=0, keepdims=True)
    x2 = (x - sum_x / n) ** 2
    tot += float((x2.sum(axis=1) ** 2).sum())      # = np.sum(x2.T @ x2)
  return tot


@pytest.mark.gpu
@pytest.mark.parametrize('c,pre,post,off,lens,batch', [
    (5, 2, 3, 0, (700, 333, 1021), 100),
    (16, 0, 7, 2, (900, 0, 901), 64),
    (64, 0, 31, 0, (3000, 2500), 500),
    (3, 1, 1, -3, (640, 129, 7), 50),
    (70, 0, 0, 0, (1000,), 300),           # shorter last minibatch (1000 = 3 * 300 + 100)
])
def test_shrinkage_moment_matches_reference_accumulation(dev, c, pre, post, off, lens, batch):
  """Row F2: the Ledoit-Wolf moment of brain_model.py:440-443 (running mean including the
  current minibatch) from the raw recordings, against the literal minibatch loop."""
  rng = np.random.default_rng(99 + c)
  files = [(rng.standard_normal((n, c)) + 0.7).astype(np.float32) for n in lens]
  streams = []
  for x in files:
    a = np.zeros((x.shape[0], 1), np.float32)
    xl, _, _, _ = o_lag.window_streams(x, a, a, a, pre=pre, post=post, input_offset=off)
    streams.append(xl)
  stream = np.concatenate(streams)
  drop = batch != 300
  total = (stream.shape[0] // batch) * batch if drop else stream.shape[0]
  want = _lw_moment_numpy([stream[i:i + batch] for i in range(0, total, batch)])
  h = dev.default_handle()
  xd = h.to_device(np.concatenate(files))
  offs = np.concatenate(([0], np.cumsum(lens)))
  used = None
  if drop:
    used, left = [], total
    for s in streams:
      used.append(min(left, s.shape[0]))
      left -= used[-1]
  got = dev.shrinkage_moment(xd, offs, pre, post, batch, input_offset=off, rows_used=used, handle=h)
  assert abs(got - want) <= 2e-6 * abs(want)


@pytest.mark.gpu
def test_ledoit_wolf_regression_matches_reference_golden(dev):
  """lamb = -1, use_ridge = False against the output of the reference itself (g2_ridge.npz,
  'shrink_lw') and, on a lagged case, against the oracle in float64."""
  from telluride_decoding_amd import brain_data, brain_model
  g = golden('g2_ridge')
  bd = brain_data.TestBrainData('eeg', 'env', 100.0, final_batch_size=100)
  for i in range(3):
    bd.add_file(g['c1_eeg%d' % i], g['c1_env%d' % i][:, 0:1])
  w, b, cx, _, sh = brain_model.calculate_linear_regressor_parameters_from_dataset(
      bd.create_dataset('train'), lamb=-1, use_ridge=False)
  assert abs(sh - float(g['shrink_lw_shrinkage'])) < 1e-3 * abs(float(g['shrink_lw_shrinkage']))
  np.testing.assert_allclose(w, g['shrink_lw_w'], rtol=1e-3, atol=2e-5)
  np.testing.assert_allclose(cx, g['shrink_lw_cov_x'], rtol=1e-4, atol=1e-4)
  # generic-iterable entry point (already lagged minibatches), float64 oracle
  rng = np.random.default_rng(5)
  files = []
  for n in (1500, 801):
    x = rng.standard_normal((n, 6)).astype(np.float32)
    y = (x[:, :1] * 0.5 + rng.standard_normal((n, 1)) * 0.1).astype(np.float32)
    files.append((x, y, y, np.zeros((n, 1), np.float32)))
  batches = list(o_lag.minibatches(files, 100, pre=1, post=2))
  f64 = [({'input_1': bx['input_1'].astype(np.float64)}, by.astype(np.float64)) for bx, by in batches]
  w0, b0, _, _, sh0 = o_reg.linear_regressor_from_batches(f64, lamb=-1, use_ridge=False)
  w1, b1, _, _, sh1 = brain_model.calculate_linear_regressor_parameters_from_dataset(
      batches, lamb=-1, use_ridge=False)
  assert abs(sh1 - sh0) < 1e-4 * abs(sh0)
  # the bound is the reference's own arithmetic: the same procedure on the float32 minibatches
  w32, b32, _, _, _ = o_reg.linear_regressor_from_batches(batches, lamb=-1, use_ridge=False)
  ref32 = hd.maxnorm_rel(np.vstack((w32, b32)), np.vstack((w0, b0)))
  err = hd.maxnorm_rel(np.vstack((w1, b1)), np.vstack((w0, b0)))
  parity_log.record('ledoit_wolf_iterable', maxnorm_rel=err, elem_rel=hd.weight_rel(w1, w0), reference_fp32_rel=ref32,
                    shrinkage_rel=abs(sh1 - sh0) / abs(sh0))
  assert err < ref32 + 1e-5, (err, ref32)


@pytest.mark.gpu
@pytest.mark.parametrize('n,nrhs', [(1, 1), (5, 2), (15, 1), (16, 2), (17, 1), (31, 1), (32, 2), (33, 1), (70, 1), (300, 3),
                                    (300, 70), (513, 1), (1030, 2), (1600, 1), (2049, 1), (2600, 1), (3100, 2), (8200, 1)])
def test_general_solve_indefinite_and_singular(dev, n, nrhs):
  """td_general_solve = np.linalg.solve (brain_model.py:477) for the branch whose matrix can be
  indefinite; a singular matrix raises like NumPy does.  (Sizes on both sides of the panel widths 16 / 32, one to six
  rows per thread of the register-resident panel -- 513 .. 2600 --, 3100: the streamed panel of larger systems, and
  8200: beyond the 64 KB of dynamic LDS a kernel has by default.)"""
  import torch
  rng = np.random.default_rng(n)
  if n <= 4000:
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    eig = np.linspace(-3.0, 5.0, n) if n > 1 else np.array([-2.0])
    a = (q * eig) @ q.T + 1e-3 * rng.standard_normal((n, n))      # indefinite, not symmetric
  else:
    a = rng.standard_normal((n, n))                               # (no QR of a matrix that size: seconds of host time)
    a = a + a.T + 1e-3 * rng.standard_normal((n, n))
  b = rng.standard_normal((n, nrhs))
  h = dev.default_handle()
  got = dev.general_solve(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), handle=h)
  want = np.linalg.solve(a, b)
  np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-9 * max(1, n // 100), atol=1e-10 * max(1, n // 100))
  if 1 < n <= 4000:
    a[:, 1] = 0.0                                  # an exactly zero pivot column
    with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
      np.linalg.solve(a, b)
    with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
      dev.general_solve(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), handle=h)


@pytest.mark.parametrize('world,shape', [(2, 'narrow'), (3, 'narrow'), (8, 'narrow'),
                                         (2, 'c2'), (8, 'c2'), (5, 'wide'), (3, 'n16')])
def test_time_range_shards_equal_whole_recordings(dev, world, shape):
  """Strong-scaling unit of SURVEY 8e: ranks share long recordings by TIME RANGE (piece = range
  + halo; zero extension and edge corrections only at true ends; one packed all-reduce with
  per-recording boundary slots).  Summing the ranks' packed statistics reproduces the
  single-GPU statistics, for the regression moments and for lagged CCA moments, including a
  recording shorter than a range, a dropped remainder and cuts that fall inside the context."""
  from telluride_decoding_amd import distributed
  rng = np.random.default_rng(40 + world)
  if shape == 'narrow':        # float32 accumulate kernel, lagged CCA moments too
    c1, pre, post, c2, pre2, post2, d = 8, 2, 5, 3, 1, 2, 2
    lens = (1900, 130, 2777, 640)
  elif shape == 'n16':         # the <= 16-channel streaming kernel (ranges that begin inside a recording)
    c1, pre, post, c2, pre2, post2, d = 12, 1, 6, 0, 0, 0, 2
    lens = (1900, 130, 2777, 640)
  elif shape == 'c2':          # the bf16x3 accumulate kernel at the C2 channel / lag counts
    c1, pre, post, c2, pre2, post2, d = 64, 0, 31, 0, 0, 0, 1
    lens = (9000, 150, 20011, 4100)
  else:                        # its 192-row geometry (40 lags), 50 channels
    c1, pre, post, c2, pre2, post2, d = 50, 30, 9, 0, 0, 0, 1
    lens = (7000, 2600, 333)
  xs = [rng.standard_normal((n, c1)).astype(np.float32) for n in lens]
  x2s = [rng.standard_normal((n, max(c2, 1))).astype(np.float32) for n in lens]
  ys = [rng.standard_normal((n, d)).astype(np.float32) for n in lens]
  h = dev.default_handle()
  offs = np.concatenate(([0], np.cumsum(lens)))
  batch = 100
  cca = c2 > 0
  rows_used = list(lens)
  rows_used[-1] -= sum(lens) % batch
  whole = dev.LagStats(c1, pre, post, c2, pre2, post2, d)
  whole.accumulate(h.to_device(np.concatenate(xs)),
                   h.to_device(np.concatenate(x2s)) if cca else None,
                   h.to_device(np.concatenate(ys)), offs, rows_used=rows_used)
  want = whole.moments(want_cca=cca)
  plan = distributed.TimeShardPlan(lens, world, halo=whole.pre1 + whole.post1 + whole.pre2 +
                                   whole.post2 + 1, batch_size=batch)
  assert plan.total_frames == sum(rows_used) == sum(plan.frames_of(r) for r in range(world))
  buf = None
  for rank in range(world):
    st = whole.like()
    distributed.accumulate_time_shard(
        st, plan, rank, lambda f, a, b: (h.to_device(xs[f][a:b]),
                                         h.to_device(x2s[f][a:b]) if cca else None,
                                         h.to_device(ys[f][a:b])))
    assert st.counts()[0] == plan.frames_of(rank)
    part = st.pack(plan.total_files, plan.slot_of(rank))
    buf = part if buf is None else buf + part          # what the all-reduce(sum) computes
  merged = whole.like()
  merged.unpack(buf, plan.total_files, plan.total_frames)
  assert merged.counts() == whole.counts()
  got = merged.moments(want_cca=cca)
  scale = float(want['xtx'].abs().max())             # the diagonal: sum of squares of a channel
  for key in (('xtx', 'xty', 'x2tx2', 'xtx2', 'sum_x2') if cca else ('xtx', 'xty')):
    a, b = got[key].cpu().numpy(), want[key].cpu().numpy()
    # (a cut moves the boundaries of the kernel's float32 product chains -- <= 2048 samples each,
    # summed in float64 -- so the sums agree to float32-chain rounding, ~1e-8 of the diagonal)
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-7 * scale, err_msg=key)
  w1, b1 = merged.ridge_solve([0.1])
  w0, b0 = whole.ridge_solve([0.1])
  np.testing.assert_allclose(w1.cpu().numpy(), w0.cpu().numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('c,pre,post,d', [(64, 0, 31, 1), (16, 1, 6, 2), (40, 0, 9, 1), (24, 0, 15, 1)])
def test_deferred_finalize_equals_the_call_that_finalizes_itself(dev, c, pre, post, d):
  """td_stats_accumulate_parts(parts | TD_ACC_DEFER) + td_stats_complete on ANOTHER handle's stream: the same
  statistics, bit for bit, as the call that finalizes itself -- with a second deferred call of the first handle
  (other data: it overwrites the handle's scratch and channel tables) queued in between; a reader that
  forgets the completion gets it done for it; a reset drops a pending finalize; shapes the deferral does not
  cover (virtual images: 24 channels x 16 lags) finalize inside the call."""
  import torch
  rng = np.random.default_rng(5 + c)
  h = dev.default_handle()
  lens = (3000, 129, 5000)
  n = sum(lens)
  offs = np.concatenate(([0], np.cumsum(lens)))
  xa = h.to_device((rng.standard_normal((n, c)) * np.logspace(-1, 1, c)).astype(np.float32))
  ya = h.to_device(rng.standard_normal((n, d)).astype(np.float32))
  xb = h.to_device((rng.standard_normal((n, c)) * 30).astype(np.float32))
  yb = h.to_device(rng.standard_normal((n, d)).astype(np.float32))
  want_a = dev.LagStats(c, pre, post, d=d); want_a.accumulate(xa, None, ya, offs)
  want_b = dev.LagStats(c, pre, post, d=d); want_b.accumulate(xb, None, yb, offs)
  ma, mb = want_a.moments(), want_b.moments()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    h2 = dev.Handle()
  torch.cuda.synchronize()
  sa, sb = dev.LagStats(c, pre, post, d=d), dev.LagStats(c, pre, post, d=d)
  sa.accumulate(xa, None, ya, offs, parts=3 | 8)
  sb.accumulate(xb, None, yb, offs, parts=3 | 8)         # (the handle's scratch now belongs to this call)
  side.wait_stream(torch.cuda.current_stream())          # (the caller orders the streams, as for any use of sa there)
  with torch.cuda.stream(side):
    sa.complete(handle=h2)
    got_a = sa.moments()                                 # (on h2's stream, behind the finalize)
  got_b = sb.moments()                                   # nobody completed sb: the reader does
  torch.cuda.synchronize()
  for key in ('xtx', 'xty'):
    np.testing.assert_array_equal(got_a[key].cpu().numpy(), ma[key].cpu().numpy(), err_msg=key)
    np.testing.assert_array_equal(got_b[key].cpu().numpy(), mb[key].cpu().numpy(), err_msg=key)
  assert sa.counts() == want_a.counts()
  # a second deferred call adds to the first (completed implicitly by the accumulate entry point)
  sa.accumulate(xb, None, yb, offs, parts=3 | 8)
  sa.complete()
  both = sa.moments()
  np.testing.assert_allclose(both['xtx'].cpu().numpy(), ma['xtx'].cpu().numpy() + mb['xtx'].cpu().numpy(),
                             rtol=1e-9, atol=1e-9)
  # a reset drops a pending finalize: the statistics then hold the next call's sums only
  sb.reset()
  sb.accumulate(xa, None, ya, offs, parts=3 | 8)
  sb.reset()
  sb.accumulate(xb, None, yb, offs)
  np.testing.assert_array_equal(sb.moments()['xtx'].cpu().numpy(), mb['xtx'].cpu().numpy())
  w1, b1 = sb.ridge_solve([0.5])
  w0, b0 = want_b.ridge_solve([0.5])
  np.testing.assert_array_equal(w1.cpu().numpy(), w0.cpu().numpy())
  del h2


def test_pipeline_refuses_a_solve_partition_that_splits_an_xcd(dev):
  """FitPipeline(solve_cus=...): a CU mask holds whole XCDs (a fraction of one runs the other partition at the
  pace of that XCD's doubled-up CUs: 1.3-1.4 ms per pipelined C2 fit at 48 / 56 / 72 CUs against 0.83 at 64)."""
  import torch
  from telluride_decoding_amd import pipeline
  n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
  if n_cu != 256:
    pytest.skip('measured on the 256 CUs (8 XCDs of 32) of an MI355X, not on %d' % n_cu)
  with pytest.raises(ValueError, match='whole number of XCDs'):
    pipeline.FitPipeline(16, 0, 3, d=1, solve_cus=n_cu // 8 + n_cu // 16)
  pipe = pipeline.FitPipeline(16, 0, 3, d=1, solve_cus=n_cu // 8)
  assert pipe.defer_finalize
  del pipe


def test_narrow16_strided_inputs_parts_and_tiled_path(dev):
  """The <= 16-channel streaming accumulate (lagcov_narrow16_kernel): inputs that are column slices of
  wider arrays (row pitch > channels), the covariance part and the targets part of a call queued apart
  (bit-identical to the call that carries both), and the tiled kernels it replaces (td_set_option
  "narrow16" 0) agree with it to float32-chain rounding."""
  import torch
  rng = np.random.default_rng(77)
  h = dev.default_handle()
  c, pre, post, d = 11, 2, 9, 3
  lens = (1500, 37, 4100)
  n = sum(lens)
  offs = np.concatenate(([0], np.cumsum(lens)))
  wide = h.to_device(rng.standard_normal((n, 24)).astype(np.float32))
  wide_y = h.to_device(rng.standard_normal((n, 7)).astype(np.float32))
  x, y = wide[:, 5:5 + c], wide_y[:, 2:2 + d]
  assert x.stride(0) == 24 and y.stride(0) == 7
  both = dev.LagStats(c, pre, post, d=d)
  both.accumulate(x, None, y, offs, input_offset=1)
  m3 = both.moments()
  dense = dev.LagStats(c, pre, post, d=d)
  dense.accumulate(x.contiguous(), None, y.contiguous(), offs, input_offset=1)
  md = dense.moments()
  apart = dev.LagStats(c, pre, post, d=d)
  apart.accumulate(x, None, y, offs, input_offset=1, parts=1)
  apart.accumulate(x, None, y, offs, input_offset=1, parts=2)
  ma = apart.moments()
  for key in ('xtx', 'xty'):
    np.testing.assert_array_equal(m3[key].cpu().numpy(), md[key].cpu().numpy(), err_msg=key)
    np.testing.assert_array_equal(m3[key].cpu().numpy(), ma[key].cpu().numpy(), err_msg=key)
  h.set_option('narrow16', 0)
  try:
    tiled = dev.LagStats(c, pre, post, d=d)
    tiled.accumulate(x, None, y, offs, input_offset=1)
    mt = tiled.moments()
  finally:
    h.set_option('narrow16', 1)
  scale = float(m3['xtx'].abs().max())
  for key in ('xtx', 'xty'):
    np.testing.assert_allclose(m3[key].cpu().numpy(), mt[key].cpu().numpy(), rtol=0, atol=3e-7 * scale,
                               err_msg=key)
  # ... and a second accumulate call adds to the first (the finalize launch accumulates)
  both.accumulate(x, None, y, offs, input_offset=1)
  m6 = both.moments()
  np.testing.assert_allclose(m6['xtx'].cpu().numpy(), 2 * m3['xtx'].cpu().numpy(), rtol=1e-12, atol=0)
  np.testing.assert_allclose(m6['xty'].cpu().numpy(), 2 * m3['xty'].cpu().numpy(), rtol=1e-12, atol=0)


def test_ridge_solve_multi_equals_single_solves(dev):
  """td_ridge_solve_multi: (statistics x lambdas) in one batched factorisation gives exactly
  the weights of the per-statistics solves; a singular member fails the batch."""
  rng = np.random.default_rng(8)
  h = dev.default_handle()
  lams = [1e-3, 0.1, 10.0]
  sts = []
  for i in range(4):
    x = rng.standard_normal((1500 + 100 * i, 12)).astype(np.float32)
    y = (x[:, :2] * (i + 1) + 0.1 * rng.standard_normal((x.shape[0], 2))).astype(np.float32)
    st = dev.LagStats(12, 2, 3, d=2)
    st.accumulate(h.to_device(x), None, h.to_device(y))
    sts.append(st)
  w, b = dev.LagStats.ridge_solve_multi(sts, lams)
  assert tuple(w.shape) == (4, 3, 72, 2) and tuple(b.shape) == (4, 3, 2)
  for i, st in enumerate(sts):
    w1, b1 = st.ridge_solve(lams)
    np.testing.assert_array_equal(w[i].cpu().numpy(), w1.cpu().numpy())
    np.testing.assert_array_equal(b[i].cpu().numpy(), b1.cpu().numpy())
  w2, b2, flag = dev.LagStats.ridge_solve_multi(sts, lams, wait=False)
  h.synchronize()
  assert flag() == 0
  np.testing.assert_array_equal(w2.cpu().numpy(), w.cpu().numpy())
  zero = dev.LagStats(12, 2, 3, d=2)
  zero.accumulate(h.to_device(np.zeros((500, 12), np.float32)), None,
                  h.to_device(np.zeros((500, 2), np.float32)))
  with pytest.raises(np.linalg.LinAlgError, match='Singular matrix'):
    dev.LagStats.ridge_solve_multi(sts[:2] + [zero], [0.0])


def _loso_case(dev, rng, n_files, c, pre, post, d, alike=True, frames=1200):
  """Per-file statistics, the folds' training sums and the total for a leave-one-out sweep."""
  h = dev.default_handle()
  mix = rng.standard_normal((c, c)) * 0.3 + np.eye(c)
  files = []
  for i in range(n_files):
    n = frames + 37 * i
    x = (rng.standard_normal((n, c)) @ (mix if alike else mix * (1 + 3 * (i % 2)))).astype(np.float32)
    y = (x[:, :d] * 0.5 + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
    st = dev.LagStats(c, pre, post, d=d)
    st.accumulate(h.to_device(x), None, h.to_device(y))
    files.append(st)
  proto = files[0]
  folds = [proto.like().combine([s for g, s in enumerate(files) if g != f]) for f in range(n_files)]
  total = proto.like().combine(files)
  return files, folds, total


@pytest.mark.parametrize('c,pre,post,d,n_files,frames', [
    (8, 0, 7, 1, 5, 1200), (12, 2, 3, 2, 4, 1200), (64, 0, 31, 1, 6, 6000)])
def test_loso_pcg_solver_equals_the_direct_solves(dev, c, pre, post, d, n_files, frames):
  """td_ridge_solve_loso (preconditioned CG over all folds x lambdas, one Cholesky factor per
  lambda of the total covariance) against td_ridge_solve_multi (one factorisation per system):
  the same float32 weights up to the last bits, for well and badly conditioned lambdas, ragged
  file lengths, several outputs, and n = 2049 (padding to 2112)."""
  rng = np.random.default_rng(31)
  _, folds, total = _loso_case(dev, rng, n_files, c, pre, post, d, frames=frames)
  lams = [1e-6, 1e-2, 1.0, 1e3]
  out = dev.LagStats.ridge_solve_loso(total, folds, lams)
  assert out is not None, 'the PCG solver reported no convergence on a well-posed sweep'
  w, b, iters = out
  assert 1 <= iters <= 40
  w0, b0 = dev.LagStats.ridge_solve_multi(folds, lams)
  assert tuple(w.shape) == tuple(w0.shape) and tuple(b.shape) == tuple(b0.shape)
  w, w0, b, b0 = (t.cpu().numpy().astype(np.float64) for t in (w, w0, b, b0))
  for li in range(len(lams)):
    scale = np.abs(w0[:, li]).max()
    assert np.abs(w[:, li] - w0[:, li]).max() <= 2e-6 * scale, (lams[li], iters)
    assert np.abs(b[:, li] - b0[:, li]).max() <= 2e-6 * max(scale, np.abs(b0[:, li]).max())


def test_loso_pcg_solver_reports_when_it_cannot_converge(dev):
  """One iteration is not enough: status 1 -> None, and regression.jackknife_over_regularizations
  then takes the direct batched solve (same results as with the solver switched off)."""
  from telluride_decoding_amd import brain_data, regression
  rng = np.random.default_rng(32)
  _, folds, total = _loso_case(dev, rng, 4, 8, 0, 7, 1, alike=False)
  assert dev.LagStats.ridge_solve_loso(total, folds, [1e-6, 1.0], max_iter=1, tol=1e-14) is None
  # a preconditioner that is not positive definite (all-zero data, lambda = 0) is reported too
  h = dev.default_handle()
  zeros = []
  for _ in range(3):
    st = dev.LagStats(8, 0, 3, d=1)
    st.accumulate(h.to_device(np.zeros((400, 8), np.float32)), None, h.to_device(np.zeros((400, 1), np.float32)))
    zeros.append(st)
  zf = [zeros[0].like().combine([s for g, s in enumerate(zeros) if g != f]) for f in range(3)]
  assert dev.LagStats.ridge_solve_loso(zeros[0].like().combine(zeros), zf, [0.0]) is None
  # the sweep end to end with and without the solver
  c, n = 6, 900
  trials = []
  for i in range(5):
    x = rng.standard_normal((n + 10 * i, c)).astype(np.float32)
    y = (x[:, :1] + 0.2 * rng.standard_normal((x.shape[0], 1))).astype(np.float32)
    trials.append((x, y, y, np.zeros((x.shape[0], 1), np.float32)))
  ds = brain_data.Dataset(trials, 100, pre_context=0, post_context=3)
  lams = [1e-4, 1e-1, 10.0]
  with_pcg = regression.jackknife_over_regularizations(ds, lams)
  old = regression.USE_PCG
  regression.USE_PCG = False
  try:
    direct = regression.jackknife_over_regularizations(ds, lams)
  finally:
    regression.USE_PCG = old
  np.testing.assert_allclose(with_pcg['all_runs'], direct['all_runs'], rtol=0, atol=2e-6)
  assert regression.LAST_SWEEP['solver'] == 'direct'
  # ... and in chunks of two folds (a workspace budget that small)
  old_bytes = regression.SOLVE_WORKSPACE_BYTES
  n1 = c * 4 + 1
  n_pad = 64
  regression.SOLVE_WORKSPACE_BYTES = len(lams) * (n_pad * n_pad + n_pad * 64 + 16 * 4096) * 8 + n1 * n_pad * 8 + \
      2 * (n1 * n_pad * 8 + 9 * len(lams) * n_pad * 8) + 8
  try:
    assert regression._pcg_chunk(5, len(lams), n1, 1) == 2
    chunked = regression.jackknife_over_regularizations(ds, lams)
  finally:
    regression.SOLVE_WORKSPACE_BYTES = old_bytes
  assert regression.LAST_SWEEP['solver'] == 'pcg'
  np.testing.assert_allclose(chunked['all_runs'], with_pcg['all_runs'], rtol=0, atol=1e-9)


def test_loso_sweep_at_c5_size_pcg_equals_direct(dev):
  """BASELINE config C5 at full size (32 subjects x 31 250 samples x 64 ch, 32 lags, 20 lambdas =
  640 fits): the preconditioned-CG sweep against the direct batched Cholesky sweep -- the same
  held-out correlations to 2e-6 for every (lambda, subject), the same best lambda; every subject
  decodes (mean r > 0.9 at the best lambda: the synthetic EEG is a filtered envelope + noise)."""
  from telluride_decoding_amd import brain_data, regression, synth
  n_subj, n, c = 32, 31250, 64
  trials = synth.make_trials(5, n_subj, n, c)
  files = [(eeg, env, env[:, 0:1].astype(np.float32), att) for eeg, env, att in trials]
  ds = brain_data.Dataset(files, 1000, pre_context=0, post_context=31)
  lams = list(np.logspace(-6, 3, 20))
  got = regression.jackknife_over_regularizations(ds, lams)
  assert regression.LAST_SWEEP['solver'] == 'pcg' and 1 <= regression.LAST_SWEEP['iterations'] <= 20
  old = regression.USE_PCG
  regression.USE_PCG = False
  try:
    want = regression.jackknife_over_regularizations(ds, lams)
  finally:
    regression.USE_PCG = old
  assert got['all_runs'].shape == (20, n_subj)
  assert np.all(np.isfinite(got['all_runs']))
  np.testing.assert_allclose(got['all_runs'], want['all_runs'], rtol=0, atol=2e-6)
  best = max((v[0], k) for k, v in got.items() if k != 'all_runs')
  best_direct = max((v[0], k) for k, v in want.items() if k != 'all_runs')
  assert best[1] == best_direct[1] and best[0] > 0.9


def test_pooled_statistics_memory_comes_back_fresh(dev):
  """td_stats_destroy hands the device memory to a pool inside the library (an event marks when
  it is free) and td_stats_create takes blocks of the same size from it: a recycled block must
  read as new statistics, also when the old object was destroyed with work still queued on it and
  when the new one lives on another handle (another stream)."""
  rng = np.random.default_rng(77)
  h = dev.default_handle()
  x = h.to_device(rng.standard_normal((20000, 64)).astype(np.float32))
  y = h.to_device(rng.standard_normal((20000, 1)).astype(np.float32))
  ref = dev.LagStats(64, 0, 31, d=1)
  ref.accumulate(x, None, y)
  want = {k: v.cpu().numpy() for k, v in ref.moments().items() if v is not None}
  h2 = dev.Handle()
  for rep in range(6):
    a = dev.LagStats(64, 0, 31, d=1)
    for _ in range(3):
      a.accumulate(x, None, y)               # queued work ...
    del a                                    # ... and the object goes while it runs
    b = dev.LagStats(64, 0, 31, d=1, handle=h2 if rep % 2 else h)
    frames, nfiles = b.counts()
    assert frames == 0 and nfiles == 0
    b.accumulate(x, None, y)
    got = b.moments()
    for k, v in want.items():
      np.testing.assert_array_equal(got[k].cpu().numpy(), v)
    del b


def test_bf16_mfma_probe_reports_a_rate(dev):
  """td_probe_bf16_mfma (bench.py's sustained-pipe figure): a plausible rate, below the nominal
  2516.6 TFLOP/s, for both kinds of operands (which of the two is faster depends on how warm
  the chip is when the test runs)."""
  h = dev.default_handle()
  for split_shaped in (False, True):
    assert 300.0 < h.probe_bf16_mfma(split_shaped) < 2600.0


_TWO_RANK_GPU_WORKER = r'''
import os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
from telluride_decoding_amd import brain_data, device, distributed, regression
from tests.test_cpu_host import _loso_case

rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
torch.cuda.set_device(0)                      # both ranks on the one GPU of the box: gloo, not RCCL
dist.init_process_group('gloo')
files = _loso_case()
lens = [f[0].shape[0] for f in files]
pre, post, batch = 1, 2, 100
h = device.default_handle()

def stats_of(idx):
  st = device.LagStats(4, pre, post, d=2)
  offs = np.concatenate(([0], np.cumsum([lens[i] for i in idx])))
  st.accumulate(h.to_device(np.concatenate([files[i][0] for i in idx])), None,
                h.to_device(np.concatenate([files[i][2] for i in idx])), offs)
  return st

whole = stats_of(range(len(files)))
want = {k: v.cpu().numpy() for k, v in whole.moments().items() if v is not None}
# (a) recordings dealt to ranks: the real device statistics through pack -> all-reduce -> unpack
plan = distributed.ShardPlan(lens, world)
mine = stats_of(plan.files_of(rank))
distributed.allreduce_stats(mine, plan, rank, total_frames=sum(lens))
assert mine.counts() == whole.counts()
got = mine.moments()
for k, v in want.items():
  np.testing.assert_allclose(got[k].cpu().numpy(), v, rtol=1e-12, atol=1e-9)
# (b) the leave-one-out x lambda sweep on two ranks equals the one-rank sweep (the sweep's
#     solver included: each rank's folds against the total of ALL recordings)
ds = brain_data.Dataset(files, batch, pre, post, input_offset=2)
lams = [1e-3, 0.1, 10.0]
two = regression.jackknife_over_regularizations(ds, lams, rank=rank, world_size=world)
assert regression.LAST_SWEEP['solver'] in ('pcg', 'direct')
solo = [dist.new_group([r]) for r in range(world)][rank]
one = regression.jackknife_over_regularizations(ds, lams, rank=0, world_size=1, group=solo)
np.testing.assert_allclose(two['all_runs'], one['all_runs'], rtol=0, atol=2e-6)
dist.barrier()
dist.destroy_process_group()
print('rank %%d ok (%%s)' %% (rank, regression.LAST_SWEEP['solver']))
'''


def test_two_ranks_on_one_gpu_allreduce_and_loso_sweep(dev, tmp_path):
  """The multi-rank paths on the REAL device layer: two processes share the box's one GPU
  (gloo rendezvous on 127.0.0.1 -- RCCL needs a GPU per rank): allreduce_stats over file shards
  (pack / unpack kernels, slot layout) and jackknife_over_regularizations(world_size=2) -- table
  all-reduce, folds dealt round-robin, each rank's systems through the sweep solver, gather."""
  import os, subprocess, sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  script = tmp_path / 'worker_gpu.py'
  script.write_text(_TWO_RANK_GPU_WORKER % {'root': root})
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')}
  port = 30500 + (os.getpid() % 2000)
  procs = []
  for r in range(2):
    e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
             MASTER_PORT=str(port))
    procs.append(subprocess.Popen([sys.executable, str(script)], env=e, stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True))
  outs = []
  for p in procs:
    try:
      out, _ = p.communicate(timeout=240)
    except subprocess.TimeoutExpired:
      p.kill()
      out, _ = p.communicate()
    outs.append(out)
  for r, (p, out) in enumerate(zip(procs, outs)):
    assert p.returncode == 0, 'rank %d:\n%s' % (r, out[-3000:])
    assert 'rank %d ok' % r in out


@pytest.mark.parametrize('name', ['nolag', 'post3'])
def test_c1_exact_config_matches_reference_golden(dev, name):
  """BASELINE.json configs[0] at its stated size -- ONE 16-channel x 10 000-sample recording, batch
  100, lambda = 0.1 -- against the reference's own float32 output (golden G12) and the float64
  oracle: strict 1e-5 (the other C1 goldens are 2-3 files x 2 500)."""
  g = golden('g12_c1_10k')
  pre, post, batch = (int(v) for v in g[name + '_cfg'])
  h = dev.default_handle()
  eeg, env = g['eeg'], g['env']
  assert eeg.shape == (10000, 16)
  st = dev.LagStats(16, pre, post, d=1)
  st.accumulate(h.to_device(eeg), None, h.to_device(env[:, 0:1]), [0, 10000])
  w, b = st.ridge_solve([0.1])
  w, b = w.cpu().numpy()[0].astype(np.float64), b.cpu().numpy().astype(np.float64)
  w32, b32 = g[name + '_w'].astype(np.float64), g[name + '_b'].astype(np.float64)
  files = [(eeg.astype(np.float64), env[:, 1:2].astype(np.float64), env[:, 0:1].astype(np.float64),
            np.zeros((10000, 1)))]
  w64, b64, cx64, _, _ = o_reg.linear_regressor_from_batches(
      o_lag.minibatches(files, batch, pre=pre, post=post), lamb=0.1)
  scale = np.max(np.abs(w64))
  d_gpu_64 = max(np.max(np.abs(w - w64)), np.max(np.abs(b - b64))) / scale
  d_32_64 = max(np.max(np.abs(w32 - w64)), np.max(np.abs(b32 - b64))) / scale
  d_gpu_32 = max(np.max(np.abs(w - w32)), np.max(np.abs(b - b32))) / scale
  parity_log.record('ridge_golden_c1_10k_' + name, gpu_ref64=d_gpu_64, ref32_ref64=d_32_64,
                    gpu_ref32=d_gpu_32, strict=bool(d_gpu_32 < 1e-5))
  assert d_gpu_64 < 1e-5 and d_gpu_32 < 1e-5, (d_gpu_64, d_32_64, d_gpu_32)
  # the regularised covariance the function also returns (brain_model.py:478-481)
  m = st.moments()
  cov = m['xtx'].cpu().numpy() / 10000.0
  cov[np.diag_indices_from(cov)] += 0.1
  assert np.max(np.abs(cov - g[name + '_cov_x'])) <= 2e-6 * np.max(np.abs(cov))
  assert np.max(np.abs(cov - cx64)) <= 2e-7 * np.max(np.abs(cov))


@pytest.mark.parametrize('ratio_log2', [18, 24])
def test_within_channel_outlier_accumulate_and_weights(dev, ratio_log2):
  """ONE artefact sample 2^18 (and 2^24) times a unit-variance channel's level: the
  float16 two-piece form scales a channel by its LARGEST magnitude, so the ordinary samples of that
  channel sit 18 (24) binades below the top of the float16 range and their low piece goes
  subnormal (td_common.h: absolute error <= 2^-39 of the channel maximum per value).  All three
  accumulate modes against float64 moments -- every entry relative to sqrt(diag_i diag_j) -- and
  the ridge weights they lead to against the float64 oracle.  Measured (profiles/r04_parity.json): the
  float16 form holds 7.5e-8 on the moments and 9e-8 on the weights at BOTH ratios -- the bound of
  the header holds, no range guard to the bf16 three-piece kernel is needed."""
  rng = np.random.default_rng(18)
  h = dev.default_handle()
  n, c, post = 20000, 64, 31
  x = rng.standard_normal((n, c)).astype(np.float32)
  x[7777, 5] = np.float32(2.0 ** ratio_log2)
  y = (x[:, 3:4] * 0.7 + 0.2 * x[:, 40:41] + rng.standard_normal((n, 1))).astype(np.float32)
  xl = o_lag.lag_matrix(x.astype(np.float64), 0, post)
  xl1 = np.hstack((xl, np.ones((n, 1))))
  want, want_y = xl1.T @ xl1, xl1.T @ y.astype(np.float64)
  scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
  cov = want / n
  cov[np.diag_indices_from(cov)] += 0.1
  sol = np.linalg.solve(cov, want_y / n)
  w64 = sol[:-1]
  errs = {}
  try:
    for mode in ('f16x2', 'bf16x3', 'f32'):
      h.set_accumulate_mode(mode)
      st = dev.LagStats(c, 0, post, d=1)
      st.accumulate(h.to_device(x), None, h.to_device(y), [0, n])
      m = st.moments()
      e_m = float(np.max(np.abs(m['xtx'].cpu().numpy() - want) / scale))
      # ... and where it matters: the entries that do NOT involve the artefact channel must not feel it
      clean = np.ones(want.shape[0], bool)
      clean[5:c * (post + 1):c] = False
      got = m['xtx'].cpu().numpy()
      e_clean = float(np.max(np.abs(got[np.ix_(clean, clean)] - want[np.ix_(clean, clean)]) /
                             scale[np.ix_(clean, clean)]))
      w = st.ridge_solve([0.1])[0].cpu().numpy()[0].astype(np.float64)
      e_w = float(np.max(np.abs(w - w64)) / np.max(np.abs(w64)))
      errs[mode] = (e_m, e_clean, e_w)
      parity_log.record('outlier_2^%d_%s' % (ratio_log2, mode), moments=e_m, clean_moments=e_clean,
                        weights_vs_ref64=e_w)
  finally:
    h.set_accumulate_mode('f16x2')
  for mode, (e_m, e_clean, e_w) in errs.items():
    assert e_m < 2e-7 and e_clean < 2e-7, (mode, errs)
    assert e_w < 1e-5, (mode, errs)


@pytest.mark.parametrize('c,post,lens,off,drop', [
    (64, 31, (9000, 4000, 6001), 0, 0),       # the float16 matrix kernel: maxima travel in the statistics
    (64, 15, (5000, 5000), 0, 37),            # a dropped remainder
    (40, 7, (3000, 2500), 0, 0),              # float32 matrix kernel (<= 32... no: 40 channels, 8 lags)
    (16, 3, (2000, 1500), 2, 13),             # narrow: no maxima at all; input_offset
])
def test_targets_first_equals_the_fused_call(dev, c, post, lens, off, drop):
  """TD_ACC_TARGETS | TD_ACC_TARGETS_FIRST on ANOTHER handle and stream, then TD_ACC_MAIN (what
  pipeline.FitPipeline queues: targets(i + 1) beside the matrix kernel of fit i): the statistics --
  and the weights -- are bit-identical to the one fused call (same kernels, same maxima, same
  reduction order)."""
  import torch
  rng = np.random.default_rng(c + post)
  h = dev.default_handle()
  n = sum(lens)
  x = (rng.standard_normal((n, c)) * np.logspace(-1, 1, c)).astype(np.float32)
  y = (x[:, :1] * 0.3 + rng.standard_normal((n, 1))).astype(np.float32)
  offs = np.concatenate(([0], np.cumsum(lens)))
  zipped = [m - abs(off) for m in lens]
  used = list(zipped)
  used[-1] -= drop
  xd, yd = h.to_device(x), h.to_device(y)
  ref = dev.LagStats(c, 0, post, d=1, handle=h)
  ref.accumulate(xd, None, yd, offs, input_offset=off, rows_used=used)
  m_ref = ref.moments()
  w_ref = ref.ridge_solve([0.1])[0].cpu().numpy()
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    h2 = dev.Handle()
  st = dev.LagStats(c, 0, post, d=1, handle=h)
  for rep in range(2):                       # (twice: the statistics' own table is reused)
    st.reset()
    ev = torch.cuda.Event()
    with torch.cuda.stream(side):
      st.accumulate(xd, None, yd, offs, input_offset=off, rows_used=used, parts=2 | 4, handle=h2)
      ev.record(side)
    torch.cuda.current_stream().wait_event(ev)
    # (the second time with the MAIN call's finalize launch deferred: the pipeline's default)
    st.accumulate(xd, None, yd, offs, input_offset=off, rows_used=used, parts=1 | (8 if rep else 0))
    if rep:
      st.complete()
    m = st.moments()
    assert st.counts() == ref.counts()
    assert torch.equal(m['xtx'], m_ref['xtx']) and torch.equal(m['xty'], m_ref['xty'])
    assert np.array_equal(st.ridge_solve([0.1])[0].cpu().numpy(), w_ref)
  # the old order still works, and a TARGETS call without MAIN before it still says so
  st.reset()
  with pytest.raises(ValueError, match='TARGETS before MAIN'):
    st.accumulate(xd, None, yd, offs, input_offset=off, rows_used=used, parts=2)
  st.reset()
  st.accumulate(xd, None, yd, offs, input_offset=off, rows_used=used, parts=1)
  st.accumulate(xd, None, yd, offs, input_offset=off, rows_used=used, parts=2)
  assert torch.equal(st.moments()['xty'], m_ref['xty'])


def test_loso_folds_as_terms_of_the_total(dev):
  """td_ridge_solve_loso_terms (round 6): every fold given as the total's statistics plus signed terms (minus the
  held-out recording; minus / plus the last training recording and its truncated twin when batching drops a
  remainder) -- no fold statistics summed, the folds' dense moments from the total's in one launch.  Weights
  against the direct batched factorisation of the SUMMED fold statistics, recordings of uneven length with
  pre- and post-context and two outputs; then the whole sweep by both routes."""
  from telluride_decoding_amd import brain_data, regression
  rng = np.random.default_rng(3)
  lengths = (1230, 1111, 987, 1300, 1045, 700)
  files, stats = [], []
  h = dev.default_handle()
  c, pre, post, d = 40, 2, 5, 2
  for nf in lengths:
    x = rng.standard_normal((nf, c)).astype(np.float32)
    y = (x[:, :2] * 0.5 + rng.standard_normal((nf, 2))).astype(np.float32)
    files.append((x, y, y, np.zeros((nf, 1), np.float32)))
    st = dev.LagStats(c, pre, post, d=d, handle=h)
    st.accumulate(h.to_device(x), None, h.to_device(y), [0, nf])
    stats.append(st)
  # a truncated twin of the last recording (what a dropped remainder of 45 frames leaves of it)
  cut = dev.LagStats(c, pre, post, d=d, handle=h)
  cut.accumulate(h.to_device(files[-1][0]), None, h.to_device(files[-1][2]), [0, lengths[-1]],
                 rows_used=[lengths[-1] - 45])
  total = stats[0].like().combine(stats)
  lambdas = [1e-4, 0.1, 10.0]
  terms, sums = [], []
  for f in range(len(files) - 1):
    terms.append([(stats[f], -1.0), (stats[-1], -1.0), (cut, +1.0)])
    sums.append(stats[0].like().combine([stats[g] for g in range(len(files) - 1) if g != f] + [cut]))
  terms.append([(stats[-1], -1.0)])
  sums.append(stats[0].like().combine(stats[:-1]))
  out = dev.LagStats.ridge_solve_loso_terms(total, terms, lambdas, tol=1e-12, handle=h)
  assert out is not None, dev.LagStats.last_loso_status
  w, b, iters = out
  # ... and with a fold's models as the output columns of one filter (what td_predict_fir_per_file takes)
  w_km, b_km, _ = dev.LagStats.ridge_solve_loso_terms(total, terms, lambdas, tol=1e-12, handle=h, k_major=True)
  assert tuple(w_km.shape) == (len(terms), c * (pre + 1 + post), len(lambdas) * d)
  np.testing.assert_array_equal(w_km.cpu().numpy(),
                                w.permute(0, 2, 1, 3).reshape(len(terms), -1, len(lambdas) * d).cpu().numpy())
  np.testing.assert_array_equal(b_km.cpu().numpy(), b.cpu().numpy())
  w_ref, b_ref, flag = dev.LagStats.ridge_solve_multi(sums, lambdas, handle=h, wait=False)
  w, b, w_ref, b_ref = (t.cpu().numpy().astype(np.float64) for t in (w, b, w_ref, b_ref))
  assert flag() == 0 and 1 <= iters <= 40
  assert np.max(np.abs(w - w_ref)) <= 2e-6 * np.max(np.abs(w_ref))
  assert np.max(np.abs(b - b_ref)) <= 2e-6 * max(1.0, np.max(np.abs(b_ref)))
  # the sweep: both routes of the solver, and the direct solves
  ds = brain_data.Dataset(files, 100, pre_context=pre, post_context=post)
  runs = {}
  try:
    for name, use_terms, pcg in (('terms', True, True), ('sums', False, True), ('direct', True, False)):
      regression.USE_TERMS, regression.USE_PCG = use_terms, pcg
      runs[name] = regression.jackknife_over_regularizations(ds, lambdas)['all_runs']
      if pcg:
        assert regression.LAST_SWEEP['solver'] == 'pcg'
        assert regression.LAST_SWEEP['folds_as'] == ('terms of the total' if use_terms else 'sums')
  finally:
    regression.USE_TERMS, regression.USE_PCG = True, True
  np.testing.assert_allclose(runs['terms'], runs['sums'], rtol=0, atol=1e-7)
  np.testing.assert_allclose(runs['terms'], runs['direct'], rtol=0, atol=2e-6)
  # the statistics objects went back to the dataset's pool, and a sweep on reused objects is the same sweep
  pooled = len(ds.stats_pool(h, (c, pre, post, d)))
  assert pooled >= len(files) + 1
  again = regression.jackknife_over_regularizations(ds, lambdas)['all_runs']
  np.testing.assert_array_equal(again, runs['terms'])
  assert len(ds.stats_pool(h, (c, pre, post, d))) == pooled
  ds.release_device()
  assert len(ds.stats_pool(h, (c, pre, post, d))) == 0


@pytest.mark.parametrize('lens,c,pre,post,d,off', [
    ((5000, 7000, 3000), 64, 0, 31, 1, 0),
    ((900, 1500, 777, 130), 64, 0, 7, 1, -3),
    ((900, 1500, 777), 64, 2, 3, 2, 2),
    ((2500, 2600), 63, 0, 15, 1, 0),              # (virtual-image shapes -- rows that are not whole 16-byte granules,
    ((900, 1500, 777), 48, 1, 3, 1, 0),           #  <= 32 channels...: the call declines, nothing queued)
])
def test_accumulate_each_matches_per_file_calls(dev, lens, c, pre, post, d, off):
  """td_stats_accumulate_each (round 6): the per-recording statistics of a leave-one-out sweep from ONE targets
  launch and ONE matrix launch over all the recordings + a finalize launch each, against one td_stats_accumulate
  per recording -- frame counts exact, moments to 3e-7 (the float16 kernel's channel scales come from the maxima
  over all the recordings of the call), then each object keeps accumulating like any other."""
  rng = np.random.default_rng(11)
  h = dev.default_handle()
  n = sum(lens)
  x = h.to_device((rng.standard_normal((n, c)) * np.logspace(-1, 2, c)).astype(np.float32))
  y = h.to_device(rng.standard_normal((n, d)).astype(np.float32))
  offs = np.concatenate(([0], np.cumsum(lens)))
  used = [l - abs(off) - 7 for l in lens]
  one = []
  for f in range(len(lens)):
    st = dev.LagStats(c, pre, post, d=d)
    st.accumulate(x[offs[f]:offs[f + 1]], None, y[offs[f]:offs[f + 1]], [0, lens[f]], input_offset=off, rows_used=[used[f]])
    one.append(st)
  each = [dev.LagStats(c, pre, post, d=d) for _ in lens]
  handled = dev.LagStats.accumulate_each(each, x, y, offs, input_offset=off, rows_used=used)
  if c != 64:
    assert not handled and all(st.counts() == (0, 0) for st in each)
    return
  assert handled
  for a, b in zip(one, each):
    assert a.counts() == b.counts()
    ma, mb = a.moments(), b.moments()
    for k in ('xtx', 'xty'):
      pa, pb = ma[k].cpu().numpy(), mb[k].cpu().numpy()
      assert np.max(np.abs(pa - pb)) <= 3e-7 * np.max(np.abs(pa)), k
  # the objects are ordinary statistics afterwards: the sum of all of them solves like one call over the files
  whole = dev.LagStats(c, pre, post, d=d)
  whole.accumulate(x, None, y, offs, input_offset=off, rows_used=used)
  total = each[0].like().combine(each)
  w0, b0 = whole.ridge_solve([0.1])
  w1, b1 = total.ridge_solve([0.1])
  assert np.max(np.abs((w0 - w1).cpu().numpy())) <= 2e-6 * np.max(np.abs(w0.cpu().numpy()))
  # a second call on statistics that hold data is declined
  assert not dev.LagStats.accumulate_each(each, x, y, offs, input_offset=off, rows_used=used)


def test_c2_weights_at_full_size_match_the_oracle(dev):
  """BASELINE config C2 at FULL size -- 64 ch x 1e6 samples (10 recordings x 100 000 frames), 32 lags, minibatches
  of 1000, lambda = 0.1, bench.py's synthetic data -- through the model class, against golden G15: the oracle's
  float64 restatement of the reference's minibatch loop over the materialised lag matrix (brain_model.py:422-481),
  8.4 TFLOP of float64 products computed once in the build container (tests/golden/make_c2_full.py).
  |gpu - ref64| < 1e-5 of the largest weight, strict."""
  from telluride_decoding_amd import brain_data, brain_model, synth
  g = golden('g15_c2_full')
  trials = synth.make_trials(2, 10, 100000, 64)
  # the regenerated data are the fixture's (a seeded NumPy generator and NumPy's FFT)
  np.testing.assert_allclose(trials[0][0][:4, :4], g['eeg_head'], rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(trials[0][1][:4], g['env_head'], rtol=1e-6)
  assert abs(sum(float(t[0].astype(np.float64).sum()) for t in trials) - float(g['eeg_sum'])) < 1e-3 * (1 + abs(float(g['eeg_sum'])))
  files = [(eeg, env, env[:, 0:1].astype(np.float32), att) for eeg, env, att in trials]
  ds = brain_data.Dataset(files, 1000, pre_context=0, post_context=31)
  model = brain_model.BrainModelLinearRegression(ds, regularization_lambda=0.1)
  model.fit(ds)
  w64, b64 = g['w'], g['b'].reshape(-1)
  scale = float(np.max(np.abs(w64)))
  d_w = float(np.max(np.abs(model.w_estimate.astype(np.float64) - w64))) / scale
  d_b = float(np.max(np.abs(model.b_estimate.astype(np.float64) - b64))) / max(scale, float(np.max(np.abs(b64))))
  parity_log.record('ridge_c2_full_1e6', gpu_ref64=d_w, bias_gpu_ref64=d_b)
  assert d_w < 1e-5 and d_b < 1e-5, (d_w, d_b)
