"""The targets pass on the float16 matrix pipe (lagcov_targets_split_kernel): y^T x~ per lag, column
sums, sum of y, against float64 on the host -- the materialised lag matrix of oracle/lag.py -- and
against the float32 kernel it replaces (td_set_option "targets_f16" 0).

Distance of every entry: |d(y^T x~)[e][j]| / sqrt(sum y^2 . sum x~[e][j]^2), bound 2e-6 (the bound
test_moments_match_dense_lag_matrix puts on every moment).  Where the bound comes from: both
operands are two float16 pieces (22 bits, 2^-22 = 2.4e-7 per product, errors of random sign) under
exact power-of-two scales, chains of 32 rows in float32 (2^-24 per addition), float64 beyond; the
float32 kernel measures ~2e-7 on the same cases.  Every case records both kernels' distances
(tests/parity_log.py).

The column sums, the sum of y and the channel maxima are computed from the same float32 values in the
same order by both kernels: the sums are compared bit for bit here (last row of xtx and of xty).  The
channel-maximum table is not visible through the API; what is compared is its consumer -- xtx of
the float16 matrix kernel, which takes its scales from the table, bit for bit."""
import zlib

import numpy as np
import pytest

from oracle import lag as o_lag
from tests import parity_log

pytestmark = pytest.mark.gpu

BOUND = 2e-6


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _host(files, pre, post, off=0, used_last=None):
  """float64 on the materialised lag matrix: y^T x~, the norms of the distance, column sums, sum of y."""
  xs, ys = [], []
  for i, (x, y) in enumerate(files):
    z = np.zeros((x.shape[0], 1))
    xl, _, yl, _ = o_lag.window_streams(x.astype(np.float64), z, y.astype(np.float64), z, pre=pre, post=post,
                                        input_offset=off)
    if i == len(files) - 1 and used_last is not None:
      xl, yl = xl[:used_last], yl[:used_last]
    xs.append(xl); ys.append(yl)
  X, Y = np.concatenate(xs), np.concatenate(ys)
  with np.errstate(invalid='ignore', over='ignore'):
    return dict(xty=X.T @ Y, norm=np.sqrt(np.outer((X * X).sum(0), (Y * Y).sum(0))), n=X.shape[0])


def _gpu(dev, files, pre, post, off=0, rows_used=None, f16=1):
  h = dev.default_handle()
  c, d = files[0][0].shape[1], files[0][1].shape[1]
  lens = [f[0].shape[0] for f in files]
  offs = np.concatenate(([0], np.cumsum(lens)))
  x = np.concatenate([f[0] for f in files]) if sum(lens) else np.zeros((0, c), np.float32)
  y = np.concatenate([f[1] for f in files]) if sum(lens) else np.zeros((0, d), np.float32)
  h.set_option('targets_f16', f16)
  try:
    st = dev.LagStats(c, pre, post, d=d)
    st.accumulate(h.to_device(x), None, h.to_device(y), offs, input_offset=off, rows_used=rows_used)
    m = st.moments()
    xtx, xty = m['xtx'].cpu().numpy(), m['xty'].cpu().numpy()
  finally:
    h.set_option('targets_f16', 1)
  return dict(xty=xty[:-1], sum_y=xty[-1], colsum=xtx[-1, :-1], xtx=xtx, n=st.counts()[0])


def _dist(got, ref):
  err = np.abs(got - ref['xty'])
  zero = ref['norm'] == 0
  assert np.all(err[zero] == 0), 'a product of an all-zero column is not zero'
  return float(np.max(err[~zero] / ref['norm'][~zero])) if np.any(~zero) else 0.0


def _check(dev, name, files, pre, post, off=0, drop=0, expect_same=False):
  """Both kernels against float64; the sums that must not depend on the kernel bit for bit."""
  lens = [f[0].shape[0] for f in files]
  rows_used, used_last = None, None
  if drop:
    rows_used = [n - abs(off) for n in lens]
    used_last = rows_used[-1] = lens[-1] - abs(off) - drop
  ref = _host(files, pre, post, off, used_last)
  new = _gpu(dev, files, pre, post, off, rows_used, 1)
  again = _gpu(dev, files, pre, post, off, rows_used, 1)
  old = _gpu(dev, files, pre, post, off, rows_used, 0)
  assert new['n'] == ref['n'] == old['n']
  d_new, d_old = _dist(new['xty'], ref), _dist(old['xty'], ref)
  print('%s: f16 %.3g  f32 %.3g' % (name, d_new, d_old))
  parity_log.record('targets_split_' + name, f16=d_new, f32=d_old)
  assert d_new < BOUND, (name, d_new, d_old)
  np.testing.assert_array_equal(new['xty'], again['xty'])          # two runs bitwise equal
  np.testing.assert_array_equal(new['xtx'], again['xtx'])
  np.testing.assert_array_equal(new['colsum'], old['colsum'])      # same float32 partial sums, same order
  np.testing.assert_array_equal(new['sum_y'], old['sum_y'])
  np.testing.assert_array_equal(new['xtx'], old['xtx'])            # same channel maxima -> same scales
  if expect_same:                                                  # a shape the new kernel does not take
    np.testing.assert_array_equal(new['xty'], old['xty'])
  return new, old, ref


def _white(rng, lens, c, d=1):
  return [(rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32))
          for n in lens]


def test_c2_shape_white_and_correlated(dev):
  """64 channels x 32 lags, one target: white data, and y = a channel + noise (the sums drift)."""
  rng = np.random.default_rng(701)
  files = _white(rng, (20000, 20000), 64)
  _check(dev, 'c2_white', files, 0, 31)
  files = [(x, (0.8 * x[:, 9:10] + 0.3 * rng.standard_normal((x.shape[0], 1))).astype(np.float32)) for x, _ in files]
  _check(dev, 'c2_drift', files, 0, 31)


@pytest.mark.parametrize('c,same', [(33, True), (40, False), (63, True), (64, False), (96, False), (128, False)])
@pytest.mark.parametrize('lags', [1, 5, 31, 32])
def test_channels_and_lags(dev, c, lags, same):
  """Odd channel counts have no 8-byte row pairs and keep the float32 kernel (bitwise the same
  answer); 40, 64 take the new one, 96 and 128 as two tiles."""
  rng = np.random.default_rng(1000 + c * 40 + lags)
  _check(dev, 'c%d_l%d' % (c, lags), _white(rng, (3000, 700), c), 0, lags - 1, expect_same=same)


@pytest.mark.parametrize('name,c,pre,post,off,lens,drop', [
    ('pre_context', 64, 5, 20, 0, (3000, 640), 0),
    ('pre_context_all', 40, 31, 0, 0, (2500,), 0),
    ('offset_pos', 64, 0, 31, 2, (4097, 640), 5),
    ('offset_neg', 64, 3, 8, -3, (4097, 640), 0),
    ('dropped_remainder', 48, 0, 15, 1, (2100, 2049), 130),
    ('ten_recordings', 64, 0, 31, 0, (500, 2048, 2049, 2047, 100, 4096, 33, 700, 64, 1500), 0),
    ('tiny_recordings', 64, 0, 31, 0, (1, 31, 32, 33, 2049, 0, 2, 5000), 0),
    ('one_body', 64, 0, 31, 0, (1, 3000), 0),                 # a strip of exactly one 32-row body
    ('body_plus_row', 64, 0, 31, 0, (2, 3000), 0),            # ... and of a body plus one row
    ('two_targets', 64, 0, 31, 0, (3000, 100), 0),
])
def test_geometry(dev, name, c, pre, post, off, lens, drop):
  rng = np.random.default_rng(zlib.crc32(name.encode()) % 100000)
  _check(dev, name, _white(rng, lens, c, 2 if name == 'two_targets' else 1), pre, post, off, drop)


def _ramp(n):
  return np.exp2(np.linspace(-30.0, 30.0, n)).astype(np.float32)[:, None]


@pytest.mark.parametrize('name', ['zero_bodies', 'outlier_2^18', 'outlier_2^24', 'ramp', 'volts_vs_thousands',
                                  'denormal_channels', 'y_zero', 'x_zero'])
def test_forced_scale_branches(dev, name):
  """Scales that random data never takes: a body whose channel is all zero (scale 0), one sample far
  above its channel's level (the body's other values sit deep in the low piece), a level that moves
  60 binades along the recording (a scale per body follows it), operands 9 decades apart, denormal
  channels (the scale is applied by ldexp, beyond 2^126), all-zero operands."""
  rng = np.random.default_rng(zlib.crc32(name.encode()) % 100000)
  n, c = 6000, 64
  x = rng.standard_normal((n, c)).astype(np.float32)
  y = (0.5 * x[:, 3:4] + rng.standard_normal((n, 1))).astype(np.float32)
  if name == 'zero_bodies':
    x[1000:1200, 5] = 0
    x[:, 6] = 0
    x[64:96, 7] = 0
    y[3000:3100] = 0
  elif name.startswith('outlier'):
    x[4321, 5] = np.float32(2.0 ** int(name.split('^')[1]))
  elif name == 'ramp':
    x[:, 10:11] *= _ramp(n)
    x[:, 11:12] *= _ramp(n)[::-1]
    y = (y * _ramp(n)[::-1]).astype(np.float32)
  elif name == 'volts_vs_thousands':
    x = (x * np.float32(1e-6)).astype(np.float32)
    y = (y * np.float32(3000.0)).astype(np.float32)
  elif name == 'denormal_channels':
    x[:, 20] = (x[:, 20].astype(np.float64) * 1e-40).astype(np.float32)
    x[:, 21] = (x[:, 21].astype(np.float64) * 3e-39).astype(np.float32)
    x[:, 22] = np.where(np.arange(n) % 2 == 0, x[:, 22], np.float32(1e-42))
    assert np.all(np.abs(x[:, 20]) < np.finfo(np.float32).tiny)
  elif name == 'y_zero':
    y[:] = 0
  elif name == 'x_zero':
    x[:] = 0
  _check(dev, name, [(x, y)], 0, 31)


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('row', [2048, 2048 + 31, 2048 + 13, 0, 5999])
def test_non_finite_x(dev, value, row):
  """A NaN or an infinity in x at a body's first, last and an interior row (and at the recording's
  ends): non-finite in every lag of that channel, as float32 arithmetic leaves it, finite elsewhere."""
  rng = np.random.default_rng(77)
  n, c, lags = 6000, 64, 32
  x = rng.standard_normal((n, c)).astype(np.float32)
  y = rng.standard_normal((n, 1)).astype(np.float32)
  x[row, 17] = value
  x[(row + 1000) % n, 40] = value
  bad = np.zeros(c * lags, bool)
  for lag in range(lags):
    bad[lag * c + 17] = bad[lag * c + 40] = True
  for f16 in (0, 1):
    got = _gpu(dev, [(x, y)], 0, lags - 1, f16=f16)['xty'][:, 0]
    assert np.all(~np.isfinite(got[bad])), f16
    assert np.all(np.isfinite(got[~bad])), f16
  x[row, 17] = x[(row + 1000) % n, 40] = 0
  ref = _host([(x, y)], 0, lags - 1)
  err = np.abs(got[:, None] - ref['xty'])[~bad] / ref['norm'][~bad]          # (the float16 kernel's)
  assert float(np.max(err)) < BOUND


@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_non_finite_y(dev, value):
  """A non-finite target reaches every lag of every channel (A[m][v] = y[v - m] meets every row of x)."""
  rng = np.random.default_rng(78)
  n, c = 3000, 64
  x = rng.standard_normal((n, c)).astype(np.float32)
  y = rng.standard_normal((n, 1)).astype(np.float32)
  y[1500] = value
  for f16 in (1, 0):
    got = _gpu(dev, [(x, y)], 0, 31, f16=f16)['xty']
    assert np.all(~np.isfinite(got)), f16
