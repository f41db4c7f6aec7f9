"""The float16 lag kernel's k-step with the lags +0, +1, +4, +5 per wave (lagcov.hip: bf_kstep_skip).

Every case runs LagStats.accumulate on random data and compares, for every lag e, the block
sum_t x[t] x[t + e]^T of the moments with the float64 sum of the materialised products.  Random
data gives every lag a block of its own, so a lag that lands in another lag's place of the slab
fails; the tolerance is the one test_moments_match_dense_lag_matrix holds the float16 mode to.
"""
import numpy as np
import pytest

from oracle import lag as o_lag

pytestmark = pytest.mark.gpu

TOL = 2e-6          # max |error| / max |reference|: test_gpu_fit.test_moments_match_dense_lag_matrix


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _files(c, lens, seed):
  rng = np.random.default_rng(seed)
  return [(rng.standard_normal((n, c)).astype(np.float32),
           rng.standard_normal((n, 1)).astype(np.float32)) for n in lens]


def _dense(files, post):
  """float64, the lag matrix materialised: [x~ | 1]^T [x~ | 1] and [x~ | 1]^T y."""
  xs, ys = [], []
  for x, y in files:
    z = np.zeros((x.shape[0], 1))
    xl, _, yl, _ = o_lag.window_streams(x.astype(np.float64), z, y.astype(np.float64),
                                        z.astype(np.float32), pre=0, post=post, pre2=0, post2=0,
                                        input_offset=0)
    xs.append(xl); ys.append(yl)
  X = np.concatenate(xs); Y = np.concatenate(ys)
  X1 = np.hstack((X, np.ones((X.shape[0], 1))))
  return X1.T @ X1, X1.T @ Y


def _accumulate(dev, files, c, post, parts=(3,)):
  h = dev.default_handle()
  st = dev.LagStats(c, 0, post, d=1)
  offs = np.concatenate(([0], np.cumsum([f[0].shape[0] for f in files])))
  xd = h.to_device(np.concatenate([f[0] for f in files]))
  yd = h.to_device(np.concatenate([f[1] for f in files]))
  for p in parts:
    st.accumulate(xd, None, yd, offs, parts=p)
  m = st.moments()
  return m['xtx'].cpu().numpy(), m['xty'].cpu().numpy()


CASES = {
    # two whole tiles and a cut tile of 44 rows: the masked k-step three times, the last one partial
    '64x32_300': (64, 31, (300,)),
    # a cut tile of ONE row; operand spans that reach the zeros past a recording's end
    '64x32_129_1000': (64, 31, (129, 1000)),
    # the last lag group only partly asked for: lags >= the lag count land nowhere
    '64x5': (64, 4, (300,)),
    '64x13': (64, 12, (129, 1000)),
    # the 99-dword geometry, five lag groups
    '64x40': (64, 39, (300, 700)),
    # channels absent from the tile
    '34x32': (34, 31, (300,)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_every_lag_block_matches_the_float64_products(dev, name):
  c, post, lens = CASES[name]
  files = _files(c, lens, 77 + c + post)
  ref_xtx, ref_xty = _dense(files, post)
  xtx, xty = _accumulate(dev, files, c, post)
  scale = np.max(np.abs(ref_xtx))
  worst = 0.0
  for e in range(post + 1):
    # lag e: the channel block (lag column 0, lag column e)
    blk = np.s_[0:c, e * c:(e + 1) * c]
    err = np.max(np.abs(xtx[blk] - ref_xtx[blk])) / scale
    worst = max(worst, err)
    assert err < TOL, 'lag %d: %.3g' % (e, err)
  print('%s: worst lag block %.3g of the largest moment' % (name, worst))
  assert np.max(np.abs(xtx - ref_xtx)) / scale < TOL
  assert np.max(np.abs(xty - ref_xty)) / np.max(np.abs(ref_xty)) < TOL
  np.testing.assert_array_equal(xtx, xtx.T)


def test_two_parts_equal_one_call_bitwise(dev):
  c, post, lens = CASES['64x32_300']
  files = _files(c, lens, 77 + c + post)
  one = _accumulate(dev, files, c, post, parts=(3,))
  two = _accumulate(dev, files, c, post, parts=(1, 2))
  np.testing.assert_array_equal(two[0], one[0])
  np.testing.assert_array_equal(two[1], one[1])
