"""The pipelined runs of whole k-steps in the plain float16 lag kernel (lagcov.hip: bf_krun_skip).

A tile's whole k-steps run as three blocks (k-steps 0-1, 2-5, 6-7) in which the LDS reads of k-step s + 1 are
issued inside the MFMAs of k-step s and the two B register blocks swap roles from one k-step to the next.  The
shapes are the smallest at which that can go wrong: one, two and three whole tiles with no cut tile (every run
head, every role swap, every run exit, with and without a next tile to stage), a cut tile of one row right
after a pipelined tile, a B span that reaches the zeros past a recording's end, the 99-dword geometry, channels
absent from the tile, and one workgroup that walks several slabs.

Every case runs on two handles.  The default handle's plan cuts even these recordings into slabs of ONE tile
(one work item per CU as long as there are tiles), so a handle that declares 4 CUs (td_set_cu_count) runs them
too: its plan keeps a recording in one slab, the tiles follow one another in one workgroup, and where there
are several slabs (two recordings; 8400 rows) ONE workgroup walks them all.

As in test_gpu_lag_kstep.py: LagStats.accumulate on seeded random data, every lag block against the float64
products of the materialised lag matrix, tolerance 2e-6 of the largest moment, xtx symmetric.

Bit-identity.  Only the place of the LDS reads in the instruction stream moved: operand words and the order of
a lag's products are those of the parent, so xtx is the parent's bit for bit.  PARENT_SHA256 holds the SHA-256
of the xtx bytes (float32, C order) that the library of the parent commit d7050a2 ("Move the stand-alone lag
kernel families out of lagcov.hip; add isa_diff") gave for these seeds, run once through TD_HOTPATH_LIB:
  64x32_384,     default handle  60f78cefaf7390ffdaee23c28bb77a0edc24cadc6290b4730134ca1e4c0eb749
  64x32_384,     4-CU handle     b9993049ce5afe63a90e026dcc67eb3a03e86e35a3764d150178d2c86f174f7b
  64x32_128_512, default handle  021b2aeec2b76bc6dbadc2eb1e077e681f82b80a9a772a6488402e778f4b7c3e
  64x32_128_512, 4-CU handle     5e2f9c780e0f86b12cd15e020a1b5a6f89c4328bfcfe93492d66092c194712ea
"""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import lag as o_lag

pytestmark = pytest.mark.gpu

TOL = 2e-6          # max |error| / max |reference|: test_gpu_fit.test_moments_match_dense_lag_matrix

SMALL_CUS = 4       # one work item per round of 32 lags: a recording <= 8192 rows stays one slab

CASES = {
    # one, two and three whole tiles, no cut tile
    '64x32_128': (64, 31, (128,)),
    '64x32_256': (64, 31, (256,)),
    '64x32_384': (64, 31, (384,)),
    # three whole tiles, then a cut tile of ONE row: the masked step right after a pipelined tile
    '64x32_385': (64, 31, (385,)),
    # a tile whose B span reaches the zeros past a recording's end, followed by another recording
    '64x32_128_512': (64, 31, (128, 512)),
    # the 99-dword geometry, five lag groups
    '64x40_512': (64, 39, (512,)),
    # channels absent from the tile (and rows that are not 16-byte aligned)
    '34x32_384': (34, 31, (384,)),
}

# the parent commit's xtx for these seeds: {case: {CUs the handle declares (0: the device's): SHA-256}}
PARENT_SHA256 = {
    '64x32_384': {0: '60f78cefaf7390ffdaee23c28bb77a0edc24cadc6290b4730134ca1e4c0eb749',
                  SMALL_CUS: 'b9993049ce5afe63a90e026dcc67eb3a03e86e35a3764d150178d2c86f174f7b'},
    '64x32_128_512': {0: '021b2aeec2b76bc6dbadc2eb1e077e681f82b80a9a772a6488402e778f4b7c3e',
                      SMALL_CUS: '5e2f9c780e0f86b12cd15e020a1b5a6f89c4328bfcfe93492d66092c194712ea'},
}


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


@pytest.fixture(scope='module')
def small_handle(dev):
  """A handle of the test's own that declares SMALL_CUS CUs: the slab plan and the grid follow that count."""
  h = dev.Handle()
  h.check(h.lib.td_set_cu_count(h.ptr, ctypes.c_int(SMALL_CUS)))
  return h


def _files(c, lens, seed):
  rng = np.random.default_rng(seed)
  return [(rng.standard_normal((n, c)).astype(np.float32),
           rng.standard_normal((n, 1)).astype(np.float32)) for n in lens]


def _lagged(files, post):
  """float64, the lag matrix materialised: [x~ | 1] and y."""
  xs, ys = [], []
  for x, y in files:
    z = np.zeros((x.shape[0], 1))
    xl, _, yl, _ = o_lag.window_streams(x.astype(np.float64), z, y.astype(np.float64),
                                        z.astype(np.float32), pre=0, post=post, pre2=0, post2=0,
                                        input_offset=0)
    xs.append(xl); ys.append(yl)
  X = np.concatenate(xs); Y = np.concatenate(ys)
  return np.hstack((X, np.ones((X.shape[0], 1)))), Y


def _accumulate(dev, h, files, c, post):
  st = dev.LagStats(c, 0, post, d=1, handle=h)
  offs = np.concatenate(([0], np.cumsum([f[0].shape[0] for f in files])))
  xd = h.to_device(np.concatenate([f[0] for f in files]))
  yd = h.to_device(np.concatenate([f[1] for f in files]))
  st.accumulate(xd, None, yd, offs)
  m = st.moments()
  return m['xtx'].cpu().numpy(), m['xty'].cpu().numpy()


_REF = {}


def _reference(name):
  """(files, xtx, xty) of a case in float64: computed once, shared by the two handles' runs."""
  if name not in _REF:
    c, post, lens = CASES[name]
    files = _files(c, lens, 1977 + c + post + sum(lens))
    X1, Y = _lagged(files, post)
    _REF[name] = (files, X1.T @ X1, X1.T @ Y)
  return _REF[name]


def run_case(dev, h, name):
  """xtx, xty of a case on the handle h."""
  c, post, _ = CASES[name]
  return _accumulate(dev, h, _reference(name)[0], c, post)


@pytest.mark.parametrize('cus', [0, SMALL_CUS], ids=['default', 'cu4'])
@pytest.mark.parametrize('name', list(CASES))
def test_every_lag_block_matches_the_float64_products(dev, small_handle, name, cus):
  c, post, _ = CASES[name]
  _, ref_xtx, ref_xty = _reference(name)
  xtx, xty = run_case(dev, small_handle if cus else dev.default_handle(), name)
  scale = np.max(np.abs(ref_xtx))
  worst = 0.0
  for e in range(post + 1):
    # lag e: the channel block (lag column 0, lag column e)
    blk = np.s_[0:c, e * c:(e + 1) * c]
    err = np.max(np.abs(xtx[blk] - ref_xtx[blk])) / scale
    worst = max(worst, err)
    assert err < TOL, 'lag %d: %.3g' % (e, err)
  print('%s, %s handle: worst lag block %.3g of the largest moment' % (name, 'a 4-CU' if cus else 'the default', worst))
  assert np.max(np.abs(xtx - ref_xtx)) / scale < TOL
  assert np.max(np.abs(xty - ref_xty)) / np.max(np.abs(ref_xty)) < TOL
  np.testing.assert_array_equal(xtx, xtx.T)
  if name in PARENT_SHA256:
    sha = hashlib.sha256(np.ascontiguousarray(xtx, dtype=np.float32).tobytes()).hexdigest()
    print('%s, %d CUs: sha256(xtx) %s' % (name, cus, sha))
    assert sha == PARENT_SHA256[name][cus]


def test_one_workgroup_walks_two_slabs(dev, small_handle):
  """8400 rows are two slabs (a slab is at most 8192 rows: 32 whole tiles and a cut tile of 104 rows each) and
  the 4-CU handle's grid is one workgroup per lag group, which walks both: the __syncthreads and the reload
  between two work items with a pipelined run on both sides.  The reference is the block row of the lag-0
  channels -- x^T x~, every lag block the kernel sums, 2 GFLOP in float64 where the whole 2049 x 2049 matrix
  is 70 -- and the column of ones; the rest of xtx is put together from those by the finalize launch, which
  the cases above check in full."""
  c, post, n = 64, 31, 8400
  files = _files(c, (n,), 1977 + n)
  X1, Y = _lagged(files, post)
  ref_rows = X1[:, :c].T @ X1                    # [c, c (post + 1) + 1]
  ref_ones = X1[:, -1] @ X1
  xtx, xty = _accumulate(dev, small_handle, files, c, post)
  # the largest moment of the whole xtx lies on its diagonal (a Gram matrix): the columns' sums of squares
  scale = float(np.max(np.sum(X1 * X1, axis=0)))
  for e in range(post + 1):
    blk = np.s_[0:c, e * c:(e + 1) * c]
    err = np.max(np.abs(xtx[blk] - ref_rows[blk])) / scale
    assert err < TOL, 'lag %d: %.3g' % (e, err)
  assert np.max(np.abs(xtx[:c] - ref_rows)) / scale < TOL
  assert np.max(np.abs(xtx[-1] - ref_ones)) / scale < TOL
  assert np.max(np.abs(xty - X1.T @ Y)) / np.max(np.abs(X1.T @ Y)) < TOL
  np.testing.assert_array_equal(xtx, xtx.T)
