"""Every branch of the solvers' host code (chol.hip, solve.hip, loso.hip and the handle options in api.hip), bit for bit
against the parent.

None of the factorisation, wide, multi, asynchronous, leave-one-out or td_chol_* routes has a floating-point atomic in
its kernels (the only atomic is the atomicExch of an int flag), so host code that moved without changing -- workspace
offsets, the padded batch of systems, the CholParams of every launch, the order of launches -- gives the parent's
bytes; a system padded at the wrong offset, a lambda table of another batch or a step of the preconditioner with the
wrong `m` does not.  One seeded case per branch at the smallest shapes at which these routes can go wrong: the tables
of tests/chol_edges.py (which say what each shape reaches), one case through each outside caller of td_chol_*, and
three hand-offs between conjugate gradients and the factorisation at shapes of tests/test_gpu_cg_solve.py.  Every case
runs twice on objects of its own (assert_array_equal) and the SHA-256 of its output must equal PARENT_SHA256: what the
library of the parent commit 2f07840 ("State the four online training banks' shared push path once") gave for these
seeds on the MI355X, run once through TD_HOTPATH_LIB.  Accuracy against float64 is the business of
test_gpu_chol_edges.py, test_gpu_cg_edges.py, test_gpu_cca_solve.py and test_gpu_cca_sweep_edges.py.

What a case hashes:
  ridge-*   every chol_edges.RIDGE_CASES entry on a handle set to 'cholesky': w, b, the asynchronous flag where there is
            one, and last_solve_info() after td_ridge_solve / _async (they reset the report).  td_ridge_solve_multi does
            not touch the report: the case asserts that it is what it was before the call.
  loso-*    every chol_edges.LOSO_CASES entry: w, b, status and iteration count; the terms cases also the k_major w, b.
            The report is untouched (asserted).
  spd-*     chol_edges.SPD_SIZE_LOOP through td_spd_solve: the solution.
  cca_chain td_cca_solve on the Cholesky-whitening route (td_chol_factor with K2 rows riding along, td_chol_back) at
            K1 = 12, K2 = 1 with cca_fused 0 (the one-launch dense stage would take K1 <= 64, K2 <= 16): the five outputs,
            the sweep counts and the route bits.
  cca_sweep cca_sweep_edges' k1_65 (two 64-blocks) through td_chol_batch_forward / _backward: the eight outputs.
  cg_dense  an automatic solve of one system of 129 unknowns that converges on the dense one-launch route: w, b, report.
  cg_gated  2049 unknowns, lambda = 1e-6: the conditioning gate (status 4) sends it on to the factorisation.
  cg_async_compact   an 'async_cg' solve on a handle masked to 64 CUs: the compact route, nothing waits; w, b, flag, report.
"""
import ctypes
import hashlib

import numpy as np
import pytest

from tests import cca_sweep_edges as se
from tests import cg_edges
from tests import chol_edges as xe

pytestmark = pytest.mark.gpu

# the parent commit's output: SHA-256 of the bytes of every array a case returns, in order
PARENT_SHA256 = {
    'ridge-c9-pre0-post6-d1-l1-solve1': 'f023545f25d01fc8c06490fd5c5352895a6745582715cbab1d9cfea78378fa68',
    'ridge-c8-pre0-post7-d8-l2-solve1': '0eb85d6d76fcb6229ae7b43da8ca76ed16e1a8f4d36bff842fcea569d97fabc6',
    'ridge-c15-pre0-post16-d1-l3-async1': '48f1003d9ac9c7a70ba3f6dd5ff8c1d1f79a463a7313e332cd2627a606bb86a9',
    'ridge-c16-pre1-post14-d8-l9-solve1': '13f7447a00c32543a225814c644055ae12771e4dd83949f1abfb99fae3763e8d',
    'ridge-c64-pre0-post7-d1-l2-solve1': '1319bcf0c710d4aa46ef4e3c8c3a038e584fd837500b9325b68adb10d5af5895',
    'ridge-c8-pre0-post7-d8-l3-multi3': '51c46f3558f4b9451544f5364ce5f3aa802291da369458ce8090742ec1401a33',
    'ridge-c16-pre0-post15-d1-l1-multi2': '40ab71a1fc646e3097d4cb2f41a069ccb209d2ab86c70c2a63598f0efb8805dc',
    'ridge-c9-pre0-post6-d9-l1-solve1': '0e0c8389ba6a8cc7a39ef5e6191c958d11598a611c21b14a4c7e58f9f293b5b5',
    'ridge-c8-pre0-post7-d63-l2-solve1': '0f3fd5ff2141e370867af5dfd8fc4b6f4bf64583e741199e1b4cf072efc0036f',
    'ridge-c15-pre0-post16-d64-l1-solve1': 'a8e199db37b4cbd492a78817d656f3111685bd7667908f70f3465d06c4dcb350',
    'ridge-c8-pre0-post7-d65-l1-async1': '87da6b222b7f22e1b864082d15261c24359e1f13204514185389a30e0ba20d2f',
    'ridge-c16-pre0-post15-d73-l1-multi2': 'b37d4a853f5e9e75fcd0184d30a36cfdc4a8bc0d5b5235600d8addf70c6ce13e',
    'ridge-c9-pre0-post6-d129-l1-solve1': 'e15eee244a6ecf4c149198be7c6ebe53a179c0c6c7c9e618bdeade1da1b42531',
    'loso-c9-pre0-post6-d1-f1-l1': 'f157cec8d17b88575332a648c8cf2c2b031e51df16f4c30538d43550f3443bee',
    'loso-c8-pre0-post7-d8-f4-l4': 'd12b4eae5a9827f7f1e33f4835b36892535564d89949af22c4799747e86ff63d',
    'loso-c16-pre0-post7-d7-f5-l5': '8a816d16c6546e541814e264c7b0b969b35dfabccd842c7b2c75981f281c1c9f',
    'loso-c16-pre0-post11-d8-f9-l9': '56a2f3dce8470f107da7c0e4ae120ac291c53707e0cc5e1e640373e36e973146',
    'loso-c16-pre0-post15-d1-f33-l2': 'dfb855bae5509264f5c72e7103d8d1e0f2bea9809a50abe47f06961aab276abb',
    'loso-c16-pre0-post15-d1-f31-l3': 'dbdffac5e19d629a4883f07ff5e7248cb31edb000c7d4e188264b35701e56996',
    'loso-c16-pre0-post23-d1-f3-l8': '3190c36d2a0b70c11d0d76e39f95390a2abba007faf594cc05dde5910e215e07',
    'loso-c16-pre0-post31-d2-f3-l1': '84cc1ef7f690ef44e067065ba5eb3ce9019bf0ce8b8c162ee1518831dfd85666',
    'loso-c16-pre1-post14-d7-f5-l5-terms': 'ae3400fa2c4ac7b932d5d2c6bbb7c3a46a6f840a580292384094a8910933205e',
    'loso-c8-pre0-post7-d1-f4-l9-terms': '479db3499336601d94738954e8e62ef87ea5eda2ec74b2d2a102412d1484e99d',
    'spd-n1-rhs1-b1': 'f6a13dd9d88e15af5857937bf8b5407481c686b18d1d072fb8ac7f4ca33c00eb',
    'spd-n63-rhs1-b2': 'a00bb9942c87b021e446817fec5e9ed34f70d89bfda9c81de342a7d00391904a',
    'spd-n64-rhs2-b1': '1ee770c19dc9c70aa1fd0a82d81f56bc45cc040de28c03a20a2900e613aea5ce',
    'spd-n65-rhs3-b2': '74c80de87b43e6d012645ee4dd76b8a838aa8ded99f2b5ca10e021dc40707601',
    'spd-n200-rhs1-b3': 'd61f2cccf5d3afbf7861cf0efc7fab1a94c72dac2f7a8792706f6f2b1463bf31',
    'spd-n513-rhs4-b1': '99218b92cb6be5535efd52c474c0327e825f34635cc9fc0b8cec9735ea4b37b0',
    'cca_chain': '70eeea349f77d8a6cd3bec4c287f2847ceed5818b51e71e73feb165db8fec624',
    'cca_sweep': 'b75065395c9acea1a96f9c723c7377cc7967f72c10fdbec4553d082f3e73e69a',
    'cg_dense': '4c203d78256918bf7b935e9fca56ebb066c84a7c0ff43a5ddf6c4fcc2fcc27ed',
    'cg_gated': '436e09f63c187909d4e47829a1df6ae443d2e230f83f46e75ddc978685ffb830',
    'cg_async_compact': 'de257932f72d47db55dc095b7883567b14612b16af628596403fdcc3ac23b95b',
}


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _info(h):
  i = h.last_solve_info()
  return np.array([{'none': 0, 'cholesky': 1, 'cg': 2}[i['solver']], i['iterations'], i['cg_status']], np.int32)


def _stats_of(dev, h, case, files):
  st = dev.LagStats(case.c, case.pre, case.post, d=case.d, handle=h)
  x = np.concatenate([f[0] for f in files])
  y = np.concatenate([f[1] for f in files])
  offs = np.concatenate(([0], np.cumsum([len(f[0]) for f in files])))
  st.accumulate(h.to_device(x), None, h.to_device(y), offs, handle=h)
  return st


def _ridge(dev, case):
  h = dev.default_handle()
  lams = xe.lambdas(case.n_lambda)
  sts = [_stats_of(dev, h, case, xe.ridge_files(case, s)) for s in range(case.stats)]
  h.set_solver('cholesky')
  try:
    if case.route == 'solve':
      w, b = sts[0].ridge_solve(lams, handle=h)
      return [w.cpu().numpy(), b.cpu().numpy(), _info(h)]
    if case.route == 'async':
      w, b, flag = sts[0].ridge_solve_async(lams, handle=h)
      h.synchronize()
      return [w.cpu().numpy(), b.cpu().numpy(), np.array([flag()], np.int32), _info(h)]
    before = _info(h)
    w, b = dev.LagStats.ridge_solve_multi(sts, lams, handle=h)
    np.testing.assert_array_equal(_info(h), before)
    return [w.cpu().numpy(), b.cpu().numpy()]
  finally:
    h.set_solver('auto')


def _loso(dev, case):
  h = dev.default_handle()
  lams = xe.lambdas(case.n_lambda)
  files = xe.loso_files(case)
  stats = {g: _stats_of(dev, h, case, [f]) for g, f in enumerate(files)}
  total = stats[0].like().combine([stats[g] for g in range(case.n_files)])
  before = _info(h)
  if case.as_terms:
    x, y = files[-1]
    cut = dev.LagStats(case.c, case.pre, case.post, d=case.d, handle=h)
    cut.accumulate(h.to_device(x), None, h.to_device(y), [0, len(x)], rows_used=[len(x) - xe.TRUNCATED], handle=h)
    stats['cut'] = cut
    terms = [[(stats[g], sg) for g, sg in fold] for fold in xe.terms_folds(case.n_files)]
    outs = []
    for k_major in (False, True):
      out = dev.LagStats.ridge_solve_loso_terms(total, terms, lams, tol=xe.CG_TOL, handle=h, k_major=k_major)
      assert out is not None, dev.LagStats.last_loso_status
      outs += [out[0].cpu().numpy(), out[1].cpu().numpy(), np.array([0, out[2]], np.int32)]
  else:
    sums = [stats[0].like().combine([stats[g] for g, _ in p]) for p in xe.loso_fold_parts(case)]
    out = dev.LagStats.ridge_solve_loso(total, sums, lams, tol=xe.CG_TOL, handle=h)
    assert out is not None, dev.LagStats.last_loso_status
    outs = [out[0].cpu().numpy(), out[1].cpu().numpy(), np.array([0, out[2]], np.int32)]     # (status, iterations)
  np.testing.assert_array_equal(_info(h), before)
  return outs


def _spd_call(h, a, rhs, n, nrhs, batch):
  return h.lib.td_spd_solve(h.ptr, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(rhs.data_ptr()), n, nrhs, batch)


def _spd(dev, size):
  import torch
  h = dev.default_handle()
  n, nrhs, batch = size
  a, rhs = xe.spd_system(xe.SpdCase(n, nrhs, batch, None, 'the size loop'))
  ad, rd = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(rhs)).cuda()
  h.check(_spd_call(h, ad, rd, n, nrhs, batch))
  return [rd.cpu().numpy()]


def _cca_chain(dev, _):
  h = dev.default_handle()
  rng = np.random.default_rng(1000 + 12 * 17 + 1)
  n, c1, c2 = 9000, 12, 1
  src = rng.standard_normal((n, 3)).astype(np.float32)
  x = (src @ rng.standard_normal((3, c1)) + rng.standard_normal((n, c1)) + 2.0).astype(np.float32)
  x2 = (src @ rng.standard_normal((3, c2)) + 0.5 * rng.standard_normal((n, c2)) - 1.0).astype(np.float32)
  st = dev.LagStats(c1, 0, 0, c2, 0, 0, handle=h)
  st.accumulate(h.to_device(x), h.to_device(x2), None, [0, n])
  h.set_option('cca_fused', 0)
  try:
    out = st.cca_solve(n - 1, 0.1, 1, handle=h)
  finally:
    h.set_option('cca_fused', 1)
  assert st.last_cca_route == 'cholesky' and not st.last_cca_fused
  return [t.cpu().numpy() for t in out[:5]] + [np.array(out[5], np.int32)]


def _cca_sweep(dev, _):
  h = dev.default_handle()
  case = next(c for c in se.CASES if c.name == 'k1_65')
  pre1, post1, pre2, post2 = se.lags(case)
  stats = []
  for x, x2 in se.make_parts(case):
    st = dev.LagStats(case.c1, pre1, post1, case.c2, pre2, post2, 0, handle=h)
    st.accumulate(h.to_device(x), h.to_device(x2), None, [0, len(x)])
    stats.append(st)
  total = stats[0].like().combine(stats[:case.n_total])
  terms = [[(stats[p], sg) for p, sg in fold] for fold in case.folds]
  out = dev.LagStats.cca_solve_loso_terms(total, terms, se.fold_batches(case), case.batch_size, list(case.lambdas),
                                          case.dim, handle=h)
  return [np.asarray(t.cpu()) for t in out]


def _cg_stats(dev, h, c, post, frames, files, seed=3):
  from telluride_decoding_amd import synth
  trials = synth.make_trials(seed, files, frames, c)
  eeg = np.concatenate([t[0] for t in trials])
  env = np.concatenate([t[1][:, :1] for t in trials])
  st = dev.LagStats(c, 0, post, d=1, handle=h)
  st.accumulate(h.to_device(eeg), None, h.to_device(env), np.arange(files + 1, dtype=np.int64) * frames, handle=h)
  return st


def _cg_dense(dev, _):
  h = dev.default_handle()
  w, b = _cg_stats(dev, h, 16, 7, 3000, 2).ridge_solve([0.1])
  info = _info(h)
  assert info[0] == 2 and info[2] == 0 and 0 < info[1] <= 160, info
  assert h.last_cg_plan()['kernel'] == 'resident'
  return [w.cpu().numpy(), b.cpu().numpy(), info]


def _cg_gated(dev, _):
  h = dev.default_handle()
  w, b = _cg_stats(dev, h, 64, 31, 6000, 3).ridge_solve([1e-6])
  info = _info(h)
  assert info.tolist() == [1, 0, 4], info
  return [w.cpu().numpy(), b.cpu().numpy(), info]


def _cg_async_compact(dev, _):
  import torch
  h, stream, (lib, p) = cg_edges.masked_handle(dev)
  with torch.cuda.stream(stream):
    st = _cg_stats(dev, h, 32, 7, 3000, 4, seed=3 + 32)
    h.set_option('async_cg', 1)
    w, b, flag = st.ridge_solve_async([0.1], handle=h)
    h.synchronize()
    out = [w.cpu().numpy(), b.cpu().numpy(), np.array([flag()], np.int32), _info(h)]
    assert h.last_cg_plan()['kernel'] == 'compact' and out[2][0] == 0 and out[3][0] == 2, (h.last_cg_plan(), out[2:])
  del st, h
  torch.cuda.synchronize()
  lib.td_stream_destroy(p)
  return out


CASES = {}
CASES.update({'ridge-' + xe.ridge_id(c): (_ridge, c) for c in xe.RIDGE_CASES})
CASES.update({'loso-' + xe.loso_id(c): (_loso, c) for c in xe.LOSO_CASES})
CASES.update({'spd-n%d-rhs%d-b%d' % s: (_spd, s) for s in xe.SPD_SIZE_LOOP})
CASES.update(cca_chain=(_cca_chain, None), cca_sweep=(_cca_sweep, None), cg_dense=(_cg_dense, None),
             cg_gated=(_cg_gated, None), cg_async_compact=(_cg_async_compact, None))


@pytest.mark.parametrize('name', list(CASES))
def test_route_gives_the_parents_bytes(dev, name):
  run, case = CASES[name]
  first, second = run(dev, case), run(dev, case)
  assert len(first) == len(second)
  shas = []
  for outs in (first, second):
    sha = hashlib.sha256()
    for u in outs:
      sha.update(np.ascontiguousarray(u).tobytes())
    shas.append(sha.hexdigest())
  print('ROUTE %s %s %s' % (name, shas[0], shas[1]))
  for u, v in zip(first, second):
    np.testing.assert_array_equal(u, v)
  assert shas[0] == PARENT_SHA256[name]


# the refusals that moved or pass through a shared helper: (what is wrong, the exception, the message); two bad
# arguments at once: the one the parent checks first is reported
INVALID, STATE = ValueError, 'HotPathError'
MESSAGES = [
    ('spd_nrhs_9', INVALID, 'td_spd_solve: nrhs must be in [1, 8], not 9'),
    ('spd_empty', INVALID, 'td_spd_solve: empty problem'),
    ('spd_empty+spd_nrhs_9', INVALID, 'td_spd_solve: empty problem'),
    ('ridge_no_lambda', INVALID, 'td_ridge_solve: need at least one lambda'),
    ('ridge_d0', INVALID, 'td_ridge_solve: statistics were created without a target (d = 0)'),
    ('ridge_no_lambda+ridge_d0', INVALID, 'td_ridge_solve: need at least one lambda'),
    ('ridge_no_data', STATE, 'td_ridge_solve: no data accumulated'),
    ('async_no_data', STATE, 'td_ridge_solve: no data accumulated'),
    ('multi_layouts', INVALID, 'td_ridge_solve_multi: layouts differ'),
    ('multi_one_empty', STATE, 'td_ridge_solve_multi: no data accumulated'),
    ('multi_layouts_then_empty', INVALID, 'td_ridge_solve_multi: layouts differ'),
    ('multi_empty_then_layouts', STATE, 'td_ridge_solve_multi: no data accumulated'),
    ('loso_d9', INVALID, 'td_ridge_solve_loso: outputs per solve must be in [1, 8]'),
    ('loso_max_iter_0', INVALID, 'td_ridge_solve_loso: bad sizes'),
    ('loso_max_iter_0+loso_d9', INVALID, 'td_ridge_solve_loso: bad sizes'),
    ('loso_layouts', INVALID, 'td_ridge_solve_loso: layouts differ'),
    ('loso_empty_fold', STATE, 'td_ridge_solve_loso: a fold has no data'),
    ('loso_empty_fold_then_layouts', STATE, 'td_ridge_solve_loso: a fold has no data'),
    ('terms_sign_half', INVALID, 'td_ridge_solve_loso_terms: a sign is +1 or -1'),
    ('terms_decreasing', INVALID, 'td_ridge_solve_loso_terms: term_begin must not decrease'),
    ('terms_layouts', INVALID, 'td_ridge_solve_loso_terms: layouts differ'),
    ('terms_layouts+terms_sign_half', INVALID, 'td_ridge_solve_loso_terms: layouts differ'),
    ('option_unknown', INVALID, "td_set_option: unknown option 'no_such_option'"),
    ('option_narrow16_2', INVALID, 'td_set_option: narrow16 is 0 or 1'),
    ('solver_mode_7', INVALID, 'td_set_solver: unknown mode 7'),
]


def test_refusals_word_for_word(dev):
  """The messages of MESSAGES and which of two bad arguments is reported.  None of these calls queues device work."""
  import torch
  from telluride_decoding_amd import _lib
  h = dev.default_handle()
  rng = np.random.default_rng(7)

  def stats(c, d, rows, post=1):
    st = dev.LagStats(c, 0, post, d=d, handle=h)
    if rows:
      x = rng.standard_normal((rows, c)).astype(np.float32)
      y = rng.standard_normal((rows, max(d, 1))).astype(np.float32)[:, :d]
      st.accumulate(h.to_device(x), None, h.to_device(y) if d else None, [0, rows], handle=h)
    return st

  full, full2, empty, other, wide = stats(4, 1, 50), stats(4, 1, 60), stats(4, 1, 0), stats(4, 1, 50, post=2), stats(4, 9, 50)
  no_target = dev.LagStats(4, 0, 1, 2, 0, 0, handle=h)                 # CCA statistics: d = 0
  out = h.empty((4096,), 'float32')
  buf = torch.zeros(64, dtype=torch.float64, device=out.device)
  optr = ctypes.c_void_p(out.data_ptr())
  lam, lam_p = _lib.f64_array([0.1])
  ptrs = lambda sts: (ctypes.c_void_p * len(sts))(*[s.ptr for s in sts])
  status, iters = ctypes.c_int(0), ctypes.c_int(0)
  flag = ctypes.POINTER(ctypes.c_int)()

  def loso(total, folds, max_iter=40):
    return h.lib.td_ridge_solve_loso(h.ptr, total.ptr, ptrs(folds), len(folds), lam_p, 1, max_iter, 1e-12, optr, optr,
                                     ctypes.byref(status), ctypes.byref(iters))

  def terms(sts, begin, signs):
    begin, signs = np.asarray(begin, np.int32), np.asarray(signs, np.float64)
    return h.lib.td_ridge_solve_loso_terms(
        h.ptr, full.ptr, ptrs(sts), begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        signs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(begin) - 1, lam_p, 1, 40, 1e-12, 0, optr, optr,
        ctypes.byref(status), ctypes.byref(iters))

  calls = {
      'spd_nrhs_9': lambda: _spd_call(h, buf, buf, 2, 9, 1),
      'spd_empty': lambda: _spd_call(h, buf, buf, 0, 1, 1),
      'spd_empty+spd_nrhs_9': lambda: _spd_call(h, buf, buf, 2, 9, 0),
      'ridge_no_lambda': lambda: h.lib.td_ridge_solve(h.ptr, full.ptr, lam_p, 0, optr, optr),
      'ridge_d0': lambda: h.lib.td_ridge_solve(h.ptr, no_target.ptr, lam_p, 1, optr, optr),
      'ridge_no_lambda+ridge_d0': lambda: h.lib.td_ridge_solve(h.ptr, no_target.ptr, lam_p, 0, optr, optr),
      'ridge_no_data': lambda: h.lib.td_ridge_solve(h.ptr, empty.ptr, lam_p, 1, optr, optr),
      'async_no_data': lambda: h.lib.td_ridge_solve_async(h.ptr, empty.ptr, lam_p, 1, optr, optr, ctypes.byref(flag)),
      'multi_layouts': lambda: h.lib.td_ridge_solve_multi(h.ptr, ptrs([full, other]), 2, lam_p, 1, optr, optr, None),
      'multi_one_empty': lambda: h.lib.td_ridge_solve_multi(h.ptr, ptrs([full, empty]), 2, lam_p, 1, optr, optr, None),
      'multi_layouts_then_empty': lambda: h.lib.td_ridge_solve_multi(h.ptr, ptrs([full, other, empty]), 3, lam_p, 1,
                                                                     optr, optr, None),
      'multi_empty_then_layouts': lambda: h.lib.td_ridge_solve_multi(h.ptr, ptrs([full, empty, other]), 3, lam_p, 1,
                                                                     optr, optr, None),
      'loso_d9': lambda: loso(wide, [wide]),
      'loso_max_iter_0': lambda: loso(full, [full2], max_iter=0),
      'loso_max_iter_0+loso_d9': lambda: loso(wide, [wide], max_iter=0),
      'loso_layouts': lambda: loso(full, [full2, other]),
      'loso_empty_fold': lambda: loso(full, [full2, empty]),
      'loso_empty_fold_then_layouts': lambda: loso(full, [empty, other]),
      'terms_sign_half': lambda: terms([full2], [0, 1], [0.5]),
      'terms_decreasing': lambda: terms([full2, full2], [0, 2, 1], [1.0, -1.0]),
      'terms_layouts': lambda: terms([other], [0, 1], [1.0]),
      'terms_layouts+terms_sign_half': lambda: terms([other], [0, 1], [0.5]),
      'option_unknown': lambda: h.lib.td_set_option(h.ptr, b'no_such_option', 1),
      'option_narrow16_2': lambda: h.lib.td_set_option(h.ptr, b'narrow16', 2),
      'solver_mode_7': lambda: h.lib.td_set_solver(h.ptr, 7),
  }
  assert list(calls) == [m[0] for m in MESSAGES]
  for wrong, exc, message in MESSAGES:
    with pytest.raises(_lib.HotPathError if exc == STATE else exc) as err:
      h.check(calls[wrong]())
    assert str(err.value) == message, wrong
  # nothing changed: the handle's options are what they were and it solves
  w, _ = full.ridge_solve([0.1], handle=h)
  assert np.all(np.isfinite(w.cpu().numpy()))
