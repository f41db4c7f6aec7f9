"""CPU tests of the Jacobi / SVD / CCA dense-stage edge sweep (tests/eig_edges.py): the restated constants equal the
source's, the restated orderings meet every pair, the tables reach every branch the sweep names, the numpy models of the
kernels' algebra sit inside the bounds they help to set, the tables' data meet the bounds' conditions (gaps, eigenvalue
margins, the factor of 100 around the Gram cuts), the models say what a NaN channel gives, and seven wrong kernels,
modelled in numpy, land outside.  No GPU needed."""
import itertools

import numpy as np
import pytest

from tests import cca_sweep_edges as cs
from tests import eig_edges as ee

CCA = {c.name: c for c in ee.CCA_CASES}


def test_restated_constants_equal_the_source():
  found = ee.source_constants()
  assert set(found) == set(ee.CONSTANT_NAMES.values()) | set(ee.LITERALS) | {'CHOL2'}
  for mine, value in found.items():
    if mine != 'CHOL2':
      assert value == getattr(ee, mine), mine
  assert found['CHOL2'] == (ee.FUSED_K2, ee.CHOL_K2) and ee.FUSED_K1 == ee.NB
  assert np.finfo(np.longdouble).eps < 2.0 ** -60          # the relative-accuracy reference runs in np.longdouble


def test_round_robin_meets_every_pair_once_per_sweep():
  for n_players in range(2, 65, 2):
    met = []
    for rnd in range(n_players - 1):
      pairs = [ee.rr_pair(n_players, rnd, k) for k in range(n_players // 2)]
      assert all(p < q for p, q in pairs)
      assert sorted(i for pq in pairs for i in pq) == list(range(n_players))       # every player once per round
      met += pairs
    assert sorted(met) == list(itertools.combinations(range(n_players), 2))        # every pair once per sweep
  assert [ee.players(n) for n in (1, 2, 3, 63, 64)] == [2, 2, 4, 64, 64]


def test_block_rounds_meet_every_element_pair_every_outer_sweep():
  """Round 0 runs the full ordering inside every block pair, the later rounds the 32 x 32 cross pairs only: together
  every pair of the padded matrix's elements, at least once."""
  cross = {(int(p), int(q)) for ps, qs in ee.cross_rounds() for p, q in zip(ps, qs)}
  assert cross == {(p, q) for p in range(ee.HB) for q in range(ee.HB, ee.NB)}
  assert len({(int(p), int(q)) for ps, qs in ee.cross_rounds(fixed=True) for p, q in zip(ps, qs)}) == ee.HB
  for nblocks in range(4, 11, 2):
    pl = ee.block_plan(nblocks * ee.HB)
    assert (pl.np, pl.nblocks, pl.pairs) == (nblocks * ee.HB, nblocks, nblocks // 2)
    assert [(r, c) for r, _, c in pl.launches] == [(r, r > 0) for r in range(nblocks - 1)]
    met = set()
    for rnd, pairs, cross_only in pl.launches:
      for b in range(pairs):
        bp, bq = ee.rr_pair(nblocks, rnd, b)
        idx = list(range(bp * ee.HB, bp * ee.HB + ee.HB)) + list(range(bq * ee.HB, bq * ee.HB + ee.HB))
        local = cross if cross_only else set(itertools.combinations(range(ee.NB), 2))
        met |= {(idx[p], idx[q]) for p, q in local}
    assert met == set(itertools.combinations(range(pl.np), 2))
  assert ee.block_plan(65).np == 128 and ee.block_plan(193).nblocks == 8


def test_eig_table_reaches_every_branch():
  cases = ee.EIG_CASES
  assert len({ee.eig_id(c) for c in cases}) == len(cases)
  assert {c.n for c in cases} == {1, 2, 3, 16, 17, 32, 33, 63, 64, 65, 96, 127, 128, 129, 192, 193}
  reached = set()
  for c in cases:
    route = 'direct' if c.n <= ee.NB else 'block'
    reached.add((route, c.kind))
    if route == 'direct' and c.n & 1:
      reached.add(('phantom player', ee.players(c.n)))
    if route == 'block':
      reached.add(('blocks', ee.block_plan(c.n).nblocks, 'padding', ee.block_plan(c.n).np - c.n))
    if c.kind in ee.DIAGONAL_KINDS:
      model = ee.eig_reference(c)[2]
      assert model.rotations == 0 and model.sweeps == (0 if route == 'direct' else 1)
      reached.add((route, 'quick reject'))
  want = {(r, k) for r in ('direct', 'block') for k in ee.EIG_KINDS}
  want |= {('direct', 'quick reject'), ('block', 'quick reject'), ('phantom player', 2), ('phantom player', 4),
           ('phantom player', 64), ('blocks', 4, 'padding', 63), ('blocks', 4, 'padding', 0), ('blocks', 6, 'padding', 63),
           ('blocks', 8, 'padding', 63), ('blocks', 6, 'padding', 0)}
  assert want <= reached, want - reached


def test_svd_table_reaches_every_branch():
  cases = ee.SVD_CASES
  assert len({ee.svd_id(c) for c in cases}) == len(cases)
  assert ee.svd_small_doubles(8, 865) == 7000 and ee.svd_small_doubles(8, 866) == 7016
  assert ee.svd_small_doubles(1, 6997) <= ee.SMALL_SVD_DOUBLES < ee.svd_small_doubles(1, 7001)
  reached = set()
  for c in cases:
    if c.kind in ('graded', 'cut_below', 'cut_above') or c.k <= 16:
      route = ee.svd_reference(c)[3]
    else:
      route = ee.svd_route(c.k, c.m)             # ('gram': the Gram matrix is formed)
    reached.add((c.k, c.m, route))
    reached.add((c.kind, route))
    reached.add(('dim', c.dim if c.dim < c.k else 'k'))
    reached.add('tall' if c.tall else 'wide')
    if c.k & 1 and c.k > 1:
      reached.add(('bye', route))
  want = {(8, 865, 'small'), (8, 866, 'gram'), (8, 866, 'rounds'), (1, 6997, 'small'), (1, 7001, 'rounds'),
          (64, 255, 'rounds'), (64, 256, 'gram'), (64, 256, 'rounds'), (65, 300, 'rounds'), (2, 9, 'small'),
          (16, 64, 'small'), ('bye', 'rounds'), 'tall', 'wide', ('dim', 1), ('dim', 4), ('dim', 5), ('dim', 'k'),
          ('cut_below', 'rounds'), ('cut_above', 'gram'), ('tie', 'small'), ('tie', 'gram'), ('tie', 'rounds'),
          ('orthogonal', 'small'), ('orthogonal', 'gram'), ('orthogonal', 'rounds'), ('repeated_column', 'small'),
          ('repeated_column', 'rounds'), ('graded', 'small'), ('graded', 'gram'), ('graded', 'rounds')}
  assert want <= reached, want - reached
  # the k > 1 guard of the host loop: one vector beyond the LDS route reports one sweep and rotates nothing
  assert ee.svd_reference(ee.SvdCase(1, 7001, 1, 'graded', True))[3:] == ('rounds', 1)
  # the Gram matrix of the repeated column and of dim = k graded vectors falls below its cut
  assert ee.svd_reference(ee.SvdCase(8, 866, 8, 'repeated_column', True))[3] == 'rounds'
  assert ee.svd_reference(ee.SvdCase(8, 866, 8, 'graded', True))[3] == 'rounds'


def test_svd_preconditions():
  """The factor of 100 on either side of the Gram cut, on LAPACK's singular values; the ties are ties and the null
  places null; the orthogonal kind's dot products are exactly zero and its tied norms equal to the bit."""
  for c in ee.SVD_CASES:
    if c.k > 16 and c.kind not in ('cut_below', 'cut_above'):
      continue
    data = ee.svd_matrix(c)
    ss = np.linalg.svd(data.t, compute_uv=False)
    ratio = (ss[c.dim - 1] / ss[0]) ** 2
    if c.kind == 'cut_below':
      assert ratio * 0.99 * ee.CUT_MARGIN <= ee.GRAM_CUT <= ratio * 1.01 * ee.CUT_MARGIN, ratio
    if c.kind == 'cut_above':
      assert ee.GRAM_CUT * 0.99 * ee.CUT_MARGIN <= ratio <= ee.GRAM_CUT * 1.01 * ee.CUT_MARGIN, ratio
    for i, j in data.ties:
      assert abs(ss[i] - ss[j]) <= 8 * ee.U64 * ss[0]
    for i in data.null:
      assert ss[i] <= 8 * max(c.k, c.m) * ee.U64 * ss[0]
    if c.kind == 'orthogonal':
      g = data.t.T if c.tall else data.t
      gg = g @ g.T
      assert np.count_nonzero(gg - np.diag(np.diag(gg))) == 0 and gg[1, 1] == gg[2, 2]


def test_cca_tables_reach_every_branch():
  assert len(CCA) == len(ee.CCA_CASES)
  assert {ee.cca_k(c) for c in ee.FUSED_CASES} >= set(ee.FUSED_SHAPES)
  assert all(max(ee.cca_k(c)) <= 257 and ee.cca_rows(c) >= 200 for c in ee.CCA_CASES)
  reached = set()
  for c in ee.CCA_CASES:
    mom = ee.cca_cpu_moments(c)
    k1, k2 = ee.cca_k(c)
    for fused in (True, False):
      if c in ee.CHAIN_CASES and fused:
        continue                       # (the chain cases are run once: nothing switches)
      ref = ee.cca_reference(c, mom, fused)
      res = ref.resolved
      denom = ee.cca_denom(c, mom.frames)
      route = ee.cca_route(k1, k2, c.reg, ee.EPS_EIG, denom, mom.frames, ee.cca_options(c, fused))
      assert route.one_launch == (fused and c in ee.FUSED_CASES)
      where = 'one launch' if res.fused else 'chain'
      reached.add((where, 'x', res.route_x))
      reached.add((where, 'y', 'cholesky' if res.y_chol else 'eigen', 'dropped', ref.dropped_y))
      reached.add((where, 'svd', ref.svd_route))
      reached.add((where, 'proof' if route.psd_proof else 'certificate'))
      if res.fused:
        reached.add(('one launch', 'k1 - 4 k2', max(-1, min(1, k1 - 4 * k2)), ref.svd_route))
        reached.add(('one launch', 'dim', c.dim if c.dim < k2 else 'k2'))
        if c.dim > 4:
          reached.add(('one launch', 'want += 4', ref.svd_route))
        if c.l1 > 1:
          reached.add(('one launch', 'expanded moments'))
        if k2 & 1 and not res.y_chol:
          reached.add(('one launch', 'y eigen route', 'phantom player'))
      if route.one_launch and not res.fused:
        reached.add(('one launch', 'status 1'))
      if not res.fused:
        reached.add(('chain', 'k2', k2, res.route_x, res.route_y))
        reached.add(('chain', 'cols', route.cols))
        if c.whitening:
          reached.add(('chain', 'cca_whitening', route.cols))
  want = {
      ('one launch', 'x', 'cholesky'), ('one launch', 'y', 'cholesky', 'dropped', 0),
      ('one launch', 'y', 'eigen', 'dropped', 1),                      # the y side's eigen route inside the launch
      ('one launch', 'svd', 'gram'), ('one launch', 'svd', 'rounds'), ('one launch', 'proof'),
      ('one launch', 'certificate'), ('one launch', 'status 1'), ('one launch', 'expanded moments'),
      ('one launch', 'k1 - 4 k2', 0, 'gram'), ('one launch', 'k1 - 4 k2', -1, 'rounds'),
      ('one launch', 'k1 - 4 k2', 1, 'gram'), ('one launch', 'k1 - 4 k2', 0, 'rounds'),      # the Gram fall-back
      ('one launch', 'k1 - 4 k2', 1, 'rounds'), ('one launch', 'want += 4', 'gram'),
      ('one launch', 'want += 4', 'rounds'), ('one launch', 'dim', 1), ('one launch', 'dim', 4),
      ('one launch', 'dim', 5), ('one launch', 'dim', 'k2'), ('one launch', 'y eigen route', 'phantom player'),
      ('chain', 'k2', 16, 'cholesky', 'eigen'), ('chain', 'k2', 17, 'cholesky', 'cholesky'),
      ('chain', 'k2', 64, 'cholesky', 'cholesky'), ('chain', 'k2', 65, 'eigen', 'eigen'),
      ('chain', 'k2', 20, 'cholesky', 'eigen'),                         # chol2's certificate fails, x keeps its factor
      ('chain', 'k2', 20, 'eigen', 'cholesky'), ('chain', 'k2', 70, 'eigen', 'eigen'),
      ('chain', 'cols', True), ('chain', 'cols', False), ('chain', 'cca_whitening', True),
      ('chain', 'cca_whitening', False), ('chain', 'svd', 'small'), ('chain', 'svd', 'rounds'),
      ('chain', 'y', 'eigen', 'dropped', 1), ('chain', 'x', 'eigen'), ('chain', 'certificate'), ('chain', 'proof'),
  }
  assert want <= reached, want - reached
  # the thresholds of the routes themselves
  r = lambda k1, k2, **o: ee.cca_route(k1, k2, 0.1, ee.EPS_EIG, 99, 100, o)
  assert r(64, 16).one_launch and not r(65, 16).one_launch and not r(64, 17).one_launch and not r(12, 13).one_launch
  assert not r(64, 16, cca_fused=0).one_launch and not r(64, 16, cca_whitening=1).one_launch
  assert (r(70, 16).use_chol2, r(70, 17).use_chol2, r(70, 64).use_chol2, r(70, 65).use_chol2) == (False, True, True, False)
  assert r(70, 64).use_chol and not r(70, 65).use_chol and not r(12, 20).use_chol and r(12, 20).use_chol2
  assert not ee.cca_route(8, 2, 0.1, ee.EPS_EIG, 101, 100).psd_proof and not ee.cca_route(8, 2, 2e-12, 1e-12, 99, 100).psd_proof


@pytest.mark.parametrize('case', ee.CCA_CASES, ids=ee.cca_id)
def test_cca_preconditions_and_model_inside_the_bound(case):
  """On the CPU's sums: the gaps, the eigenvalue margins around eps_eig, at most one excluded component (deficient
  kinds only), and the model of the route taken inside the bound it helps to set -- for the one launch and the chain."""
  mom = ee.cca_cpu_moments(case)
  for fused in ((True, False) if case in ee.FUSED_CASES else (False,)):
    ref = ee.cca_reference(case, mom, fused)
    assert ref.pair.g >= 2.0 * ee.G_MIN, ref.pair.g
    excluded = int(np.sum(~ref.compared))
    assert excluded <= 1 and (excluded == 0 or case.kind in ('copy', 'zero'))
    cxx, cyy, _ = ref.cov
    for c in (cxx, cyy):
      assert ee.eig_margin(c)[1]
    if case.kind in ('copy', 'zero') and case.reg == 0.0:
      assert ee.eig_margin(cyy)[0] <= ee.EPS_EIG and ref.dropped_y == 1 and not ref.resolved.y_chol
      assert excluded == (1 if case.dim == ee.cca_k(case)[1] else 0)
    if case.kind == 'zero' and case.reg > 0.0:
      assert ref.dropped_y == 0 and excluded == 1 and ref.model.e[-1] == 0.0
    if case.kind == 'indefinite':
      assert ee.eig_margin(cxx)[0] < -100.0 * ee.EPS_EIG and not ref.resolved.fused and ref.resolved.route_x == 'eigen'
    if case.kind == 'uncorrelated':
      ratio = (ref.pair.e[-1] / ref.pair.e[0]) ** 2
      assert 0.0 < ratio < ee.GRAM_CUT_FUSED / 100.0 and ref.svd_route == ('rounds' if fused else 'small')
    rep = ee.cca_check(ee.model_outputs(ref), ref)
    assert not rep.failures and rep.ratio_e <= 1.0 and rep.ratio_rot <= 1.0, rep


EIG_CPU = [c for c in ee.EIG_CASES if c.n in (1, 2, 3, 17, 32, 63, 64, 65, 129)]


@pytest.mark.parametrize('case', EIG_CPU, ids=ee.eig_id)
def test_eig_model_inside_the_bound(case):
  """A subset of the sizes, for time (the GPU test builds the model of every row).  The model is a term of its own
  bound; what this holds is that the bound stays a rounding bound, what the model returns for diagonal input, and that a
  power-of-two scaling changes none of its bits."""
  lap, mod, model = ee.eig_reference(case)
  bound = ee.eig_bounds(case)
  assert all(m <= b for m, b in zip(mod, bound))
  assert all(b <= 8.0 * 64.0 * case.n * ee.U64 for b in bound), bound          # (the bound itself stays a rounding bound)
  if case.kind in ee.DIAGONAL_KINDS:
    a = ee.eig_matrix(case)
    assert np.array_equal(model.vecs, np.eye(case.n)) and np.array_equal(model.vals, np.diag(a))
  if case.kind in ee.SCALED_KINDS:
    plain = ee.eig_reference(ee.EigCase(case.n, 'pd'))[2]
    assert model.sweeps == plain.sweeps and model.rotations == plain.rotations
    assert np.array_equal(model.vals, plain.vals * ee.SCALED_KINDS[case.kind])         # (a power of two: the same bits)


@pytest.mark.parametrize('n', [3, 16, 17, 63, 64, 65])
def test_relative_accuracy_of_the_model_and_of_an_absolute_threshold(n):
  """The float64 model keeps the small eigenvalues of the graded matrix to ~1e-11 of themselves against the longdouble
  Jacobi; LAPACK agrees with that reference wherever it is accurate (the largest eigenvalues); a model whose rotation
  threshold is relative to the largest diagonal entry lands far outside 8 x the model's value."""
  case = ee.EigCase(n, 'graded')
  ref = ee.graded_reference(n)
  assert np.all(ref > 0)
  lap = np.linalg.eigvalsh(ee.eig_matrix(case))
  assert abs(lap[-1] - ref[-1]) <= 8 * n * ee.U64 * ref[-1]
  rel = ee.relative_error(ee.eig_reference(case)[2].vals, ref)
  assert rel <= 1e-10, rel
  wrong = ee.relative_error(ee.sym_eig_model(ee.eig_matrix(case), 'absolute').vals, ref)
  print('n %d: model %.3g, absolute threshold %.3g' % (n, rel, wrong))
  if n >= 16:                          # (three by three, either threshold converges to the same matrix)
    assert wrong > 8.0 * rel and wrong > 1e-7


SVD_CPU = [c for c in ee.SVD_CASES if c.k <= 16 or c.kind in ('cut_below', 'cut_above') or
           (c.kind in ('orthogonal', 'repeated_column') and c.tall)]


@pytest.mark.parametrize('case', SVD_CPU, ids=ee.svd_id)
def test_svd_model_inside_the_bound(case):
  """A subset of the table, for time: every shape up to 16 vectors, both Gram-cut kinds, the orthogonal and the
  repeated-column kinds.  The vector and the tie bounds are the gap term alone, so the model can miss them."""
  mod, lap_triplet, gaps, route, sweeps = ee.svd_reference(case)
  bound = ee.svd_bounds(case)
  assert mod.s_rel <= bound.s_rel and mod.s_null <= bound.s_null and np.all(mod.vec <= bound.vec)
  assert mod.triplet <= bound.triplet and mod.tie <= bound.tie
  assert (sweeps == 0) == (route in ('small', 'gram'))
  if case.kind == 'orthogonal':                    # no rotation at all: the rotation side is rows of the identity
    v = ee.jacobi_svd_model(ee.svd_matrix(case).t, case.dim)[2 if case.tall else 0]
    assert np.all((v == 0.0) | (v == 1.0)) and np.all(v.sum(axis=1) == 1.0) and sweeps <= 1


def test_a_nan_channel_gives_no_finite_correlation():
  """The models after the two fixes: whichever route the SVD takes, vectors that are all NaN end in the rounds (the
  Gram matrix's eigenvalues are not finite), every norm ranks 0, every wanted place stays at index 0 -- in range --
  and every e is NaN.  The selector that started from -1 indexed norms[-1]."""
  for k, m in ((8, 865), (8, 866), (31, 207), (65, 300)):
    r, picks = ee.nan_svd_outputs(k, m, 5)
    assert r.route != 'gram' and not np.any(np.isfinite(r.sig))
    assert min(picks) >= 0 and picks[1:] == [0, 0, 0, 0]
    assert min(ee.nan_svd_outputs(k, m, 5, start=-1)[1]) == -1
  assert ee.svd_route(31, 207) == 'gram' and ee.svd_route(31, 207, [1.0, np.nan] + [0.5] * 29, 5) == 'rounds'
  for name in ('reg_8x2', 'chain_70x17', 'chain_12x20'):
    case = CCA[name]
    mom = ee.cca_cpu_moments(case)
    sxx, sxy, sx = mom.sxx.copy(), mom.sxy.copy(), mom.sx.copy()
    sxx[1, :] = sxx[:, 1] = sxy[1, :] = sx[1] = np.nan
    k1, k2 = ee.cca_k(case)
    denom = ee.cca_denom(case, mom.frames)
    cxx, cyy, cxy, _, _ = ee.covariances(cs.Mom(sxx, mom.syy, sxy, sx, mom.sy, mom.frames), denom, case.reg)
    route = ee.cca_route(k1, k2, case.reg, ee.EPS_EIG, denom, mom.frames)
    out = ee.dense_model(cxx, cyy, cxy, case.dim, ee.EPS_EIG, route)
    assert not out.resolved.fused and out.resolved.route_x == 'eigen'       # no factor of a NaN matrix: the chain decides
    assert not np.any(np.isfinite(out.e))


# ---- wrong kernels ---------------------------------------------------------------------------------------------------
def test_wrong_phantom_player_lands_outside():
  case = ee.EigCase(63, 'pd')
  a = ee.eig_matrix(case)
  w = ee.sym_eig_model(a, 'phantom')
  got, bound = ee.eig_measure(a, w.vals, w.vecs), ee.eig_bounds(case)
  assert got.residual > bound.residual and got.orthogonality > bound.orthogonality and got.spectrum > bound.spectrum


def test_wrong_cross_only_round_lands_outside():
  """q = HB + tid in every cross-only round: 32 of the 1024 cross pairs are ever rotated."""
  case = ee.EigCase(65, 'pd')
  a = ee.eig_matrix(case)
  w = ee.sym_eig_model(a, 'cross_fixed')
  got, bound = ee.eig_measure(a, w.vals, w.vecs), ee.eig_bounds(case)
  assert got.residual > bound.residual and got.spectrum > bound.spectrum


def test_wrong_tie_rule_is_rejected_by_the_exact_order():
  """j > i: still a permutation, and inside every bound (a tied pair is compared by its span) -- what rejects it is the
  orthogonal kind, whose rotation side the GPU test holds to the model's rows of the identity, in order."""
  for k, m in ((8, 865), (8, 866)):
    case = ee.SvdCase(k, m, k, 'orthogonal', True)
    data = ee.svd_matrix(case)
    right = ee.jacobi_svd_model(data.t, k)
    wrong = ee.jacobi_svd_model(data.t, k, tie='higher')
    (i, j), = data.ties
    assert right[3] == wrong[3] == ee.svd_reference(case)[3]
    assert right[2][i].argmax() == 1 and right[2][j].argmax() == 2 and wrong[2][i].argmax() == 2
    assert not np.array_equal(right[2], wrong[2])


def test_wrong_gram_route_below_its_cut_lands_outside():
  for case in (ee.SvdCase(8, 866, 5, 'cut_below', True), ee.SvdCase(64, 256, 5, 'cut_below', True)):
    data = ee.svd_matrix(case)
    u, s, v, route, _ = ee.jacobi_svd_model(data.t, case.dim, wrong='gram_below_cut')
    assert route == 'gram' and ee.svd_measure(data, case.dim, u, s, v).s_rel > ee.svd_bounds(case).s_rel
  for name in ('uncorrelated_28x7', 'uncorrelated_64x16'):     # the one launch's own cut
    mom = ee.cca_cpu_moments(CCA[name])
    ref = ee.cca_reference(CCA[name], mom)
    bad = ee.cca_reference(CCA[name], mom, wrong='gram_below_cut')
    rep = ee.cca_check(ee.model_outputs(bad), ref)
    assert ref.svd_route == 'rounds' and bad.svd_route == 'gram' and rep.ratio_e > 1.0 and rep.ratio_rot > 1.0


def test_wrong_eigenvalue_filter_lands_outside():
  """lambda >= eps keeps the exactly zero eigenvalue of the zero column at eps_eig = 0: 0^-1/4."""
  for name in ('zero_8x2', 'zero_17x16'):
    mom = ee.cca_cpu_moments(CCA[name])
    ref = ee.cca_reference(CCA[name], mom)
    right = ee.cca_reference(CCA[name], mom, eps=0.0)
    assert right.dropped_y == 1 and not ee.cca_check(ee.model_outputs(right), ref).failures
    wrong = ee.cca_reference(CCA[name], mom, eps=0.0, wrong='filter_ge')
    rep = ee.cca_check(ee.model_outputs(wrong), ref)
    assert wrong.dropped_y == 0 and rep.ratio_e > 1.0 and rep.ratio_rot > 1.0
