"""CPU tests of the Cholesky / leave-one-out edge sweep (tests/chol_edges.py): the restated constants equal the
source's, the restated launch list updates every tile exactly once, the tables reach every branch the sweep names, the
numpy model of the kernel's algebra sits inside the bound it helps to set, the tables' data meet the bound's conditions
(conditioning, pivot margins), and six wrong kernels, modelled in numpy, land outside it.  No GPU needed."""
import collections

import numpy as np
import pytest

from tests import chol_edges as xe


def test_restated_constants_equal_the_source():
  found = xe.source_constants()
  assert set(found) == set(xe.CONSTANT_NAMES)
  for name, mine in xe.CONSTANT_NAMES.items():
    assert found[name] == getattr(xe, mine), name
  assert np.finfo(np.longdouble).eps < 2.0 ** -60          # the residuals of the bound are formed in np.longdouble


def test_every_launch_updates_every_tile_exactly_once():
  """Brute force over the grid: for nblk 1..10 and batch 1..17, both modes as the launch list has them, every
  system below `batch` gets every lower tile of the updated set and the right-hand-side row exactly once, tile 0 --
  the look-ahead tile (jlo, jlo) -- from workgroup 0, and no workgroup past `batch` does anything."""
  for nblk in range(1, 11):
    n = nblk * xe.NB
    for batch in range(1, 18):
      ow = xe.outer_cols(batch)
      ups = xe.updates(n, batch)
      assert len(xe.panels(n, batch)) == nblk
      assert len(ups) == nblk - 1                       # every diagonal block but the first is a look-ahead tile
      assert [u.jlo for u in ups] == list(range(1, nblk))
      for u in ups:
        assert u.col_mode == (1 if u.jlo % ow else 0) and u.kf == (u.jlo - 1) // ow * ow and u.kw == u.jlo - u.kf
        assert u.workers >= 2 and u.grid % u.workers == 0
        if u.col_mode:
          want = [(bi, u.jlo) for bi in range(u.jlo, nblk + 1)]
        else:
          want = [(bi, bj) for bj in range(u.jlo, nblk) for bi in list(range(bj, nblk)) + [nblk]]
        assert len(want) == u.n_tiles
        work = collections.Counter(xe.grid_work(u, batch))
        assert set(work.values()) == {1}
        assert set(work) == {(s, wk) for s in range(batch) for wk in range(u.workers)}
        got = collections.Counter()
        for wk in range(u.workers):
          tiles = [xe.tile_of(u, t, nblk) for t in xe.worker_tiles(u, wk)]
          assert tiles, (nblk, batch, u, wk)            # no idle bulk workgroup
          if wk == 0:
            assert tiles == [(u.jlo, u.jlo)]
          got.update(tiles)
        assert got == collections.Counter(want), (nblk, batch, u)
        assert xe.busiest_bulk(u) <= 3 or u.n_tiles - 1 > 3 * (u.workers - 1)
        systems = xe.grid_systems(u, batch)
        assert set(range(batch)) <= systems and max(systems) < (-(-batch // 8) * 8 if batch >= 8 else batch)
      for p in xe.panels(n, batch):
        wg, pos = xe.rhs_panel_slot(p, nblk)
        assert wg == p.workgroups - 1 and 0 <= pos < p.tiles_per_wg


def test_spd_table_reaches_every_branch():
  cases = xe.SPD_CASES
  assert len({xe.spd_id(c) for c in cases}) == len(cases) and 35 <= len(cases) <= 50
  assert {(c.n, c.nrhs, c.batch) for c in cases} >= set(xe.SPD_SIZE_LOOP)       # the loop of test_spd_solve_sizes
  assert {c.n for c in cases} >= {1, 2, 16, 17, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 448, 512, 513, 577}
  assert {c.batch for c in cases} >= {1, 2, 3, 7, 8, 9, 15, 16, 17}
  assert {c.nrhs for c in cases} >= {1, 2, 7, 8} and max(c.nrhs for c in cases) == xe.MAX_RHS
  assert max(c.n for c in cases) == 577
  reached = set()
  for c in cases:
    nblk = xe.n_blocks(c.n)
    ow = xe.outer_cols(c.batch)
    for u in xe.updates(c.n, c.batch):
      reached.add(('update', u.kw, 'column' if u.col_mode else 'trailing'))
      reached.add(('bulk walks', min(3, xe.busiest_bulk(u))))
      reached.add(('bulk walks', xe.laziest_bulk(u)))
      if xe.by_xcd(c.batch):
        last = c.batch - 8 * ((c.batch - 1) // 8)
        reached.add(('xcd group of', last, 'updated'))
    reached.add(('outer blocks', min(3, -(-nblk // ow)), 'ow', ow))
    reached.add(('batch', c.batch))
    if c.batch > 2:
      for p in xe.panels(c.n, c.batch):
        reached.add(('rhs row at', xe.rhs_panel_slot(p, nblk)[1]))
    if c.nrhs == xe.MAX_RHS:
      reached.add(('nrhs 8', 'ow', ow))
    if c.scale:
      reached.add(('scaled', c.batch, c.scale))
  want = {
      ('update', 1, 'column'), ('update', 2, 'column'), ('update', 3, 'column'),
      ('update', 1, 'trailing'), ('update', 4, 'trailing'),
      ('outer blocks', 2, 'ow', 4), ('outer blocks', 3, 'ow', 4), ('outer blocks', 3, 'ow', 1),
      ('batch', 1), ('batch', 2), ('batch', 3),
      ('xcd group of', 8, 'updated'), ('xcd group of', 1, 'updated'), ('xcd group of', 7, 'updated'),
      ('bulk walks', 3), ('bulk walks', 1),
      ('rhs row at', 0), ('rhs row at', 1), ('rhs row at', 2),
      ('nrhs 8', 'ow', 1), ('nrhs 8', 'ow', 4),
      ('scaled', 3, (1e-20, 1.0, 1e15)),
  }
  assert want <= reached, want - reached
  # chol_update_kernel<4> in trailing mode needs five blocks: n = 200 (the old loop's batched shape) never had it
  assert not any(u.kw == 4 for u in xe.updates(200, 3))
  # a ragged group's systems past `batch` exist in the grid and return
  u = xe.updates(193, 9)[0]
  assert xe.grid_systems(u, 9) == set(range(16)) and {s for s, _ in xe.grid_work(u, 9)} == set(range(9))


def test_ridge_and_loso_tables_reach_every_branch():
  ridge = xe.RIDGE_CASES
  assert len({xe.ridge_id(c) for c in ridge}) == len(ridge)
  assert {xe.stat_n(c) for c in ridge} == {64, 65, 256, 257, 513}
  assert {c.d for c in ridge if c.d <= xe.MAX_RHS} == {1, 8}
  assert {c.d for c in ridge if c.d > xe.MAX_RHS} == {9, 63, 64, 65, 73, 129}
  assert {c.n_lambda for c in ridge} == {1, 2, 3, 9} and {c.route for c in ridge} == {'solve', 'async', 'multi'}
  assert any(c.route == 'multi' and c.stats == 3 and c.n_lambda == 3 for c in ridge)
  nbs, trips = set(), set()
  for c in ridge:
    if c.d > xe.MAX_RHS:                               # ridge_solve_wide: 64 columns a factorisation, 8 rows a trip back
      for c0 in range(0, c.d, 64):
        nb = min(64, c.d - c0)
        nbs.add(nb)
        trips.add(nb - (-(-nb // 8) - 1) * 8)
  assert nbs == {63, 64, 1, 9} and {1, 7, 8} <= trips

  loso = xe.LOSO_CASES
  assert len({xe.loso_id(c) for c in loso}) == len(loso)
  plans = {c: xe.loso_plan(xe.stat_n(c), c.d, xe.loso_folds(c), c.n_lambda) for c in loso}
  assert {p.nblk for p in plans.values()} == {1, 2, 3, 4, 5, 7, 9}
  assert {p.ms[-1] for p in plans.values()} == {1, 2, 3, 4} and {p.nbig for p in plans.values()} == {1, 2, 3}
  assert any(p.nbig == 2 and xe.stat_n(c) < 2049 for c, p in plans.items())
  assert any(p.ms == (4,) for p in plans.values())                          # m = 4 with nothing beyond
  plain = {c: p for c, p in plans.items() if not c.as_terms}
  assert {c.d * c.n_files for c in plain} >= {1, 31, 32, 33, 35, 72}
  assert {c.n_lambda * c.d for c in plain} >= {1, 32, 35, 72}
  assert {c.n_lambda for c in loso} == {1, 2, 3, 4, 5, 8, 9}
  assert any(c.n_files == 1 for c in loso) and any(c.d == 8 for c in loso)
  # the row chunks: blockIdx.z >= 1 of the substitutions and of the matvec, full and partial last chunks
  assert {p.chunks for p in plans.values()} >= {1, 2, 3} and {p.mv_chunks for p in plans.values()} >= {1, 2, 3}
  assert {p.last_rows for p in plans.values() if p.chunks >= 2} >= {1, 3, 8}
  assert {p.last_rows for p in plans.values() if p.chunks == 1} >= {1, 31, 32}
  assert {p.mv_last_rows for p in plans.values() if p.mv_chunks >= 2} >= {3, 8}
  for c in loso:
    if c.d * c.n_files in (33, 35, 72):
      assert plans[c].chunks >= 2, c
  # the largest case: 33 recordings at n = 257, the smallest size with two big blocks
  big = [c for c in loso if c.n_files >= 31]
  assert big and all(xe.stat_n(c) == 257 and plans[c].nbig == 2 for c in big) and max(c.n_files for c in loso) == 33
  terms = [c for c in loso if c.as_terms]
  assert terms and all(min(xe.lambdas(c.n_lambda)) >= 1e-2 for c in loso)
  folds = xe.terms_folds(5)
  assert [len(f) for f in folds] == [3, 3, 3, 3, 1, 0]
  assert sorted(sg for _, sg in folds[0]) == [-1.0, -1.0, 1.0]


def test_singular_table_covers_the_blocks_and_positions():
  cases = xe.SINGULAR_CASES
  assert len({xe.singular_id(c) for c in cases}) == len(cases)
  n = xe.SINGULAR_N
  assert {c.j for c in cases if c.batch == 1} == {1, 15, 16, 63, 64, 79, 80, 255, 256, 320, n - 1}
  assert all(c.i < c.j < n for c in cases) and {c.batch for c in cases} == {1, 3, 9}
  for batch in (3, 9):
    members = {c.member for c in cases if c.batch == batch}
    assert members == {0, batch // 2, batch - 1}, members
  # which launch factors block j // 64: chol_diag_kernel, or the look-ahead workgroup of an update in either mode
  by = set()
  for c in cases:
    blk = c.j // xe.NB
    if blk == 0:
      by.add((xe.outer_cols(c.batch), 'diag', c.j % 16 in (0, 15)))
    else:
      u = xe.updates(n, c.batch)[blk - 1]
      assert u.jlo == blk
      by.add((xe.outer_cols(c.batch), 'column' if u.col_mode else 'trailing', u.kw))
  assert {(4, 'column', 1), (4, 'column', 3), (4, 'trailing', 4), (1, 'trailing', 1), (1, 'diag', True),
          (4, 'diag', True)} <= by, by


@pytest.mark.parametrize('case', xe.SINGULAR_CASES + [xe.NAN_CASE], ids=xe.singular_id)
def test_pivot_margins_of_the_singular_cases_and_their_twins(case):
  """Conditions on the inputs: the duplicated row leaves a pivot of at most t / 8 at step j (t = 64 n eps max|diag|),
  the twin's smallest pivot is at least 8 t; every other member of the batch is as safe as the twin."""
  if case is xe.NAN_CASE:
    a, rhs = xe.nan_system()
    sol = np.linalg.solve(a[case.member], rhs[case.member])       # the reference decides: NaN out, nothing raised
    assert not np.any(np.isfinite(sol))
    return
  bad, _ = xe.singular_system(case, False)
  good, _ = xe.singular_system(case, True)
  m = case.member
  t = xe.pivot_tolerance(bad[m])
  piv = xe.unblocked_pivots(bad[m], case.j)
  assert len(piv) == case.j + 1 and np.min(piv[:case.j]) >= 8.0 * t
  assert abs(piv[case.j]) <= t / 8.0, (piv[case.j], t)
  for k in range(case.batch):
    assert np.min(xe.unblocked_pivots(good[k])) >= 8.0 * xe.pivot_tolerance(good[k])
    if k != m:
      assert np.array_equal(bad[k], good[k])


def test_the_model_sits_inside_the_bound_it_helps_to_set():
  """The reference against the model, no device: each within 8 x the other (or 8 x 2^-53), both far below the
  a-priori cap; the tables' matrices have cond <= 5e3."""
  worst = 0.0
  for case in xe.SPD_CASES:
    ref = xe.spd_reference(case)
    floor = np.maximum(ref.eta_lapack, xe.U)
    assert np.all(ref.eta_model <= 8.0 * floor), xe.spd_id(case)
    assert np.all(ref.eta_lapack <= 8.0 * np.maximum(ref.eta_model, xe.U)), xe.spd_id(case)
    assert np.all(ref.bound <= 64.0 * xe.U) and np.all(ref.bound <= 8.0 * max(ref.cap, xe.U)), xe.spd_id(case)
    worst = max(worst, float(np.max(ref.eta_model / floor)))
    a, _ = xe.spd_system(case)
    if case.n > 1:
      ev = np.linalg.eigvalsh(a[0])
      assert ev[-1] / ev[0] <= 5e3
  assert worst <= 4.0, worst


def _ridge_cpu_reference(case, stat):
  files = xe.ridge_files(case, stat)
  xtx, xty, frames = xe.sum_moments([(xe.file_moments(x, y, case.pre, case.post), 1.0) for x, y in files])
  batch = case.n_lambda * (case.stats if case.d <= xe.MAX_RHS else 1)
  return xe.ridge_reference(xtx, xty, frames, xe.lambdas(case.n_lambda), batch)


@pytest.mark.parametrize('case', xe.RIDGE_CASES, ids=xe.ridge_id)
def test_ridge_bound_is_one_float32_rounding_on_the_tables_data(case):
  for stat in range(case.stats):
    ref = _ridge_cpu_reference(case, stat)
    assert xe.e_over_rounding(ref) <= 1.0, (xe.e_over_rounding(ref), ref.cond)
    assert np.all(ref.cond < 100.0), ref.cond


_LOSO_REFS = {}


def _loso_cpu_reference(case):
  if case not in _LOSO_REFS:
    _, folds = xe.loso_cpu_moments(case)
    _LOSO_REFS[case] = xe.loso_reference(folds, xe.lambdas(case.n_lambda))
  return _LOSO_REFS[case]


@pytest.mark.parametrize('case', xe.LOSO_CASES, ids=xe.loso_id)
def test_loso_bound_is_one_float32_rounding_on_the_tables_data(case):
  ref = _loso_cpu_reference(case)
  assert ref.w.shape == (xe.loso_folds(case), case.n_lambda, xe.stat_n(case) - 1, case.d)
  assert xe.e_over_rounding(ref) <= 1.0, (xe.e_over_rounding(ref), ref.cond.max())
  assert np.all(ref.cond < 100.0), ref.cond.max()
  # ... and the sweep's own stopping rule is within reach: the model of the iteration converges well inside 40 steps
  # on the fold least like the total, at the smallest lambda
  total, folds = xe.loso_cpu_moments(case)
  fold = int(np.argmin([f[2] for f in folds]))
  lam = xe.lambdas(case.n_lambda)[0]
  xtx, xty, frames = folds[fold]
  x, converged, iterations = xe.pcg_model(xtx / frames, xty[:, 0] / frames, lam, xe.preconditioner(total[0], total[2], lam))
  assert converged and iterations <= 30, iterations
  assert _loso_ratio(x, ref, fold, 0, 0) <= 1.0


# ---- the wrong kernels -----------------------------------------------------------------------------------------------
def _case(table, ident, text):
  (case,) = [c for c in table if ident(c) == text]
  return case


@pytest.mark.parametrize('wrong,text,member', [
    ('drop_last_kw', 'n257-rhs8-b3', 1),      # <4> in trailing mode: the last of four panel columns
    ('drop_last_kw', 'n129-rhs1-b2', 0),      # <1> in trailing mode: the only one
    ('skip_rhs_col', 'n129-rhs2-b3', 2),      # <1> and <2> in column mode
    ('skip_rhs_col', 'n193-rhs2-b9', 8),
    ('unfactored', 'n193-rhs2-b9', 8),        # the ragged group of 1
    ('unfactored', 'n129-rhs1-b15', 14),      # the last of a ragged group of 7
], ids=lambda v: str(v))
def test_wrong_factorisations_fail_the_bound(wrong, text, member):
  case = _case(xe.SPD_CASES, xe.spd_id, text)
  a, rhs = xe.spd_system(case)
  ref = xe.spd_reference(case)
  if wrong == 'unfactored':
    assert xe.by_xcd(case.batch) and case.batch % 8 and member == case.batch - 1 and xe.updates(case.n, case.batch)
  if wrong == 'skip_rhs_col':
    assert any(u.col_mode for u in xe.updates(case.n, case.batch))
  good = xe.model_solve(a[member], rhs[member], xe.outer_cols(case.batch))
  assert np.all(xe.backward_error(a[member], good, rhs[member], ref.a_norm[member]) <= ref.bound[member])
  bad = xe.model_solve(a[member], rhs[member], xe.outer_cols(case.batch), wrong)
  eta = xe.backward_error(a[member], bad, rhs[member], ref.a_norm[member])
  assert np.all(eta > 1e6 * ref.bound[member]), eta / ref.bound[member]


def _loso_system(case, fold, li, out):
  """(a_f, rhs, total xtx, total frames, lambdas, reference) of one system of a leave-one-out case."""
  total, folds = xe.loso_cpu_moments(case)
  xtx, xty, frames = folds[fold]
  return xtx / frames, xty[:, out] / frames, total[0], total[2], xe.lambdas(case.n_lambda), _loso_cpu_reference(case)


def _loso_ratio(x, ref, fold, li, out):
  bw, bb = xe.loso_bounds(ref)
  dw = np.abs(x[:-1] - ref.w[fold, li, :, out]) / bw[fold, li, :, out]
  return float(max(dw.max(), abs(x[-1] - ref.b[fold, li, out]) / bb[fold, li, out]))


@pytest.mark.parametrize('wrong', ['right', 'chunk 1 never preconditioned', 'last big block treated as full',
                                   'matvec chunk 1 reads the lambda of chunk 0'])
def test_wrong_loso_kernels_fail_the_checks(wrong):
  """What the GPU test asserts of every system: status converged within 40 iterations AND inside the bound."""
  if wrong == 'chunk 1 never preconditioned':
    case = _case(xe.LOSO_CASES, xe.loso_id, 'c16-pre0-post15-d1-f33-l2')
    fold, li, out = 32, 1, 0                               # row out * F + fold = 32: the second chunk's only row
    assert xe.loso_plan(257, 1, 33, 2).chunks == 2 and out * case.n_files + fold >= xe.LOSO_ROWS
  else:
    case = _case(xe.LOSO_CASES, xe.loso_id, 'c16-pre0-post7-d7-f5-l5')
    fold, li, out = 1, 4, 6                                # matvec row li * d + out = 34: the second chunk
    plan = xe.loso_plan(xe.stat_n(case), case.d, case.n_files, case.n_lambda)
    assert plan.ms == (3,) and plan.mv_chunks == 2 and li * case.d + out >= xe.LOSO_ROWS
  a_f, rhs, txx, tframes, lams, ref = _loso_system(case, fold, li, out)
  lam_mv = lams[li]
  precond = xe.preconditioner(txx, tframes, lams[li], zero_head=(wrong == 'last big block treated as full'))
  if wrong == 'chunk 1 never preconditioned':
    precond = lambda r: np.zeros_like(r)                   # z keeps the workspace's zeros
  if wrong == 'matvec chunk 1 reads the lambda of chunk 0':
    lam_mv = lams[(li * case.d + out - xe.LOSO_ROWS) // case.d]
    assert lam_mv != lams[li]
  x, converged, iterations = xe.pcg_model(a_f, rhs, lam_mv, precond)
  ratio = _loso_ratio(x, ref, fold, li, out)
  if wrong == 'right':
    assert converged and 1 <= iterations <= 40 and ratio <= 1.0, (converged, iterations, ratio)
  else:
    assert not converged or ratio > 100.0, (converged, iterations, ratio)
