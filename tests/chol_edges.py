"""The edge cases of the blocked float64 Cholesky (csrc/chol.hip), of the ridge routes over it (csrc/solve.hip) and of
the leave-one-out preconditioned-CG sweep (csrc/loso.hip) (tests/test_gpu_chol_edges.py, tests/test_cpu_chol_edges.py): the case tables, the data builders, the float64
references with their derived bounds, restatements of the integer arithmetic by which chol_factor_forward and
ridge_solve_loso_impl pick their launches, and numpy models of the kernel's algebra, right and wrong.  A plain module,
not a conftest.

td_spd_solve (float64 out) is held to a normwise backward error per right-hand-side column,
  eta(x) = ||b - A x||_2 / (||A||_2 ||x||_2)        (the residual formed in np.longdouble),
  eta_gpu <= 8 max(eta_lapack, eta_model, 2^-53)   and   eta_gpu <= n gamma_{3n+1}   (Higham, Cholesky solve):
eta_lapack is np.linalg.cholesky and two triangular solves of the same system, eta_model a numpy model of the kernel's
own algebra (64-blocks, explicit L_kk^-1 for panel and back-substitution, outer blocks of `ow` columns, the padding
diagonal = the largest real diagonal entry).  The 8 is the project's factor over a measured reference uncertainty (8 D
in cca_sweep_edges); it multiplies the reference and the model, never the kernel's own result.

The float32 ridge outputs, elementwise for w and b:   |gpu - ref| <= 2^-24 |ref| + E,
  E = cond_2(A) 8 max(eta_lapack, eta_model, 2^-53) ||[w; b]_ref||_2
with A = xtx / frames + lambda I (bias row included) and rhs = xty / frames from the device's own float64 moments, solved
by np.linalg.solve: cg_edges.reference, reused.  The leave-one-out calls add the stopping rule of their conjugate
gradients, E += 4 cond_2(A_f) tol ||ref||_2 (the form and the factor of cg_edges).  The tables keep E <= 2^-24 max|ref|
(lambdas >= 1e-2, recordings of about 4 (k + 1) frames): the bound is in effect one or two float32 roundings."""
import collections
import functools
import os
import re

import numpy as np

from oracle import lag as o_lag
from tests import cg_edges as ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the constants of solve_common.h / chol.hip / solve.hip / td_tile64.h, restated (tests/test_cpu_chol_edges.py reads them from the source) ----
NB = 64               # td_tile64::NB
MAX_RHS = 8           # kMaxRhs
OUTER_COLS = 4        # kOuterCols
PANEL_TILES = 3       # kPanelTiles
LOSO_ROWS = 32        # kLosoRows
BIG = 4               # kBig
CG_TOL = 1e-12        # kCgTol (and the default tol of ridge_solve_loso)
U = 2.0 ** -53        # unit roundoff of float64
EPS = 2.220446049250313e-16      # the literal of diag_tol_kernel

CONSTANT_NAMES = {'NB': 'NB', 'kMaxRhs': 'MAX_RHS', 'kOuterCols': 'OUTER_COLS', 'kPanelTiles': 'PANEL_TILES',
                  'kLosoRows': 'LOSO_ROWS', 'kBig': 'BIG', 'kCgTol': 'CG_TOL'}


def source_constants():
  """{name in the source: value} of the constants above, read from the text of the solver files of csrc/ and of
  csrc/td_tile64.h."""
  found = {}
  for name in ('solve_common.h', 'chol.hip', 'solve.hip', 'loso.hip', 'td_tile64.h'):
    with open(os.path.join(ROOT, 'telluride_decoding_amd', 'csrc', name)) as f:
      text = f.read()
    for m in re.finditer(r'constexpr\s+(int|double)\s+(\w+)\s*=\s*([-+.\w]+)\s*;', text):
      if m.group(2) in CONSTANT_NAMES:
        assert m.group(2) not in found, m.group(2)
        found[m.group(2)] = int(m.group(3)) if m.group(1) == 'int' else float(m.group(3))
  return found


# ---- the route arithmetic of chol_factor_forward, restated -----------------------------------------------------------
def padded(n):
  return -(-n // NB) * NB


def n_blocks(n):
  return padded(n) // NB


def outer_cols(batch):
  return 1 if batch <= 2 else OUTER_COLS


def panel_tiles(batch):
  return 1 if batch <= 2 else PANEL_TILES


def by_xcd(batch):
  return batch >= 8


# one launch of chol_update_kernel<kw> / of chol_panel_kernel
Update = collections.namedtuple('Update', 'kw col_mode kf jlo n_tri n_tiles workers grid')
Panel = collections.namedtuple('Panel', 'k tiles_per_wg workgroups')


def launches(n, batch):
  """The launches of chol_factor_forward behind chol_diag_kernel, in order."""
  nblk, ow, pt = n_blocks(n), outer_cols(batch), panel_tiles(batch)
  out = []

  def update(kf, kw, jlo, col_mode):
    rem = nblk - jlo
    tri = rem if col_mode else rem * (rem + 1) // 2
    n_tiles = rem + 1 if col_mode else tri + rem
    bulk = max(1, min((n_tiles - 1 + 2) // 3, n_tiles - 1))
    systems = -(-batch // 8) * 8 if by_xcd(batch) else batch
    out.append(Update(kw, col_mode, kf, jlo, tri, n_tiles, 1 + bulk, (1 + bulk) * systems))

  for kb in range(0, nblk, ow):
    cols = min(ow, nblk - kb)
    for q in range(cols):
      c = kb + q
      if q > 0:
        update(kb, q, c, 1)
      out.append(Panel(c, pt, (nblk - c + pt - 1) // pt))
    if kb + ow < nblk:
      update(kb, ow, kb + ow, 0)
  return out


def updates(n, batch):
  return [u for u in launches(n, batch) if isinstance(u, Update)]


def panels(n, batch):
  return [p for p in launches(n, batch) if isinstance(p, Panel)]


def grid_work(u, batch):
  """(sys, wk) of every workgroup of an update launch that passes `if (sys >= p.batch) return`."""
  for b in range(u.grid):
    slot = b >> 3 if by_xcd(batch) else b
    sys = (slot // u.workers) * 8 + (b & 7) if by_xcd(batch) else slot // u.workers
    if sys < batch:
      yield sys, slot % u.workers


def grid_systems(u, batch):
  """The `sys` values a grid produces, returned or not."""
  if not by_xcd(batch):
    return {b // u.workers for b in range(u.grid)}
  return {((b >> 3) // u.workers) * 8 + (b & 7) for b in range(u.grid)}


def tile_of(u, t, nblk):
  """upd_tile: (bi, bj) of tile t of an update launch; bi = nblk is the right-hand-side row."""
  if u.col_mode:
    return (u.jlo + t if t < u.n_tri else nblk), u.jlo
  if t < u.n_tri:
    ti = 0
    while (ti + 1) * (ti + 2) // 2 <= t:
      ti += 1
    return u.jlo + ti, u.jlo + (t - ti * (ti + 1) // 2)
  return nblk, u.jlo + (t - u.n_tri)


def worker_tiles(u, wk):
  """The tiles workgroup wk of a system walks: 0 (the look-ahead tile) or wk, wk + workers - 1, ..."""
  return [0] if wk == 0 else list(range(wk, u.n_tiles, u.workers - 1))


def busiest_bulk(u):
  return max(len(worker_tiles(u, wk)) for wk in range(1, u.workers))


def laziest_bulk(u):
  return min(len(worker_tiles(u, wk)) for wk in range(1, u.workers))


def rhs_panel_slot(p, nblk):
  """(workgroup, position among its tiles_per_wg tiles) of the right-hand-side row in a panel launch."""
  t = nblk - p.k - 1              # row tiles k + 1 .. nblk - 1, then the right-hand-side rows
  return t // p.tiles_per_wg, t % p.tiles_per_wg


LosoPlan = collections.namedtuple('LosoPlan', 'nblk nbig ms chunks last_rows mv_chunks mv_last_rows factor_batch')


def loso_plan(n, d, folds, n_lambda):
  """ridge_solve_loso_impl: the 256-wide steps (m 64-blocks each), the row chunks of the substitutions
  (blockIdx.z of loso_big_solve_kernel / loso_big_update_kernel) and of loso_matvec_kernel."""
  nblk = n_blocks(n)
  nbig = -(-nblk // BIG)
  ms = tuple(min(BIG, nblk - BIG * kb) for kb in range(nbig))
  rows, mv = d * folds, n_lambda * d
  chunks, mv_chunks = -(-rows // LOSO_ROWS), -(-mv // LOSO_ROWS)
  return LosoPlan(nblk, nbig, ms, chunks, rows - (chunks - 1) * LOSO_ROWS, mv_chunks,
                  mv - (mv_chunks - 1) * LOSO_ROWS, n_lambda)


# ---- the tables ------------------------------------------------------------------------------------------------------
SpdCase = collections.namedtuple('SpdCase', 'n nrhs batch scale why')      # scale: None or one factor per member


def _spd_table():
  t = []
  add = lambda n, nrhs, batch, why, scale=None: t.append(SpdCase(n, nrhs, batch, scale, why))
  # batch 1 and 2: the chain of one-column outer blocks (ow = 1, one tile per panel workgroup, kw = 1 trailing)
  add(1, 1, 1, 'one unknown (the size loop of test_spd_solve_sizes)')
  add(2, 2, 1, 'two unknowns, two right-hand sides')
  add(16, 1, 2, 'exactly the first 16-column sub-panel of factor_inv_tile')
  add(17, 7, 1, 'one column in the second sub-panel; 7 right-hand sides')
  add(63, 1, 2, 'one padding row (the size loop)')
  add(64, 2, 1, 'one full block, no padding (the size loop)')
  add(65, 3, 2, 'one real row in the second block (the size loop)')
  add(128, 8, 1, 'two full blocks; nrhs = kMaxRhs')
  add(129, 1, 2, 'three blocks: the first trailing update with a bulk tile below the look-ahead tile')
  add(192, 2, 2, 'three full blocks')
  add(193, 7, 1, 'four blocks')
  add(256, 1, 1, 'four full blocks')
  add(257, 8, 2, 'five blocks, 8 right-hand sides, two systems')
  add(320, 1, 1, 'five full blocks')
  add(321, 2, 2, 'six blocks: a bulk workgroup of the first trailing update walks 3 tiles')
  add(448, 1, 1, 'seven full blocks')
  add(512, 7, 2, 'eight full blocks')
  add(513, 4, 1, 'nine blocks (the size loop)')
  add(577, 8, 1, 'ten blocks: the largest system, kMaxRhs')
  # batch 3 .. 7: outer blocks of four columns, three tiles per panel workgroup, plain system order
  add(1, 1, 3, 'the first ow = 4 batch, one block: no update launch at all')
  add(64, 8, 3, 'one full block, kMaxRhs')
  add(65, 1, 3, 'two blocks: chol_update_kernel<1> in column mode; the rhs row second of a panel workgroup')
  add(129, 2, 3, 'three blocks: <2> in column mode; the rhs row first, second and third')
  add(200, 1, 3, 'four blocks: <3> in column mode (the size loop)')
  add(193, 7, 3, 'four blocks, 7 right-hand sides: the one bulk workgroup of <1> in column mode walks 3 tiles')
  add(256, 1, 3, 'four full blocks: one outer block exactly, no trailing update')
  add(257, 8, 3, 'five blocks: the first <4> in trailing mode, a second outer block of one column')
  add(321, 1, 3, 'six blocks: the trailing update has 5 tiles on two bulk workgroups')
  add(513, 2, 3, 'nine blocks: a third outer block; the first trailing update has 20 tiles')
  add(577, 7, 3, 'ten blocks: the third outer block has two columns')
  add(70, 2, 3, 'tol and the padding diagonal are per system: members scaled 1e-20, 1 and 1e15', (1e-20, 1.0, 1e15))
  add(65, 2, 7, 'the last batch in plain system order')
  add(257, 1, 7, 'seven systems through the trailing update')
  add(320, 8, 7, 'five full blocks, kMaxRhs, seven systems')
  # batch >= 8: the XCD-aware placement, grid rounded up to 8 systems
  add(64, 1, 8, 'by_xcd with one block: only the panel and diag launches')
  add(129, 8, 8, 'one full XCD group through <1> and <2> in column mode')
  add(257, 2, 8, 'one full XCD group through <4> in trailing mode')
  add(17, 1, 9, 'ragged group of 1, one block')
  add(193, 2, 9, 'ragged group of 1 through every column-mode instance')
  add(321, 7, 9, 'ragged group of 1 through the trailing update and the second outer block')
  add(129, 1, 15, 'ragged group of 7')
  add(65, 7, 16, 'two full groups')
  add(257, 1, 16, 'two full groups through the trailing update')
  add(2, 8, 17, 'two full groups and a ragged one, two unknowns')
  add(192, 1, 17, 'three groups, the last of 1: three full blocks')
  add(257, 2, 17, 'three groups, the last of 1, through <4> in trailing mode')
  return t


SPD_CASES = _spd_table()
SPD_SIZE_LOOP = ((1, 1, 1), (63, 1, 2), (64, 2, 1), (65, 3, 2), (200, 1, 3), (513, 4, 1))    # moved from test_gpu_fit.py


def spd_id(case):
  return 'n%d-rhs%d-b%d%s' % (case.n, case.nrhs, case.batch, '-scaled' if case.scale else '')


# route: 'solve' (ridge_solve on a handle set to 'cholesky'), 'async' (ridge_solve_async), 'multi' (ridge_solve_multi over
# `stats` statistics objects of different data)
RidgeCase = collections.namedtuple('RidgeCase', 'c pre post d n_lambda route stats why')

RIDGE_CASES = [
    RidgeCase(9, 0, 6, 1, 1, 'solve', 1, 'k + 1 = 64: one full block, one system'),
    RidgeCase(8, 0, 7, 8, 2, 'solve', 1, 'k + 1 = 65, d = kMaxRhs, two lambdas (the ow = 1 chain)'),
    RidgeCase(15, 0, 16, 1, 3, 'async', 1, 'k + 1 = 256, three lambdas: the first ow = 4 batch, asynchronous'),
    RidgeCase(16, 1, 14, 8, 9, 'solve', 1, 'k + 1 = 257, nine lambdas: a ragged XCD group, d = 8'),
    RidgeCase(64, 0, 7, 1, 2, 'solve', 1, 'k + 1 = 513'),
    RidgeCase(8, 0, 7, 8, 3, 'multi', 3, '3 statistics x 3 lambdas: a batch of 9'),
    RidgeCase(16, 0, 15, 1, 1, 'multi', 2, 'k + 1 = 257, two statistics x one lambda'),
    # wide targets: td_chol_factor with nb right-hand-side rows, td_chol_back 8 rows a trip
    RidgeCase(9, 0, 6, 9, 1, 'solve', 1, 'd = 9: nb = 9, the last trip of td_chol_back has 1 row'),
    RidgeCase(8, 0, 7, 63, 2, 'solve', 1, 'd = 63: nb = 63, last trip of 7 rows'),
    RidgeCase(15, 0, 16, 64, 1, 'solve', 1, 'd = 64: the right-hand-side tile is exactly 64 rows (full-tile load path)'),
    RidgeCase(8, 0, 7, 65, 1, 'async', 1, 'd = 65: nb = 64 then 1'),
    RidgeCase(16, 0, 15, 73, 1, 'multi', 2, 'd = 73: nb = 64 then 9, two statistics, k + 1 = 257'),
    RidgeCase(9, 0, 6, 129, 1, 'solve', 1, 'd = 129: nb = 64, 64, 1'),
]


def ridge_id(case):
  return 'c%d-pre%d-post%d-d%d-l%d-%s%d' % (case.c, case.pre, case.post, case.d, case.n_lambda, case.route, case.stats)


# n_files recordings; as_terms: td_ridge_solve_loso_terms with the folds of terms_folds() -- one more fold than files
LosoCase = collections.namedtuple('LosoCase', 'c pre post d n_files n_lambda as_terms why')

LOSO_CASES = [
    LosoCase(9, 0, 6, 1, 1, 1, False, 'nblk 1; one fold (the total itself), one row, one lambda'),
    LosoCase(8, 0, 7, 8, 4, 4, False, 'nblk 2, m = 2; d = 8: 32 rows per lambda and 32 matvec rows, one full chunk'),
    LosoCase(16, 0, 7, 7, 5, 5, False, 'nblk 3, m = 3; 35 rows per lambda and 35 matvec rows: a second chunk of 3'),
    LosoCase(16, 0, 11, 8, 9, 9, False, 'nblk 4, m = 4 with nothing beyond; 72 rows: three chunks; 9 lambdas'),
    LosoCase(16, 0, 15, 1, 33, 2, False, 'nblk 5, nbig 2, m = 1; 33 folds: a second chunk of one row'),
    LosoCase(16, 0, 15, 1, 31, 3, False, 'nblk 5; 31 rows: one chunk, one row masked'),
    LosoCase(16, 0, 23, 1, 3, 8, False, 'nblk 7, nbig 2, m = 3; 8 lambdas: one full XCD group of preconditioners'),
    LosoCase(16, 0, 31, 2, 3, 1, False, 'nblk 9, nbig 3, m = 1; one lambda'),
    LosoCase(16, 1, 14, 7, 5, 5, True, 'terms: a fold of zero terms, folds of three mixed-sign terms, k_major; 42 rows'),
    LosoCase(8, 0, 7, 1, 4, 9, True, 'terms: nblk 2, 9 lambdas (ragged XCD group of preconditioners)'),
]


def loso_id(case):
  return 'c%d-pre%d-post%d-d%d-f%d-l%d%s' % (case.c, case.pre, case.post, case.d, case.n_files, case.n_lambda,
                                             '-terms' if case.as_terms else '')


def stat_n(case):
  """Unknowns of a ridge / leave-one-out case: k + 1."""
  return case.c * (case.pre + 1 + case.post) + 1


def lambdas(n_lambda):
  """All >= 1e-2 (the bound's condition on the inputs), spread over three decades."""
  return [1e-2] if n_lambda == 1 else [float(v) for v in np.logspace(-2, 1, n_lambda)]


def loso_folds(case):
  return case.n_files + 1 if case.as_terms else case.n_files


TRUNCATED = 45      # frames the truncated twin of the last recording lacks (the terms cases)


def terms_folds(n_files):
  """The folds of a terms case over files 0 .. n_files - 1 and 'cut', the truncated twin of the last one:
  fold f < n_files - 1 = total - file f - last + cut (three mixed-sign terms), fold n_files - 1 = total - last,
  fold n_files = the total (zero terms).  [(name, sign), ...] per fold."""
  last = n_files - 1
  folds = [[(f, -1.0), (last, -1.0), ('cut', +1.0)] for f in range(last)]
  return folds + [[(last, -1.0)], []]


# SINGULAR_CASES: n = 321, row / column j an exact copy of row / column i < j in member `member` of `batch`
SingularCase = collections.namedtuple('SingularCase', 'j i batch member why')
SINGULAR_N = 321

SINGULAR_CASES = [
    SingularCase(1, 0, 1, 0, 'the second pivot of the first block'),
    SingularCase(15, 7, 1, 0, 'the last column of the first 16-column sub-panel'),
    SingularCase(16, 15, 1, 0, 'the first column of the second sub-panel'),
    SingularCase(63, 31, 1, 0, 'the last column of the first block'),
    SingularCase(64, 63, 1, 0, 'the first column of a block factored by the look-ahead workgroup (trailing mode, kw 1)'),
    SingularCase(79, 3, 1, 0, 'a sub-panel edge of the second block'),
    SingularCase(80, 79, 1, 0, 'the next sub-panel of the second block'),
    SingularCase(255, 128, 1, 0, 'the last column of the fourth block'),
    SingularCase(256, 0, 1, 0, 'the fifth block'),
    SingularCase(320, 319, 1, 0, 'the last real row, next to the padding'),
    SingularCase(15, 0, 3, 0, 'batch 3, first member: the first block (chol_diag_kernel)'),
    SingularCase(64, 1, 3, 1, 'batch 3, middle member: look-ahead of <1> in column mode'),
    SingularCase(255, 254, 3, 2, 'batch 3, last member: look-ahead of <3> in column mode'),
    SingularCase(256, 255, 3, 1, 'batch 3: look-ahead of <4> in trailing mode'),
    SingularCase(320, 64, 3, 0, 'batch 3: second outer block, column mode, the last real row'),
    SingularCase(16, 2, 9, 0, 'batch 9, first member'),
    SingularCase(79, 78, 9, 4, 'batch 9, middle member: column mode'),
    SingularCase(256, 100, 9, 8, 'batch 9, the ragged group\'s only member: trailing mode'),
    SingularCase(320, 300, 9, 8, 'batch 9, the ragged group\'s only member: the last real row'),
]
NAN_CASE = SingularCase(200, 100, 9, 4, 'a NaN at (200, 100) and (100, 200) of member 4 of 9')


def singular_id(case):
  return 'j%d-i%d-b%d-m%d' % (case.j, case.i, case.batch, case.member)


# ---- data ------------------------------------------------------------------------------------------------------------
def spd_matrices(n, batch, seed):
  """G G^T + 0.5 I with G [n, n + 8] standard normal: cond <= 5e3 at every n of the tables."""
  rng = np.random.default_rng([seed, n, batch])
  g = rng.standard_normal((batch, n, n + 8))
  return g @ g.transpose(0, 2, 1) + 0.5 * np.eye(n)


@functools.lru_cache(maxsize=None)
def spd_system(case):
  """(a [batch, n, n], rhs [batch, n, nrhs]) float64 of an SPD case; read-only."""
  a = spd_matrices(case.n, case.batch, 11)
  if case.scale:
    a = a * np.asarray(case.scale)[:, None, None]
  rhs = np.random.default_rng([12, case.n, case.nrhs, case.batch]).standard_normal((case.batch, case.n, case.nrhs))
  a.setflags(write=False)
  rhs.setflags(write=False)
  return a, rhs


@functools.lru_cache(maxsize=None)
def singular_system(case, twin):
  """(a [batch, n, n], rhs [batch, n, 1]): member `member` has row / column j an exact copy of row / column i; the twin
  has that copy's diagonal entry raised by 2^-10 of itself (pivot j = 2^-10 a_ii instead of rounding noise)."""
  n = SINGULAR_N
  a = spd_matrices(n, case.batch, 21).copy()
  m = a[case.member]
  m[case.j, :] = m[case.i, :]
  m[:, case.j] = m[:, case.i]
  assert m[case.j, case.j] == m[case.i, case.i] and np.array_equal(m, m.T)
  if twin:
    m[case.j, case.j] *= 1.0 + 2.0 ** -10
  rhs = np.random.default_rng([22, case.batch]).standard_normal((case.batch, n, 1))
  a.setflags(write=False)
  rhs.setflags(write=False)
  return a, rhs


def nan_system():
  case = NAN_CASE
  a = spd_matrices(SINGULAR_N, case.batch, 23).copy()
  a[case.member, case.j, case.i] = a[case.member, case.i, case.j] = np.nan
  rhs = np.random.default_rng([24, case.batch]).standard_normal((case.batch, SINGULAR_N, 2))
  return a, rhs


def pivot_tolerance(a):
  """tol of diag_tol_kernel: 64 n eps max|diag|."""
  return 64.0 * len(a) * EPS * np.max(np.abs(np.diag(a)))


def unblocked_pivots(a, upto=None):
  """The pivots of the unblocked right-looking float64 Cholesky of `a`, up to and including step `upto`; the sweep
  stops behind a pivot that is not positive."""
  a = np.array(a, np.float64)
  n = len(a)
  upto = n - 1 if upto is None else upto
  piv = np.empty(upto + 1)
  for j in range(upto + 1):
    piv[j] = a[j, j]
    if not piv[j] > 0.0:
      return piv[:j + 1]
    col = a[j + 1:, j] / np.sqrt(piv[j])
    a[j + 1:, j + 1:] -= np.outer(col, col)
  return piv


@functools.lru_cache(maxsize=None)
def make_files(c, pre, post, d, n_files, seed):
  """n_files recordings of white-noise EEG, float32, of about 4 (k + 1) frames and unequal length, with targets y =
  x mix / sqrt(c) + noise.  [(x [len, c], y [len, d]), ...]"""
  rng = np.random.default_rng([seed, c, pre, post, d, n_files])
  k1 = c * (pre + 1 + post) + 1
  mix = rng.standard_normal((c, d)) / np.sqrt(c)
  files = []
  for i in range(n_files):
    rows = 4 * k1 + 37 * i
    x = rng.standard_normal((rows, c)).astype(np.float32)
    y = (x @ mix + 0.5 * rng.standard_normal((rows, d))).astype(np.float32)
    files.append((x, y))
  return files


def file_moments(x, y, pre, post, rows=None):
  """(xtx [n, n], xty [n, d], frames) of one recording in float64 from the materialised lag matrix (oracle.lag), bias
  column last; rows: only the first `rows` frames (the truncated twin)."""
  lagged = o_lag.lag_matrix(x.astype(np.float64), pre, post)[:rows]
  lagged = np.concatenate((lagged, np.ones((len(lagged), 1))), axis=1)
  return lagged.T @ lagged, lagged.T @ y.astype(np.float64)[:len(lagged)], len(lagged)


def sum_moments(parts):
  """[(moments, sign), ...] -> summed (xtx, xty, frames)."""
  xtx = sum(sg * m[0] for m, sg in parts)
  xty = sum(sg * m[1] for m, sg in parts)
  return xtx, xty, int(round(sum(sg * m[2] for m, sg in parts)))


def ridge_files(case, stat):
  """The two recordings of statistics object `stat` of a ridge case."""
  return make_files(case.c, case.pre, case.post, case.d, 2, 31 + stat)


def loso_files(case):
  return make_files(case.c, case.pre, case.post, case.d, case.n_files, 41)


def loso_fold_parts(case):
  """Per fold the [(file index or 'cut', sign), ...] whose signed sum is the fold's training statistics."""
  nf = case.n_files
  if case.as_terms:
    everything = [(g, 1.0) for g in range(nf)]
    return [everything + terms for terms in terms_folds(nf)]
  if nf == 1:
    return [[(0, 1.0)]]                 # one recording: the only fold is the total itself
  return [[(g, 1.0) for g in range(nf) if g != f] for f in range(nf)]


@functools.lru_cache(maxsize=None)
def loso_cpu_moments(case):
  """(total, [fold moments]) of a leave-one-out case from the lag matrices in numpy."""
  files = loso_files(case)
  mom = {g: file_moments(x, y, case.pre, case.post) for g, (x, y) in enumerate(files)}
  x, y = files[-1]
  mom['cut'] = file_moments(x, y, case.pre, case.post, rows=len(x) - TRUNCATED)
  total = sum_moments([(mom[g], 1.0) for g in range(case.n_files)])
  return total, [sum_moments([(mom[g], sg) for g, sg in parts]) for parts in loso_fold_parts(case)]


# ---- the numpy model of the kernel's algebra -------------------------------------------------------------------------
def model_solve(a, rhs, ow, wrong=None):
  """a [n, n], rhs [n, nrhs] -> x [n, nrhs] by the algebra of chol_factor_forward / chol_backward for one system:
  identity padding with the largest real diagonal entry, 64-blocks, L_kk^-1 formed explicitly and applied as a
  product in the panel and in the back-substitution, outer blocks of `ow` columns (left-looking inside, one
  rank-64 ow update of the trailing matrix outside), the right-hand sides riding along as rows.
  wrong: None, or one of the planted errors
    'drop_last_kw'   the last of the kw panel columns missing from the last tile of the first trailing update
    'skip_rhs_col'   the right-hand-side row skipped by every column-mode update
    'unfactored'     no update launch reaches this system (a ragged XCD group's member that returns early): the
                     look-ahead tiles stay as they are, their inverses are the workspace's zeros."""
  a, rhs = np.asarray(a, np.float64), np.asarray(rhs, np.float64)
  n, nrhs = rhs.shape
  npad = padded(n)
  nblk = npad // NB
  top = np.max(np.abs(np.diag(a)))
  big = np.zeros((npad, npad))
  big[:n, :n] = a
  idx = np.arange(n, npad)
  big[idx, idx] = top if top > 0.0 else 1.0
  rt = np.zeros((nrhs, npad))
  rt[:, :n] = rhs.T
  linv = [np.zeros((NB, NB)) for _ in range(nblk)]
  blk = lambda i: slice(i * NB, (i + 1) * NB)
  dropped = []

  def factor(k):
    t = big[blk(k), blk(k)]
    low = np.linalg.cholesky(np.tril(t) + np.tril(t, -1).T)
    t[:] = low
    linv[k] = np.linalg.solve(low, np.eye(NB))

  def update(kf, kw, jlo, col_mode):
    if wrong == 'unfactored':
      return
    cols = slice(kf * NB, (kf + kw) * NB)
    for bj in ([jlo] if col_mode else range(jlo, nblk)):
      xj = big[blk(bj), cols]
      for bi in range(bj, nblk):
        use = cols
        if wrong == 'drop_last_kw' and not col_mode and not dropped and (bi, bj) == (nblk - 1, nblk - 1):
          use = slice(kf * NB, (kf + kw - 1) * NB)
          dropped.append((bi, bj))
        big[blk(bi), blk(bj)] -= big[blk(bi), use] @ big[blk(bj), use].T
      if not (wrong == 'skip_rhs_col' and col_mode):
        rt[:, blk(bj)] -= rt[:, cols] @ xj.T
    factor(jlo)

  def panel(c):
    for bi in range(c + 1, nblk):
      big[blk(bi), blk(c)] = big[blk(bi), blk(c)] @ linv[c].T
    rt[:, blk(c)] = rt[:, blk(c)] @ linv[c].T

  factor(0)
  for kb in range(0, nblk, ow):
    cols = min(ow, nblk - kb)
    for q in range(cols):
      if q > 0:
        update(kb, q, kb + q, 1)
      panel(kb + q)
    if kb + ow < nblk:
      update(kb, ow, kb + ow, 0)
  sol = np.zeros((nrhs, npad))
  for k in range(nblk - 1, -1, -1):
    w = rt[:, blk(k)] @ linv[k]                    # w_k = L_kk^-T z_k
    sol[:, blk(k)] = w
    for m in range(k):
      rt[:, blk(m)] -= w @ big[blk(k), blk(m)]     # z_m -= L_km^T w_k
  return sol[:, :n].T.copy()


def lapack_solve(a, rhs):
  """np.linalg.cholesky and the two triangular solves."""
  low = np.linalg.cholesky(a)
  return np.linalg.solve(low.T, np.linalg.solve(low, rhs))


def norm2(a):
  return float(np.max(np.abs(np.linalg.eigvalsh(a))))


def backward_error(a, x, b, a_norm=None):
  """eta per right-hand-side column, the residual in np.longdouble."""
  assert np.finfo(np.longdouble).eps < 2.0 ** -60
  a_norm = norm2(a) if a_norm is None else a_norm
  al, xl = np.asarray(a, np.longdouble), np.asarray(x, np.longdouble)
  r = np.asarray(b, np.longdouble) - al @ xl
  num = np.sqrt(np.sum(r * r, axis=0))
  den = np.longdouble(a_norm) * np.sqrt(np.sum(xl * xl, axis=0))
  return np.asarray(num / den, np.float64)


def apriori_cap(n):
  """n gamma_{3n+1}: Higham, Accuracy and Stability, theorem 10.4 (Cholesky solve), for any order of summation."""
  k = 3 * n + 1
  return n * (k * U) / (1.0 - k * U)


SpdReference = collections.namedtuple('SpdReference', 'a_norm eta_lapack eta_model bound cap')   # [batch, nrhs] each


@functools.lru_cache(maxsize=None)
def spd_reference(case):
  a, rhs = spd_system(case)
  return system_reference(a, rhs)


def system_reference(a, rhs, skip=()):
  """The reference of a batch: per member and right-hand-side column eta of LAPACK and of the model, and the bound
  8 max(eta_lapack, eta_model, 2^-53).  Members in `skip` (not finite) get NaN."""
  batch, n, nrhs = rhs.shape
  ow = outer_cols(batch)
  a_norm = np.full(batch, np.nan)
  el, em = np.full((batch, nrhs), np.nan), np.full((batch, nrhs), np.nan)
  for m in range(batch):
    if m in skip:
      continue
    a_norm[m] = norm2(a[m])
    el[m] = backward_error(a[m], lapack_solve(a[m], rhs[m]), rhs[m], a_norm[m])
    em[m] = backward_error(a[m], model_solve(a[m], rhs[m], ow), rhs[m], a_norm[m])
  return SpdReference(a_norm, el, em, 8.0 * np.maximum(np.maximum(el, em), U), apriori_cap(n))


def spd_distance(a, rhs, x, ref, skip=()):
  """(eta_gpu [batch, nrhs], the largest eta_gpu / bound) of a device solution x [batch, n, nrhs]."""
  eta = np.full(ref.bound.shape, np.nan)
  for m in range(len(a)):
    if m not in skip:
      eta[m] = backward_error(a[m], x[m], rhs[m], ref.a_norm[m])
  return eta, float(np.nanmax(eta / ref.bound))


# ---- the float32 ridge outputs ---------------------------------------------------------------------------------------
def ridge_reference(xtx, xty, frames, lams, batch, cg_tol=0.0):
  """cg_edges.reference of A = xtx / frames + lambda I, rhs = xty / frames, with this module's E:
  cond 8 max(eta_lapack, eta_model, 2^-53) ||sol||_2 per output, + 4 cond cg_tol ||sol||_2 for the leave-one-out calls.
  batch: systems the device factors at once (the model's outer blocks)."""
  ref = ce.reference(xtx, xty, frames, lams, 1.0)          # e = 4 cond TOL ||sol||
  xtx, xty = np.asarray(xtx, np.float64), np.asarray(xty, np.float64)
  n = len(xtx)
  e = np.empty_like(ref.e)
  for li, lam in enumerate(lams):
    a = xtx / frames + lam * np.eye(n)
    rhs = xty / frames
    a_norm = norm2(a)
    eta = np.maximum(backward_error(a, lapack_solve(a, rhs), rhs, a_norm),
                     backward_error(a, model_solve(a, rhs, outer_cols(batch)), rhs, a_norm))
    unit = ref.e[li] / (4.0 * ce.TOL)                      # cond ||sol||_2 per output
    e[li] = unit * 8.0 * np.maximum(eta, U) + 4.0 * unit * cg_tol
  return ref._replace(e=e)


def loso_reference(fold_moments, lams, cg_tol=CG_TOL):
  """Per fold the ridge_reference of its own moments (xtx, xty, frames), stacked as the device returns them:
  w [folds, n_lambda, k, d], b [folds, n_lambda, d], cond / e likewise."""
  refs = [ridge_reference(xtx, xty, frames, lams, len(lams), cg_tol) for xtx, xty, frames in fold_moments]
  return ce.Reference(*(np.stack([getattr(r, f) for r in refs]) for f in ce.Reference._fields))


def loso_bounds(ref):
  return 2.0 ** -24 * np.abs(ref.w) + ref.e[:, :, None, :], 2.0 ** -24 * np.abs(ref.b) + ref.e


def loso_distance(w, b, ref):
  bw, bb = loso_bounds(ref)
  dw, db = np.abs(np.asarray(w, np.float64) - ref.w), np.abs(np.asarray(b, np.float64) - ref.b)
  return float(dw.max()), float(db.max()), float(max((dw / bw).max(), (db / bb).max()))


def e_over_rounding(ref):
  """The largest E / (2^-24 max|ref|) over the systems and outputs of a reference: <= 1 is the tables' condition."""
  axis = -2
  top = np.maximum(np.max(np.abs(ref.w), axis=axis), np.abs(ref.b))
  return float(np.max(ref.e / (2.0 ** -24 * top)))


# ---- numpy models of the leave-one-out sweep, right and wrong --------------------------------------------------------
def pcg_model(a_f, rhs, lam_matvec, precond, max_iter=40, tol=CG_TOL):
  """One system of ridge_solve_loso_impl: preconditioned conjugate gradients on (a_f + lam_matvec I) x = rhs with
  z = precond(r); convergence looked at after iteration 3 and every later one.  (x, converged, iterations)"""
  x = np.zeros_like(rhs)
  r = rhs.copy()
  z = precond(r)
  p = z.copy()
  rz = r @ z
  bb = rhs @ rhs
  for it in range(1, max_iter + 1):
    q = a_f @ p + lam_matvec * p
    s = p @ q
    alpha = rz / s if s > 0.0 else 0.0
    x = x + alpha * p
    r = r - alpha * q
    z = precond(r)
    s = r @ z
    beta = s / rz if rz > 0.0 else 0.0
    p = z + beta * p
    rz = s
    if it >= min(3, max_iter) and r @ r <= tol * tol * bb:
      return x, True, it
  return x, False, max_iter


def preconditioner(total_xtx, total_frames, lam, zero_head=False):
  """r -> (P + lambda I)^-1 r by the Cholesky factor of the total's matrix.  zero_head: the planted error of a last
  big block of three 64-blocks treated as full -- the workgroup of its nonexistent fourth tile stores 64 numbers past
  the end of a row, onto the first 64 of the next row's forward-substituted vector (rows are np numbers apart); the
  tiles of X it multiplies by were never written, so it stores the workspace's zeros."""
  low = np.linalg.cholesky(np.asarray(total_xtx) / total_frames + lam * np.eye(len(total_xtx)))

  def apply(r):
    y = np.linalg.solve(low, r)
    if zero_head:
      y[:NB] = 0.0
    return np.linalg.solve(low.T, y)
  return apply
