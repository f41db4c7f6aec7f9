"""The edge cases of the Jacobi eigen-solver, the one-sided Jacobi SVD and the CCA dense stage of csrc/eig.hip
(tests/test_gpu_eig_edges.py, tests/test_cpu_eig_edges.py): the case tables, the data builders, float64 / longdouble
references with their derived bounds, restatements of the arithmetic by which the host and the kernels pick a route, and
numpy models of the kernels' algebra, right and wrong.  A plain module, not a conftest.

td_sym_eigh, normwise, each quantity q held to  q_gpu <= 8 max(q_lapack, q_model, n 2^-53):
  residual   ||A V - V diag(vals)||_F / ||A||_F          (formed in np.longdouble)
  orthogonality  ||V^T V - I||_F
  spectrum   ||sort(vals) - eigvalsh(A)||_2 / ||A||_F    (q_lapack: LAPACK's residual, which bounds its own eigenvalue
             errors by Weyl's inequality; q_model: the model's distance to LAPACK)
The 8 is the project's factor over a measured reference uncertainty (8 D in cca_sweep_edges, 8 eta in chol_edges); it
multiplies the reference and the model, never the kernel's own result.  Relative accuracy, graded positive definite
matrices only: max |vals - ref| / ref against the same cyclic Jacobi in np.longdouble (threshold 1e-18), held to 8 x the
float64 model's own value.

td_jacobi_svd: s within rtol = 8 max(model's relative error against LAPACK, 2^-53 max(m, n)) and, for the components
the table declares null, the same as an absolute bound relative to s_1; 1 - |u_i . u_ref| and 1 - sign v_i . v_ref (one
sign per pair) within the gap term 64 (m + n) 2^-53 / g_i; T v_i = s_i u_i normwise within
8 max(model, LAPACK, max(m, n) 2^-53); tied singular values by the projector on the span of their vectors, within the
gap term of the tied places (g: the group's distance to the other singular values).

td_cca_solve: the bound of cca_sweep_edges as it stands (pair_bounds), R1 the eigh / svd route, R2 the model of the
algebra the case takes (one launch or chain; Cholesky or eigen whitening per side; Gram matrix or rounds), both from
the device's own float64 moments.  Means bit for bit np.float32(sum * (1.0 / frames))."""
import collections
import functools
import os
import re

import numpy as np

from tests import cca_sweep_edges as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the constants of eig.hip / td_tile64.h, restated (tests/test_cpu_eig_edges.py reads them from the source) ------
NB = 64                      # td_tile64::NB
HB = 32                      # HB
ROT_TOL = 1e-15              # kRotTol
MAX_OUTER_SWEEPS = 40        # kMaxOuterSweeps
MAX_INNER_SWEEPS = 1         # kMaxInnerSweeps
SMALL_SVD_DOUBLES = 7000     # kSmallSvdDoubles
FLOOR = 1e-290               # below it nothing is rotated (jacobi_rotation, the SVD rounds)
GRAM_CUT = 1e-10             # jacobi_svd: lam[dim - 1] > 1e-10 lam[0]
GRAM_CUT_FUSED = 1e-8        # cca_small_kernel: low > 1e-8 top
FUSED_K1 = 64                # td_cca_one_launch: k1 <= NB
FUSED_K2 = 16                # ... k2 <= 16 (and the chain's second Cholesky starts above it)
CHOL_K2 = 64                 # the chain's Cholesky whitenings: k2 <= 64
PIVOT_FACTOR = 64.0          # pivot tolerance 64 k eps max|diag|
EPS = 2.220446049250313e-16  # the literal of that tolerance
EPS_EIG = cs.EPS_EIG
G_MIN = cs.G_MIN
U32, U64 = cs.U32, cs.U64
LD_TOL = 1e-18               # rotation threshold of the longdouble reference

CONSTANT_NAMES = {'NB': 'NB', 'HB': 'HB', 'kRotTol': 'ROT_TOL', 'kMaxOuterSweeps': 'MAX_OUTER_SWEEPS',
                  'kMaxInnerSweeps': 'MAX_INNER_SWEEPS', 'kSmallSvdDoubles': 'SMALL_SVD_DOUBLES'}
# literals that have no name in the source: {mine: (pattern with one group, occurrences)}
LITERALS = {
    'FLOOR': (r'(?:mag2?|m2) > (1e-290)', 6),
    'GRAM_CUT': (r'lam\[dim - 1\] > (1e-10) \* lam\[0\]', 1),
    'GRAM_CUT_FUSED': (r'low > (1e-8) \* top', 1),
    'FUSED_K2': (r'return k1 <= NB && k2 <= (16) && k2 <= k1 &&', 1),
    'CHOL_K2': (r'bool use_chol = k2 <= (64) && cols && !force_eig', 1),
    'PIVOT_FACTOR': (r'(64\.0) \* k[12] \* 2\.220446049250313e-16', 2),
    'EPS': (r'64\.0 \* k[12] \* (2\.220446049250313e-16)', 2),
}


def source_constants():
  """{my name: value} of the constants above, read from the text of csrc/eig.hip and csrc/td_tile64.h."""
  found = {}
  texts = {}
  for name in ('eig.hip', 'td_tile64.h'):
    with open(os.path.join(ROOT, 'telluride_decoding_amd', 'csrc', name)) as f:
      texts[name] = f.read()
    for m in re.finditer(r'constexpr\s+(int|double)\s+(\w+)\s*=\s*([-+.\w]+)\s*;', texts[name]):
      if m.group(2) in CONSTANT_NAMES:
        assert CONSTANT_NAMES[m.group(2)] not in found, m.group(2)
        found[CONSTANT_NAMES[m.group(2)]] = int(m.group(3)) if m.group(1) == 'int' else float(m.group(3))
  for mine, (pattern, count) in LITERALS.items():
    hits = re.findall(pattern, texts['eig.hip'])
    assert len(hits) == count and len(set(hits)) == 1, (mine, hits)
    found[mine] = float(hits[0])
  m = re.search(r'use_chol2 = k2 > (\d+) && k2 <= (\d+) && !force_eig', texts['eig.hip'])
  found['CHOL2'] = (int(m.group(1)), int(m.group(2)))
  return found


# ---- the route arithmetic, restated ---------------------------------------------------------------------------------
def _round_up(v, m):
  return -(-v // m) * m


def rr_pair(n_players, rnd, k):
  """Pair k of round rnd of the round-robin of an even number of players, as (p, q) with p < q."""
  m = n_players - 1
  if k == 0:
    a, b = rnd, m
  else:
    a = rnd + k
    a = a - m if a >= m else a
    b = rnd + m - k
    b = b - m if b >= m else b
  return (a, b) if a < b else (b, a)


def players(n):
  """Players of a direct problem: n rounded up to even, at least 2 (an odd n plays with a phantom: a zero row)."""
  return max(2, n + (n & 1))


def direct_rounds(n_players):
  """[(p [pairs], q [pairs])] of one sweep of the cyclic ordering."""
  out = []
  for rnd in range(n_players - 1):
    pq = [rr_pair(n_players, rnd, k) for k in range(n_players // 2)]
    out.append((np.array([p for p, _ in pq]), np.array([q for _, q in pq])))
  return out


def cross_rounds(fixed=False):
  """The cross-only rounds of a block pair's 64 x 64 sub-problem: p in the first block, q = HB + (p + round) mod HB.
  fixed: the wrong kernel whose q does not move with the round."""
  p = np.arange(HB)
  return [(p, HB + ((p + (0 if fixed else rnd)) & (HB - 1))) for rnd in range(HB)]


BlockPlan = collections.namedtuple('BlockPlan', 'np nblocks pairs launches')


def block_plan(n):
  """The block route (n > NB): the padded size, the 32-wide blocks, the block pairs of a round, and the
  (round, pairs, cross_only) launches of jacobi64_kernel in one outer sweep."""
  np_ = _round_up(n, NB)
  nblocks = np_ // HB
  return BlockPlan(np_, nblocks, nblocks // 2, tuple((r, nblocks // 2, r > 0) for r in range(nblocks - 1)))


def svd_small_doubles(k, m):
  return k * (m | 1) + k * (k | 1) + k


def svd_route(k, m, lam=None, dim=None):
  """jacobi_svd on k vectors of length m: 'small' (one workgroup), 'gram' or 'rounds'.  lam: the Gram matrix's
  eigenvalues, without which 'gram' only says that the Gram matrix is formed."""
  if svd_small_doubles(k, m) <= SMALL_SVD_DOUBLES:
    return 'small'
  if 1 < k <= NB and m >= 4 * k:
    if lam is None:
      return 'gram'
    lam = np.asarray(lam, np.float64)
    if np.all(np.isfinite(lam)):
      lam = np.sort(lam)[::-1]
      if lam[0] > 0.0 and lam[dim - 1] > GRAM_CUT * lam[0]:
        return 'gram'
  return 'rounds'


Route = collections.namedtuple('Route', 'one_launch psd_proof use_chol use_chol2 cols')


def cca_route(k1, k2, reg, eps, denom, frames, options=None):
  """What td_cca_dense decides from the sizes and the options ({'cca_whitening': 0 | 1, 'cca_fused': 1 | 0}) alone.
  use_chol / use_chol2: the chain tries the Cholesky whitening of that side (a certificate or a factorisation may
  still refuse it: resolve)."""
  options = options or {}
  force_eig = options.get('cca_whitening', 0) == 1
  cols = k2 <= k1
  psd_proof = reg > 2.0 * eps and denom <= frames
  one_launch = k1 <= FUSED_K1 and k2 <= FUSED_K2 and cols and not force_eig and bool(options.get('cca_fused', 1))
  return Route(one_launch, psd_proof, k2 <= CHOL_K2 and cols and not force_eig,
               FUSED_K2 < k2 <= CHOL_K2 and not force_eig, cols)


def pivots_ok(c):
  """The factorisation's verdict: every pivot above 64 k eps max|diag| (NaN: no)."""
  if not np.all(np.isfinite(c)):
    return False
  return cs.smallest_pivot(c) > PIVOT_FACTOR * len(c) * EPS * np.max(np.abs(np.diag(c)))


def whitening_ok(c, route, eps):
  """A side may take its Cholesky whitening: the inertia certificate (unless the proof by regularisation holds) and
  the factorisation itself."""
  return (route.psd_proof or pivots_ok(c - eps * np.eye(len(c)))) and pivots_ok(c)


Resolved = collections.namedtuple('Resolved', 'fused route_x route_y y_chol')


def resolve(route, cxx, cyy, eps):
  """(last_cca_fused, last_cca_route, last_cca_route_y) as the device reports them, and y_chol: whether the y side is
  whitened by its Cholesky factor.  The one launch always reports ('cholesky', 'eigen'): its choice for the y side
  stays inside the kernel."""
  if route.one_launch and whitening_ok(cxx, route, eps):
    return Resolved(True, 'cholesky', 'eigen', whitening_ok(cyy, route, eps))
  x = route.use_chol and whitening_ok(cxx, route, eps)
  y = route.use_chol2 and whitening_ok(cyy, route, eps)
  return Resolved(False, 'cholesky' if x else 'eigen', 'cholesky' if y else 'eigen', y)


# ---- numpy models of the kernels' algebra ---------------------------------------------------------------------------
def rotations(app, aqq, apq, formula='rcp', tol=ROT_TOL, absolute=None):
  """(c, s, rotated) of the pairs.  formula 'rcp': jacobi_rotation, t = b / (d + sign(d) hypot(d, b)); 'rs':
  jacobi_rotation_rs, c^2 = (1 + |d| / h) / 2.  absolute: the wrong threshold tol * absolute instead of
  tol sqrt|a_pp a_qq|."""
  mag2 = apq * apq
  ref = np.abs(app * aqq) if absolute is None else absolute * absolute
  with np.errstate(all='ignore'):
    rot = (mag2 > FLOOR) & (mag2 > (tol * tol) * ref)
    d, b = aqq - app, 2 * apq
    if formula == 'rcp':
      t = b / (d + np.copysign(np.sqrt(d * d + b * b), d))
      c = 1 / np.sqrt(1 + t * t)
      s = t * c
    else:
      rh = 1 / np.sqrt(d * d + b * b)
      x2 = 0.5 + 0.5 * np.abs(d) * rh
      r2 = 1 / np.sqrt(x2)
      c = x2 * r2
      s = np.where(d >= 0, 0.5, -0.5) * b * rh * r2
  one, zero = np.ones_like(mag2), np.zeros_like(mag2)
  return np.where(rot, c, one), np.where(rot, s, zero), rot


def jacobi_lds(s_mat, rounds, max_sweeps, formula='rcp', tol=ROT_TOL, absolute=False, quick_reject=True,
               skip_idle_rounds=False):
  """The sweeps of jacobi64_kernel (quick_reject) or jacobi_wave16 (skip_idle_rounds) on s_mat, in place: every
  round's disjoint rotations from the current diagonal, S <- R^T S R (columns, then rows), J <- J R.
  (J, rotations applied, sweeps run)."""
  n = len(s_mat)
  j_mat = np.eye(n, dtype=s_mat.dtype)
  top = np.max(np.abs(np.diag(s_mat))) if absolute else None
  finite = bool(np.all(np.isfinite(s_mat)))
  if quick_reject:
    d = np.diag(s_mat)
    with np.errstate(all='ignore'):
      m2 = s_mat * s_mat
      ref = np.abs(np.outer(d, d)) if top is None else top * top
      if not np.any(np.triu((m2 > FLOOR) & (m2 > (tol * tol) * ref), 1)):
        return j_mat, 0, 0
  total = sweeps = 0
  for _ in range(max_sweeps):
    nrot = 0
    for p, q in rounds:
      c, s, rot = rotations(s_mat[p, p], s_mat[q, q], s_mat[p, q], formula, tol, top)
      if not rot.any() and (skip_idle_rounds or finite):
        continue                     # (c = 1, s = 0 leave finite values as they are; jacobi_wave16 skips the round)
      nrot += int(rot.sum())
      with np.errstate(invalid='ignore'):
        xp, xq = s_mat[:, p].copy(), s_mat[:, q].copy()
        s_mat[:, p], s_mat[:, q] = c * xp - s * xq, s * xp + c * xq
        xp, xq = s_mat[p, :].copy(), s_mat[q, :].copy()
        s_mat[p, :], s_mat[q, :] = c[:, None] * xp - s[:, None] * xq, s[:, None] * xp + c[:, None] * xq
        xp, xq = j_mat[:, p].copy(), j_mat[:, q].copy()
        j_mat[:, p], j_mat[:, q] = c * xp - s * xq, s * xp + c * xq
    total += nrot
    sweeps += 1
    if nrot == 0:
      break
  return j_mat, total, sweeps


Eig = collections.namedtuple('Eig', 'vals vecs sweeps rotations')
WRONG_EIG = ('absolute', 'phantom', 'cross_fixed')


def jacobi_direct(a, formula='rcp', dtype=np.float64, tol=ROT_TOL, wrong=None, wave16=False):
  """The direct route (n <= NB) in `dtype`: jacobi64_kernel's direct mode, or the one-wave solver of the one launch.
  Reports 0 sweeps, as sym_eig does for this route.  wrong: 'absolute' (threshold relative to the largest diagonal
  entry), 'phantom' (an odd n's padding row holds 1e-3 max|a| and not zeros: the phantom player rotates)."""
  n = len(a)
  pl = players(n)
  s_mat = np.zeros((pl, pl), dtype)
  s_mat[:n, :n] = a
  if wrong == 'phantom' and pl > n:
    s_mat[n, :n] = s_mat[:n, n] = 1e-3 * np.max(np.abs(a))
  j_mat, total, _ = jacobi_lds(s_mat, direct_rounds(pl), MAX_OUTER_SWEEPS, formula, tol, wrong == 'absolute',
                               quick_reject=not wave16, skip_idle_rounds=wave16)
  return Eig(np.diag(s_mat)[:n].copy(), j_mat[:n, :n].copy(), 0, total)


def jacobi_block(a, wrong=None):
  """The block route (n > NB) in float64: per round every block pair's 64 x 64 sub-problem takes ONE inner sweep (the
  full ordering in round 0, the cross pairs after it), then A <- J^T A J and V <- V J; converged when a whole outer
  sweep rotates nothing.  wrong: 'cross_fixed' (see cross_rounds), 'absolute'."""
  n = len(a)
  pl = block_plan(n)
  big = np.zeros((pl.np, pl.np))
  big[:n, :n] = a
  v = np.eye(pl.np)
  full, cross = direct_rounds(NB), cross_rounds(wrong == 'cross_fixed')
  sweeps = total = 0
  while sweeps < MAX_OUTER_SWEEPS:
    rotated = 0
    for rnd, pairs, cross_only in pl.launches:
      subs = []
      for b in range(pairs):
        bp, bq = rr_pair(pl.nblocks, rnd, b)
        idx = np.concatenate((np.arange(bp * HB, bp * HB + HB), np.arange(bq * HB, bq * HB + HB)))
        j_mat, rot, _ = jacobi_lds(big[np.ix_(idx, idx)].copy(), cross if cross_only else full, MAX_INNER_SWEEPS,
                                   absolute=wrong == 'absolute')
        rotated += rot
        if rot:                      # (skip[pair]: an untouched pair's J is the identity)
          subs.append((idx, j_mat))
      for idx, j_mat in subs:
        big[:, idx] = big[:, idx] @ j_mat
        v[:, idx] = v[:, idx] @ j_mat
      for idx, j_mat in subs:
        big[idx, :] = j_mat.T @ big[idx, :]
    total += rotated
    sweeps += 1
    if rotated == 0:
      return Eig(np.diag(big)[:n].copy(), v[:n, :n].copy(), sweeps, total)
  return Eig(np.diag(big)[:n].copy(), v[:n, :n].copy(), sweeps + 1, total)


def sym_eig_model(a, wrong=None):
  """td_sym_eigh / sym_eig in float64: (vals unsorted, vecs as columns, the sweeps it reports, rotations)."""
  return jacobi_direct(a, wrong=wrong) if len(a) <= NB else jacobi_block(a, wrong)


def select(vals, dim, tie='lower', start=0):
  """The index of every wanted place in descending order, as the three selectors compute it: the rank of i counts the
  larger values and, of the equal ones, those of lower index ('lower'; 'higher' is the wrong rule j > i).  A place no
  index has keeps `start` (NaN values all rank 0); start = -1 is svd_extract_kernel before its fix."""
  vals = np.asarray(vals)
  idx = np.arange(len(vals))
  with np.errstate(invalid='ignore'):
    first = (idx[None, :] < idx[:, None]) if tie == 'lower' else (idx[None, :] > idx[:, None])
    rank = np.sum((vals[None, :] > vals[:, None]) | ((vals[None, :] == vals[:, None]) & first), axis=1)
  picks = []
  for want in range(dim):
    hit = np.nonzero(rank == want)[0]
    picks.append(int(hit[-1]) if len(hit) else start)
  return picks


Svd = collections.namedtuple('Svd', 'sig gn vn route sweeps')


def _triplets(g, vt, norms, picks):
  sig = np.array([norms[i] for i in picks])
  with np.errstate(all='ignore'):
    inv = np.where(sig > 0.0, 1.0 / sig, 0.0)
  return sig, np.array([g[i] * w for i, w in zip(picks, inv)]), np.array([vt[i] for i in picks])


def svd_rounds(g, dim, tie='lower', start=0):
  """The one-sided Jacobi of svd_small_kernel / svd_round_kernel / the one launch on the rows of g [k][m]:
  (sig, gn [dim][m], vn [dim][k], sweeps run)."""
  g = np.ascontiguousarray(g, np.float64)
  g, vt, sweeps = _orthogonalised(g.shape, g.tobytes())
  norms = np.sqrt(np.sum(g * g, axis=1))
  sig, gn, vn = _triplets(g, vt, norms, select(norms, dim, tie, start))
  return sig, gn, vn, sweeps


@functools.lru_cache(maxsize=4)
def _orthogonalised(shape, data):
  """(g after the rounds, the accumulated rotations vt, sweeps run) of the float64 matrix whose bytes are `data`.  The
  rounds do not depend on dim: one run serves the consecutive table rows of a shape (shared: not to be written)."""
  g = np.frombuffer(data, np.float64).reshape(shape).copy()
  k = len(g)
  kp = k + (k & 1)
  vt = np.eye(k)
  sweeps = 0
  while sweeps < MAX_OUTER_SWEEPS and k > 1:
    nrot = 0
    for rnd in range(kp - 1):
      for pair in range(kp // 2):
        i, j = rr_pair(kp, rnd, pair)
        if j >= k:
          continue                   # bye (odd k)
        al, be, ga = g[i] @ g[i], g[j] @ g[j], g[i] @ g[j]
        mag = abs(ga)
        if not (mag > FLOOR and mag > ROT_TOL * np.sqrt(al * be)):
          continue
        tau = (be - al) / (2.0 * ga)
        t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = t * c
        g[i], g[j] = c * g[i] - s * g[j], s * g[i] + c * g[j]
        vt[i], vt[j] = c * vt[i] - s * vt[j], s * vt[i] + c * vt[j]
        nrot += 1
    sweeps += 1
    if nrot == 0:
      break
  g.setflags(write=False)
  vt.setflags(write=False)
  return g, vt, sweeps


def _gram(g):
  gg = g @ g.T
  return np.triu(gg) + np.triu(gg, 1).T          # (gram_rows_kernel computes i <= j and mirrors it)


def svd_gram(g, dim, eig, cut, tie='lower', force=False):
  """The SVD through G = g g^T: None below the cut (the caller takes the rounds), else (sig, gn, vn)."""
  vals, vecs = eig(_gram(g))[:2]
  picks = select(vals, dim, tie)
  top, low = vals[picks[0]], vals[picks[dim - 1]]
  if not (force or (np.all(np.isfinite(vals)) and top > 0.0 and low > cut * top)):
    return None
  with np.errstate(all='ignore'):
    sig = np.array([np.sqrt(vals[i]) if vals[i] > 0.0 else 0.0 for i in picks])
    inv = np.where(sig > 0.0, 1.0 / sig, 0.0)
  vn = np.array([vecs[:, i] for i in picks])
  return sig, (vn @ g) * inv[:, None], vn


def svd_model(g, dim, tie='lower', start=0, wrong=None):
  """jacobi_svd on the rows of g [k][m].  sweeps: what it reports, 0 for the small and the Gram route.  wrong
  'gram_below_cut': the Gram route whatever its eigenvalues."""
  k, m = g.shape
  route = svd_route(k, m)
  if route == 'gram':
    out = svd_gram(g, dim, jacobi_direct, GRAM_CUT, tie, force=wrong == 'gram_below_cut')
    if out is not None:
      return Svd(out[0], out[1], out[2], 'gram', 0)
    route = 'rounds'
  sig, gn, vn, sweeps = svd_rounds(g, dim, tie, start)
  if route == 'small':
    return Svd(sig, gn, vn, 'small', 0)
  return Svd(sig, gn, vn, 'rounds', max(sweeps, 1) if k > 1 else 1)


def jacobi_svd_model(t, dim, tie='lower', wrong=None):
  """td_jacobi_svd on t [m][n]: (u [dim][m], s, v [dim][n], route, sweeps); the vectors of the narrower side are the
  ones orthogonalised."""
  cols = t.shape[1] <= t.shape[0]
  r = svd_model(np.ascontiguousarray(t.T) if cols else t, dim, tie, wrong=wrong)
  return (r.gn, r.sig, r.vn, r.route, r.sweeps) if cols else (r.vn, r.sig, r.gn, r.route, r.sweeps)


def fused_svd(g, dim, wrong=None):
  """The SVD inside cca_small_kernel: the Gram matrix through the one-wave solver when k > 1, m >= 4 k and the dim-th
  eigenvalue is above 1e-8 of the first, else the rounds.  wrong 'gram_below_cut': the Gram route regardless."""
  k, m = g.shape
  if k > 1 and m >= 4 * k:
    eig = lambda a: jacobi_direct(a, 'rs', wave16=True)
    out = svd_gram(g, dim, eig, GRAM_CUT_FUSED, force=wrong == 'gram_below_cut')
    if out is not None:
      return Svd(out[0], out[1], out[2], 'gram', 0)
  sig, gn, vn, _ = svd_rounds(g, dim)
  return Svd(sig, gn, vn, 'rounds', 0)


def _whiten_chol(c):
  return np.linalg.solve(np.linalg.cholesky(c), np.eye(len(c)))           # W = L^-1


def _whiten_eig(c, eps, eig, wrong=None):
  """The reference's symmetric K = W W^T, W = V f(lambda), f = lambda^-1/4 above eps, else 0 (wrong 'filter_ge': at
  or above)."""
  vals, vecs = eig(c)[:2]
  with np.errstate(all='ignore'):
    keep = vals >= eps if wrong == 'filter_ge' else vals > eps
    w = np.where(keep, vecs / np.sqrt(np.sqrt(vals)), 0.0)
    return w @ w.T, int(np.sum(~keep))


Dense = collections.namedtuple('Dense', 'rot_x rot_y e resolved svd_route dropped_y')
WRONG_DENSE = ('filter_ge', 'gram_below_cut')


def dense_model(cxx, cyy, cxy, dim, eps, route, wrong=None):
  """The dense stage in float64 along the route the case takes: the one launch, or the chain when the route or the
  launch's own verdict says so."""
  res = resolve(route, cxx, cyy, eps)
  if res.fused:
    eig_y = lambda a: jacobi_direct(a, 'rs', wave16=True)
    svd = lambda g: fused_svd(g, dim, wrong)
  else:
    eig_y = sym_eig_model
    svd = lambda g: svd_model(g, dim)
  wx = _whiten_chol(cxx) if res.route_x == 'cholesky' else _whiten_eig(cxx, eps, sym_eig_model)[0]
  dropped = 0
  if res.y_chol:
    wy = _whiten_chol(cyy)
  else:
    wy, dropped = _whiten_eig(cyy, eps, eig_y, wrong)
  with np.errstate(all='ignore'):
    t = wx @ cxy @ wy.T
    r = svd(np.ascontiguousarray(t.T) if route.cols else t)
    u_rows, v_rows = (r.gn, r.vn) if route.cols else (r.vn, r.gn)
    return Dense(wx.T @ u_rows.T, wy.T @ v_rows.T, r.sig, res, r.route, dropped)


# ---- td_sym_eigh: the table, the data, the measures -----------------------------------------------------------------
EIG_DIRECT = (1, 2, 3, 16, 17, 32, 33, 63, 64)
EIG_BLOCK = (65, 96, 127, 128, 129, 192, 193)
# kind -> smallest n at which it means something
EIG_KINDS = {'pd': 1, 'indefinite': 2, 'rank_deficient': 3, 'graded': 3, 'diagonal': 1, 'identity': 1, 'repeated': 3,
             'clusters': 4, 'pd_up': 1, 'pd_down': 1}
DIAGONAL_KINDS = ('diagonal', 'identity')
SCALED_KINDS = {'pd_up': 2.0 ** 80, 'pd_down': 2.0 ** -80}
EigCase = collections.namedtuple('EigCase', 'n kind')
EIG_CASES = [EigCase(n, kind) for n in EIG_DIRECT + EIG_BLOCK for kind, n_min in EIG_KINDS.items() if n >= n_min]


def eig_id(case):
  return '%s_%d' % (case.kind, case.n)


@functools.lru_cache(maxsize=None)
def eig_matrix(case):
  """The case's symmetric float64 matrix (shared: not to be written)."""
  n, kind = case
  rng = np.random.default_rng(7000 + n)
  if kind in ('pd', 'pd_up', 'pd_down'):
    b = rng.standard_normal((n, n + 3))
    a = (b @ b.T / n + 0.01 * np.eye(n)) * SCALED_KINDS.get(kind, 1.0)
  elif kind == 'indefinite':
    s = rng.standard_normal((n, n))
    a = (s + s.T) * 3.0
  elif kind == 'rank_deficient':
    low = rng.standard_normal((n, n // 2))
    a = low @ low.T
  elif kind == 'diagonal':
    a = np.diag(rng.standard_normal(n) * 3.0)
  elif kind == 'identity':
    a = np.eye(n)
  else:
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    if kind == 'graded':
      d = np.logspace(0, -6, n)
      a = d[:, None] * ((q * np.logspace(0, -6, n)) @ q.T) * d[None, :]
    elif kind == 'repeated':            # 2 I with one other entry, in another basis: n - 1 equal eigenvalues
      a = 2.0 * np.eye(n) + 3.0 * np.outer(q[:, 0], q[:, 0])
    else:                               # two clusters 1e-9 wide
      lam = np.where(np.arange(n) < n // 2, 1.0, 3.0) + 1e-9 * rng.standard_normal(n)
      a = (q * lam) @ q.T
  a = (a + a.T) / 2
  a.setflags(write=False)
  return a


EigMeasure = collections.namedtuple('EigMeasure', 'residual orthogonality spectrum')


def eig_measure(a, vals, vecs):
  """The three normwise quantities; the residual and V^T V are formed in np.longdouble."""
  n = len(a)
  al, vl, dl = (np.asarray(x, np.longdouble) for x in (a, vecs, vals))
  norm = float(np.sqrt(np.sum(al * al)))
  if not (np.all(np.isfinite(vals)) and np.all(np.isfinite(vecs))):
    return EigMeasure(np.inf, np.inf, np.inf)
  res = al @ vl - vl * dl
  orth = vl.T @ vl - np.eye(n)
  spec = np.sort(np.asarray(vals, np.float64)) - np.linalg.eigvalsh(a)
  return EigMeasure(float(np.sqrt(np.sum(res * res))) / norm, float(np.sqrt(np.sum(orth * orth))),
                    float(np.sqrt(np.sum(spec * spec))) / norm)


@functools.lru_cache(maxsize=None)
def eig_reference(case):
  """(LAPACK's measure, the model's measure, the model)."""
  a = eig_matrix(case)
  lam, v = np.linalg.eigh(a)
  model = sym_eig_model(a)
  return eig_measure(a, lam, v), eig_measure(a, model.vals, model.vecs), model


def eig_bounds(case):
  """8 max(lapack, model, n 2^-53) per quantity; the spectrum's LAPACK term is LAPACK's residual (Weyl)."""
  lap, mod, _ = eig_reference(case)
  floor = case.n * U64
  return EigMeasure(8.0 * max(lap.residual, mod.residual, floor), 8.0 * max(lap.orthogonality, mod.orthogonality, floor),
                    8.0 * max(lap.residual, mod.spectrum, floor))


@functools.lru_cache(maxsize=None)
def graded_reference(n):
  """The sorted eigenvalues of the graded matrix by the cyclic Jacobi in np.longdouble, threshold 1e-18."""
  a = np.asarray(eig_matrix(EigCase(n, 'graded')), np.longdouble)
  if n <= NB:
    return np.sort(jacobi_direct(a, dtype=np.longdouble, tol=LD_TOL).vals)
  pl = players(n)                        # (the reference of a block-route size is the same plain cyclic Jacobi)
  s_mat = np.zeros((pl, pl), np.longdouble)
  s_mat[:n, :n] = a
  jacobi_lds(s_mat, direct_rounds(pl), MAX_OUTER_SWEEPS, tol=LD_TOL)
  return np.sort(np.diag(s_mat)[:n])


def relative_error(vals, ref):
  vals = np.sort(np.asarray(vals, np.longdouble))
  with np.errstate(invalid='ignore'):
    err = np.abs(vals - ref) / ref
  return float(np.max(np.where(np.isfinite(err), err, np.inf)))


# ---- td_jacobi_svd: the table, the data, the measures ---------------------------------------------------------------
# (k vectors, length m); tall: t is [m][k] (n <= m, transposed on the device), else [k][m]
SVD_SHAPES = ((8, 865), (8, 866), (1, 6997), (1, 7001), (64, 255), (64, 256), (65, 300), (2, 9), (16, 64))
SvdCase = collections.namedtuple('SvdCase', 'k m dim kind tall')


def _svd_table():
  t = []
  for k, m in SVD_SHAPES:
    for dim in sorted({d for d in (1, 4, 5, k) if d <= k}):
      t.append(SvdCase(k, m, dim, 'graded', True))
    t.append(SvdCase(k, m, min(k, 4), 'graded', False))
    if k >= 4:
      for kind in ('tie', 'orthogonal', 'repeated_column'):
        t.append(SvdCase(k, m, k, kind, True))
      t.append(SvdCase(k, m, 4, 'tie', False))
      t.append(SvdCase(k, m, 1, 'orthogonal', False))
  for k, m in ((8, 866), (64, 256)):                # the shapes that form the Gram matrix
    for kind in ('cut_below', 'cut_above'):
      t.append(SvdCase(k, m, 5, kind, True))
  return t


SVD_CASES = _svd_table()
CUT_MARGIN = 100.0          # 'cut_below' / 'cut_above': lam[dim - 1] / lam[0] that far from GRAM_CUT


def svd_id(case):
  return '%s_k%d_m%d_dim%d_%s' % (case.kind, case.k, case.m, case.dim, 'tall' if case.tall else 'wide')


SvdData = collections.namedtuple('SvdData', 't null ties')


@functools.lru_cache(maxsize=None)
def svd_matrix(case):
  """t as td_jacobi_svd gets it, the places (in descending order) the table declares null, and the groups of tied
  places."""
  k, m, dim, kind, tall = case
  rng = np.random.default_rng(k * 100000 + m)
  null, ties = (), ()
  if kind == 'graded':
    g = rng.standard_normal((k, m)) * np.logspace(0, -6, k)[:, None]
  elif kind == 'orthogonal':
    # disjoint supports of m // k entries +-(1 + i): every dot product is exactly 0 and every squared norm exact in
    # any order of summation; vector 2 takes vector 1's size, so the two norms are equal to the bit
    g = np.zeros((k, m))
    for i in range(k):
      at = i + k * np.arange(m // k)
      g[i, at] = (2.0 if i == 2 else 1.0 + i) * np.where(rng.standard_normal(len(at)) < 0, -1.0, 1.0)
    order = sorted(range(k), key=lambda i: (-(g[i] @ g[i]), i))
    ties = (tuple(sorted((order.index(1), order.index(2)))),)
  elif kind == 'repeated_column':
    g = rng.standard_normal((k, m)) * np.logspace(0, -2, k)[:, None]
    g[-1] = g[0]
    null = (k - 1,)
  else:
    u, _ = np.linalg.qr(rng.standard_normal((m, k)))
    v, _ = np.linalg.qr(rng.standard_normal((k, k)))
    if kind == 'tie':
      s = np.logspace(0, -3, k)
      s[2] = s[1]
      ties = ((1, 2),)
    else:                             # s[dim - 1]^2 / s[0]^2 = GRAM_CUT / or x CUT_MARGIN
      ratio = np.sqrt(GRAM_CUT / CUT_MARGIN if kind == 'cut_below' else GRAM_CUT * CUT_MARGIN)
      s = np.concatenate((np.geomspace(1.0, ratio, dim), ratio * np.geomspace(0.5, 0.1, k - dim)))
    g = (v * s) @ u.T
  t = np.ascontiguousarray(g.T) if tall else np.ascontiguousarray(g)
  t.setflags(write=False)
  return SvdData(t, null, ties)


SvdMeasure = collections.namedtuple('SvdMeasure', 's_rel s_null vec triplet tie')


def svd_gaps(ss, dim):
  """g_i: the smallest distance of s_i to another singular value, relative to s_1."""
  out = []
  for i in range(dim):
    others = np.delete(ss, i)
    out.append(float(np.min(np.abs(others - ss[i])) / ss[0]) if len(others) else 1.0)
  return np.array(out)


def svd_measure(data, dim, u, s, v):
  """s_rel: max |s - s_ref| / s_ref off the null places; s_null: max |s - s_ref| / s_1 on them; vec [dim]: the larger
  of |1 - |u_i . u_ref|| and |1 - sign v_i . v_ref| (0 on null and tied places); triplet: ||T v^T - u^T s||_F / ||T||_F;
  tie: ||P - P_ref||_F of the projectors on the tied vectors' span, the largest over the groups inside dim."""
  t = data.t
  uu, ss, vvt = np.linalg.svd(t, full_matrices=False)
  if not all(np.all(np.isfinite(x)) for x in (u, s, v)):
    return SvdMeasure(np.inf, np.inf, np.full(dim, np.inf), np.inf, np.inf)
  null = [i for i in data.null if i < dim]
  live = [i for i in range(dim) if i not in null]
  tied = {i for grp in data.ties for i in grp}
  s_rel = max([abs(s[i] - ss[i]) / ss[i] for i in live] or [0.0])
  s_null = max([abs(s[i] - ss[i]) / ss[0] for i in null] or [0.0])
  vec = np.zeros(dim)
  for i in live:
    if i in tied:
      continue
    du = u[i] @ uu[:, i]
    vec[i] = max(abs(abs(du) - 1.0), abs(np.sign(du) * (v[i] @ vvt[i]) - 1.0))
  tl, ul, vl, sl = (np.asarray(x, np.longdouble) for x in (t, u, v, s))
  res = tl @ vl.T - ul.T * sl
  triplet = float(np.sqrt(np.sum(res * res)) / np.sqrt(np.sum(tl * tl)))
  tie = 0.0
  for grp in data.ties:
    if max(grp) < dim:
      grp = list(grp)
      for got, ref in ((u[grp], uu[:, grp].T), (v[grp], vvt[grp])):
        tie = max(tie, float(np.linalg.norm(got.T @ got - ref.T @ ref)))
  return SvdMeasure(float(s_rel), float(s_null), vec, triplet, tie)


@functools.lru_cache(maxsize=None)
def svd_reference(case):
  """(the model's measure, LAPACK's triplet residual, the gaps g_i, the model's route, its sweeps)."""
  data = svd_matrix(case)
  u, s, v, route, sweeps = jacobi_svd_model(data.t, case.dim)
  uu, ss, vvt = np.linalg.svd(data.t, full_matrices=False)
  lap = svd_measure(data, case.dim, uu[:, :case.dim].T, ss[:case.dim], vvt[:case.dim])
  gaps = svd_gaps(ss, case.dim)
  for grp in data.ties:                # a tied group's gap is its distance to the rest
    rest = np.delete(ss, list(grp))
    for i in grp:
      if i < case.dim:
        gaps[i] = float(np.min(np.abs(rest - ss[i])) / ss[0])
  return svd_measure(data, case.dim, u, s, v), lap.triplet, gaps, route, sweeps


def svd_bounds(case):
  """SvdMeasure of bounds."""
  mod, lap_triplet, gaps, _, _ = svd_reference(case)
  size = max(case.k, case.m) * U64
  s_tol = 8.0 * max(mod.s_rel, size)
  gap_term = 64.0 * (case.k + case.m) * U64 / gaps
  tied = [i for grp in svd_matrix(case).ties for i in grp if i < case.dim]
  return SvdMeasure(s_tol, 8.0 * max(mod.s_null, size), gap_term, 8.0 * max(mod.triplet, lap_triplet, size),
                    float(np.max(gap_term[tied])) if tied else 0.0)


# ---- td_cca_solve: the table, the data, the reference ---------------------------------------------------------------
# kind: None | 'copy' (input_2's last channel repeats its first) | 'zero' (its last channel is 0) | 'indefinite'
# (denom = 2 frames - 1 and a large mean: the covariance of input_1 is indefinite) | 'uncorrelated' (input_2's last
# channel is orthogonal to input_1 and to the ones up to its float32 rounding: a canonical correlation of about 1e-8,
# small but not null -- the one launch's Gram matrix would lose it, and every component is compared)
CcaCase = collections.namedtuple('CcaCase', 'name c1 l1 c2 l2 dim reg kind whitening seed')
FUSED_SHAPES = ((1, 1), (2, 1), (2, 2), (8, 2), (7, 2), (16, 16), (17, 16), (27, 7), (28, 7), (63, 15), (64, 16))
# {name: seed} where seed 0 does not give every compared component g >= 2 G_MIN on the CPU sums (the first seed that
# does, counting from 0); as the tables stand seed 0 does everywhere, and tests/test_cpu_eig_edges.py asserts it
SEEDS = {}


def _cca_case(name, k1, k2, dim, reg, kind=None, whitening=0, lags=(1, 1)):
  l1, l2 = lags
  assert k1 % l1 == 0 and k2 % l2 == 0
  return CcaCase(name, k1 // l1, l1, k2 // l2, l2, dim, float(reg), kind, whitening, SEEDS.get(name, 0))


def _cca_table():
  fused, chain = [], []
  dims = (1, 4, 5)
  for n, (k1, k2) in enumerate(FUSED_SHAPES):
    tag = '%dx%d' % (k1, k2)
    fused.append(_cca_case('reg_' + tag, k1, k2, k2, 0.1))
    fused.append(_cca_case('noreg_' + tag, k1, k2, min(k2, dims[n % 3]), 0.0))
    if k2 > 1:
      fused.append(_cca_case('copy_' + tag, k1, k2, k2, 0.0, 'copy'))
      fused.append(_cca_case('zero_' + tag, k1, k2, k2, 0.0, 'zero'))
      fused.append(_cca_case('zero_reg_' + tag, k1, k2, k2, 0.1, 'zero'))
  for dim in (1, 4, 5, 16):            # 8 channels x 8 lags against 2 x 8 lags: the moments arrive expanded
    fused.append(_cca_case('lagged_64x16_dim%d' % dim, 64, 16, dim, 0.1, lags=(8, 8)))
  fused.append(_cca_case('copy_63x15_dim5', 63, 15, 5, 0.0, 'copy'))
  for k1, k2 in ((28, 7), (64, 16)):
    fused.append(_cca_case('uncorrelated_%dx%d' % (k1, k2), k1, k2, k2, 0.1, 'uncorrelated'))
  fused.append(_cca_case('indefinite_12x4', 12, 4, 3, 0.1, 'indefinite'))
  for k2, dim in ((16, 16), (17, 17), (64, 5), (65, 5)):
    chain.append(_cca_case('chain_70x%d' % k2, 70, k2, dim, 0.1))
  for k1 in (64, 65):
    chain.append(_cca_case('chain_%dx17' % k1, k1, 17, 1, 0.1))
  chain.append(_cca_case('chain_12x20', 12, 20, 12, 0.1))
  chain.append(_cca_case('chain_5x70', 5, 70, 5, 0.05))
  chain.append(_cca_case('chain_noreg_70x17', 70, 17, 5, 0.0))
  chain.append(_cca_case('chain_copy_70x20', 70, 20, 5, 0.0, 'copy'))
  chain.append(_cca_case('chain_copy_70x70', 70, 70, 5, 0.0, 'copy'))
  chain.append(_cca_case('chain_eigen_70x16', 70, 16, 5, 0.1, whitening=1))
  chain.append(_cca_case('chain_eigen_12x20', 12, 20, 1, 0.1, whitening=1))
  return fused, chain


FUSED_CASES, CHAIN_CASES = _cca_table()
CCA_CASES = FUSED_CASES + CHAIN_CASES


def cca_id(case):
  return case.name


def cca_k(case):
  return case.c1 * case.l1, case.c2 * case.l2


def cca_rows(case):
  k1, k2 = cca_k(case)
  return max(200, 4 * (k1 + k2))


def cca_lags(case):
  return 0, case.l1 - 1, case.l2 // 2, case.l2 - 1 - case.l2 // 2


def cca_options(case, fused=True):
  return {'cca_whitening': case.whitening, 'cca_fused': 1 if fused else 0}


def cca_data(case):
  """(x [n, c1], x2 [n, c2]) float32, the sources of cca_sweep_edges.make_parts: input_2's channel j is source j at a
  graded signal-to-noise ratio, input_1 a mixture of the sources plus noise, both with an offset (a smaller one under a
  deficient input_2: the rounding of S / denom - m^T m is what its zero eigenvalue comes out as)."""
  rng = np.random.default_rng(3000 + case.seed)
  n, r = cca_rows(case), case.c2
  grade = np.linspace(0.95, 0.3, r) if r > 1 else np.array([0.8])
  mix = rng.standard_normal((r, case.c1)) / np.sqrt(r)
  s = rng.standard_normal((n, r))
  x = (s @ mix + 0.5 * rng.standard_normal((n, case.c1)) + 1.0).astype(np.float32)
  offset_2 = -0.25 if case.kind in ('copy', 'zero') else -2.0
  x2 = (grade * s + np.sqrt(1.0 - grade ** 2) * rng.standard_normal((n, r)) + offset_2).astype(np.float32)
  if case.kind == 'copy':
    x2[:, -1] = x2[:, 0]
  if case.kind == 'zero':
    x2[:, -1] = 0.0
  if case.kind == 'indefinite':
    x[:, :2] += 4.0
  if case.kind == 'uncorrelated':
    basis = np.column_stack((np.ones(n), x.astype(np.float64)))
    z = rng.standard_normal(n)
    x2[:, -1] = (z - basis @ np.linalg.lstsq(basis, z, rcond=None)[0]).astype(np.float32)
  return x, x2


def cca_denom(case, frames):
  return 2 * frames - 1 if case.kind == 'indefinite' else frames - 1


@functools.lru_cache(maxsize=None)
def cca_cpu_moments(case):
  """cca_sweep_edges.Mom from the float64 sums of the materialised lag matrices."""
  from tests import host_cca_sweep as hc
  pre1, post1, pre2, post2 = cca_lags(case)
  x, x2 = cca_data(case)
  st = hc.LagStats(case.c1, pre1, post1, case.c2, pre2, post2, handle=object())
  st.accumulate(x, x2, None, [0, len(x)])
  return cs.Mom(st.sxx.copy(), st.syy.copy(), st.sxy.copy(), st.sx.copy(), st.sy.copy(), st.frames)


def covariances(mom, denom, reg):
  """(cxx, cyy, cxy, mean_x, mean_y) as cov_kernel and the one launch form them."""
  inv_d, inv_f = 1.0 / denom, 1.0 / mom.frames
  mx, my = mom.sx * inv_f, mom.sy * inv_f
  return (mom.sxx * inv_d - np.outer(mx, mx) + reg * np.eye(len(mx)),
          mom.syy * inv_d - np.outer(my, my) + reg * np.eye(len(my)), mom.sxy * inv_d - np.outer(mx, my), mx, my)


NULL_RATIO = 1e-6           # a component may be left out of the rotation comparison below this of e_1
CcaRef = collections.namedtuple('CcaRef', 'pair compared mean_x mean_y resolved svd_route dropped_y cov model k1 k2')


def cca_reference(case, mom, fused=True, eps=EPS_EIG, wrong=None):
  """R1, the model R2 of the route taken, D and g for one solve.  pair: a cca_sweep_edges.Pair over the COMPARED
  components (rot_x, rot_y, d_x, d_y) and over all of them (e, d_e).  compared: every component, but for the one whose
  reference singular value a deficient input_2 brings below NULL_RATIO e_1."""
  k1, k2 = len(mom.sx), len(mom.sy)
  denom = cca_denom(case, mom.frames)
  cxx, cyy, cxy, mx, my = covariances(mom, denom, case.reg)
  route = cca_route(k1, k2, case.reg, eps, denom, mom.frames, cca_options(case, fused))
  rx, ry, e, every = cs.route_r1(cxx, cyy, cxy, case.dim, eps)
  model = dense_model(cxx, cyy, cxy, case.dim, eps, route, wrong)
  compared = np.ones(case.dim, bool)
  if case.kind in ('copy', 'zero'):
    compared = ~(e < NULL_RATIO * e[0])
  with np.errstate(invalid='ignore'):
    sign = cs._align(model.rot_x, model.rot_y, rx, ry)
    d_e = float(np.max(np.abs(model.e - e))) if np.all(np.isfinite(model.e)) else np.inf
    d_x = np.max(np.abs(model.rot_x * sign - rx), axis=0) / np.max(np.abs(rx), axis=0)
    d_y = np.max(np.abs(model.rot_y * sign - ry), axis=0) / np.max(np.abs(ry), axis=0)
  lead = every[:int(np.sum(compared)) + 1]
  g = float(np.min(lead[:-1] - lead[1:]) / every[0]) if len(lead) > 1 else 1.0
  c = compared
  pair = cs.Pair(None, rx[:, c], ry[:, c], e, d_e, d_x[c], d_y[c], g)
  return CcaRef(pair, compared, mx.astype(np.float32), my.astype(np.float32), model.resolved, model.svd_route,
                model.dropped_y, (cxx, cyy, cxy), model, k1, k2)


def model_outputs(ref):
  """The model's (rot_x, rot_y, mean_x, mean_y, e) rounded to float32, as the device returns them."""
  with np.errstate(all='ignore'):
    return (ref.model.rot_x.astype(np.float32), ref.model.rot_y.astype(np.float32), ref.mean_x[None, :],
            ref.mean_y[None, :], ref.model.e.astype(np.float32))


CcaReport = collections.namedtuple('CcaReport', 'means_ok err_e ratio_e bound_e err_rot ratio_rot bound_rot invariants '
                                               'd_e d_rot g failures')
INVARIANT_TOL = 2e-6        # tests/test_gpu_online_cca_fit.py: |Rx^T Cxx Rx - I|, |Rx^T Cxy Ry - diag(e)| <= 2e-6


def cca_check(out, ref):
  """(rot_x [k1, dim], rot_y, mean_x [1, k1], mean_y, e [dim]) float32 against the reference."""
  rot_x, rot_y, mean_x, mean_y, e = (np.asarray(a) for a in out)
  p, c = ref.pair, ref.compared
  fails = []
  means_ok = np.array_equal(mean_x.ravel(), ref.mean_x) and np.array_equal(mean_y.ravel(), ref.mean_y)
  if not means_ok:
    fails.append('means differ')
  gx, gy, ge = rot_x.astype(np.float64)[:, c], rot_y.astype(np.float64)[:, c], e.astype(np.float64)
  be, bx, by = cs.pair_bounds(p, ref.k1, ref.k2)
  sign = cs._align(gx, gy, p.rot_x, p.rot_y)
  with np.errstate(invalid='ignore'):
    de, dx, dy = np.abs(ge - p.e), np.abs(gx * sign - p.rot_x), np.abs(gy * sign - p.rot_y)
    de, dx, dy = (np.where(np.isfinite(a), a, np.inf) for a in (de, dx, dy))
  sx, sy = np.max(np.abs(p.rot_x), axis=0), np.max(np.abs(p.rot_y), axis=0)
  err_rot = max((dx / sx).max(), (dy / sy).max())
  ratio_rot = max((dx / bx).max(), (dy / by).max())
  bound_rot = min((bx / sx).max(axis=0).min(), (by / sy).max(axis=0).min())
  if (de / be).max() > 1.0 or ratio_rot > 1.0:
    fails.append('e %.3g x bound, rotations %.3g x' % ((de / be).max(), ratio_rot))
  cxx, _, cxy = ref.cov
  with np.errstate(invalid='ignore'):
    inv = max(np.max(np.abs(gx.T @ cxx @ gx - np.eye(gx.shape[1]))),
              np.max(np.abs(gx.T @ cxy @ gy - np.diag(ge[c]))))
  inv = float(inv) if np.isfinite(inv) else np.inf
  if not inv <= INVARIANT_TOL:
    fails.append('invariants off by %.3g' % inv)
  return CcaReport(means_ok, float(de.max()), float((de / be).max()), float(be.min()), float(err_rot), float(ratio_rot),
                   float(bound_rot), inv, p.d_e, float(max(p.d_x.max(), p.d_y.max())), p.g, fails)


def eig_margin(c, eps=EPS_EIG):
  """(smallest eigenvalue, whether no eigenvalue lies in (eps / 100, 100 eps))."""
  lam = np.linalg.eigvalsh(c)
  return float(lam[0]), not np.any((lam > eps / 100.0) & (lam < 100.0 * eps))


# ---- a NaN in one channel of input_1 --------------------------------------------------------------------------------
def nan_svd_outputs(k, m, dim, start=0):
  """What jacobi_svd returns for vectors that are all NaN (a NaN channel makes every entry of T one: each is a sum over
  that channel's rows of cov_xy): (sig, the picks of the selector).  Every route ends in the rounds -- the Gram
  matrix's eigenvalues are not finite -- where no pair rotates and every norm ranks 0."""
  g = np.full((k, m), np.nan)
  r = svd_model(g, dim, start=start)
  norms = np.full(k, np.nan)
  return r, select(norms, dim, start=start)
