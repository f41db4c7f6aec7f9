"""The edge cases of the CCA sweep's device call (td_cca_solve_loso_terms, csrc/cca_sweep.hip over the batched
Cholesky of csrc/chol.hip; tests/test_gpu_cca_sweep_edges.py, tests/test_cpu_cca_sweep_edges.py): the case table, the
data builder, the float64 reference with its derived bound, a restatement of the host arithmetic that picks a route,
the device's three status rules, and numpy models of a wrong kernel.  A plain module, not a conftest.

The reference isolates the call.  Its inputs are plain float64 arrays -- the dense moments of the total and of every
distinct term (on the GPU the device's own, LagStats.moments(want_cca=True); on the CPU the sums of
tests/host_cca_sweep.LagStats), the folds' signed terms, the lambdas, dim and eps_eig -- from which it forms, as the
header of cca_sweep.hip states them,
  C_xx = S_xx / (frames - 1) - m_x^T m_x + lambda I,  C_yy likewise,  C_xy = S_xy / (frames - 1) - m_x^T m_y,
  m = sum * (1.0 / frames),  a fold's sums = the total's plus its signed terms in the fold's order,
and solves every (fold, lambda) pair along two float64 routes:
  R1  the reference project's: two eigh whitenings (eigenvalues <= eps_eig dropped) and an svd;
  R2  the kernel's algebra: C_xx = L L^T, W = L^-1 C_xy, K = C_yy^-1/2, B = K W^T W K = V sigma^2 V^T,
      rot_y = K V, rot_x = L^-T W rot_y / sigma.
R1 is what the GPU is held to.  D = |R1 - R2| is the reference's own uncertainty: D_e the largest over the pair's
components, D_rot per rotation column relative to that column's largest entry, after aligning the joint sign of
(rot_x, rot_y) per component.

The bound, elementwise:
  e          |gpu - ref| <= 2^-24 |ref| + 8 D_e + 64 (K1 + K2) 2^-53
  rotations  |gpu - ref| <= 2^-24 |ref| + (8 D_rot + 64 (K1 + K2) 2^-53 / g) max|ref column|
2^-24 |ref| is the float32 rounding of the output; the 8 on D covers a third summation order; the last term is the
float64 eigenvector sensitivity, g the smallest gap among the first dim + 1 reference singular values relative to
sigma_1.  Every table case has g >= 1e-3 (the seeds are chosen for it; the CPU test asserts it).
mean_x / mean_y are held bit for bit to np.float32(s * (1.0 / frames)); the biases to the float32 rounding of
-mean . rot within 1e-6 sum |mean . rot| (the rule of tests/test_gpu_cca_sweep.py)."""
import collections
import functools

import numpy as np

EPS_EIG = 1e-12
G_MIN = 1e-3
U32 = 2.0 ** -24
U64 = 2.0 ** -53

# ---- the route arithmetic of td_cca_solve_loso_terms and chol_factor_forward, restated -------------------------------
NB = 64
CHUNK_BYTES = 3 << 29          # kChunkBytes
CHUNK_SYSTEMS = 160            # kChunkSystems
MAX_COLUMNS = 4096             # n_lambda * dim


def _round_up(v, m):
  return -(-v // m) * m


Plan = collections.namedtuple('Plan', 'np nblk rt_rows ut_rows by_bytes by_count chunk clamped chunks batches '
                                      'backward_trips')
Factor = collections.namedtuple('Factor', 'ow panel_tiles by_xcd grid_systems phantom updates')


def plan(k1, k2, dim, n_folds, n_lambda):
  """What the host code of td_cca_solve_loso_terms derives from the sizes.  chunks: [(fold0, folds)]; batches: systems
  per batched factorisation; backward_trips: calls of td_chol_batch_backward (= trips of step 7 of the tail)."""
  np_ = _round_up(k1, NB)
  nblk = np_ // NB
  rt_rows, ut_rows = _round_up(k2, 8), _round_up(dim, 8)
  per_sys = 8 * (np_ * np_ + (rt_rows + 2 * ut_rows) * np_ + nblk * NB * NB)
  by_bytes, by_count = CHUNK_BYTES // (per_sys * n_lambda), CHUNK_SYSTEMS // n_lambda
  chunk = min(n_folds, by_bytes, by_count)
  clamped = chunk < 1
  chunk = max(chunk, 1)
  chunks = tuple((f0, min(chunk, n_folds - f0)) for f0 in range(0, n_folds, chunk))
  return Plan(np_, nblk, rt_rows, ut_rows, by_bytes, by_count, chunk, clamped, chunks,
              tuple(nf * n_lambda for _, nf in chunks), ut_rows // 8)


def factor_plan(nblk, batch):
  """chol_factor_forward: block columns per outer block, row tiles per panel workgroup, the XCD-aware system order of
  the update grid (batch >= 8: the grid covers a multiple of 8 systems, the phantom ones return at once), and how many
  update launches there are (none for a single block)."""
  ow = 1 if batch <= 2 else 4
  by_xcd = batch >= 8
  grid = _round_up(batch, 8) if by_xcd else batch
  updates = 0
  for kb in range(0, nblk, ow):
    cols = min(ow, nblk - kb)
    updates += cols - 1 + (1 if kb + ow < nblk else 0)
  return Factor(ow, 1 if batch <= 2 else 3, by_xcd, grid, grid - batch, updates)


# ---- the table ------------------------------------------------------------------------------------------------------
# parts: rows of every recording; the total sums the first n_total of them; folds: per fold ((part, sign), ...) in the
# order the call gets them; kind: None | 'dup_x' | 'dup_x2' | 'nan'; expect: plan fields the case is named for
Case = collections.namedtuple('Case', 'name c1 l1 c2 l2 dim lambdas parts n_total folds batch_size seed kind expect')

# lagged width -> (channels, lags)
X_SHAPES = {1: (1, 1), 2: (2, 1), 5: (5, 1), 12: (4, 3), 63: (21, 3), 64: (8, 8), 65: (13, 5), 70: (14, 5),
            127: (127, 1), 128: (16, 8), 129: (43, 3), 192: (24, 8), 193: (193, 1)}
X2_SHAPES = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (4, 1), 7: (7, 1), 8: (2, 4), 9: (3, 3), 12: (4, 3), 15: (5, 3),
             16: (2, 8), 17: (1, 17), 20: (20, 1), 33: (3, 11), 63: (3, 21), 64: (2, 32)}

TWO_FOLDS = ((), ((1, -1.0),))          # the total itself; the total minus the second recording
# the seeds at which every pair of the case has g >= 2 G_MIN on the CPU sums (the first such seed counting from 0)
SEEDS = {'k2_33': 4, 'k2_63': 12, 'k2_64': 1}


def _case(name, k1, k2, dim, lambdas, parts=(260, 170), n_total=None, folds=TWO_FOLDS, batch_size=1, kind=None,
          **expect):
  (c1, l1), (c2, l2) = X_SHAPES[k1], X2_SHAPES[k2]
  return Case(name, c1, l1, c2, l2, dim, tuple(float(v) for v in lambdas), tuple(parts),
              len(parts) if n_total is None else n_total, tuple(tuple(f) for f in folds), batch_size,
              SEEDS.get(name, 0), kind, tuple(sorted(expect.items())))


def _held_out(n):
  return tuple(((i, -1.0),) for i in range(n))


def _table():
  t = []
  for k1 in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193):
    t.append(_case('k1_%d' % k1, k1, 3, min(3, k1), (1e-3, 1.0), nblk=-(-k1 // 64)))
  for k2 in (1, 2, 7, 8, 9, 15, 16, 17, 33, 63, 64):
    t.append(_case('k2_%d' % k2, 70, k2, min(5, k2), (1e-3, 1.0), rt_rows=_round_up(k2, 8)))
  t.append(_case('k1_below_k2', 5, 12, 5, (1e-3, 1.0), rt_rows=16))
  for dim in (1, 7, 8, 9, 16, 17, 20):
    t.append(_case('dim_%d' % dim, 70, 20, dim, (1e-3, 1.0), ut_rows=_round_up(dim, 8), backward_trips=-(-dim // 8)))
  # the factorisation's batch routes at nblk = 3: 17 recordings, every fold holds out another one
  parts17 = tuple(40 + (i * 7) % 11 for i in range(17))
  for n_f, lams in ((1, (0.1,)), (2, (0.1,)), (3, (0.1,)), (7, (0.1,)), (4, (1e-2, 1.0)), (9, (0.1,)), (17, (0.1,))):
    t.append(_case('batch_%d' % (n_f * len(lams)), 129, 4, 3, lams, parts17, folds=_held_out(n_f), nblk=3,
                   batches=(n_f * len(lams),)))
  parts9 = tuple(60 + 5 * i for i in range(9))
  t.append(_case('chunks_8_1', 5, 2, 2, np.geomspace(1e-3, 10.0, 20), parts9, folds=_held_out(9), chunk=8,
                 clamped=False, chunks=((0, 8), (8, 1))))
  t.append(_case('chunk_clamp', 5, 2, 1, np.geomspace(1e-3, 10.0, 161), (150, 110), folds=_held_out(2), chunk=1,
                 clamped=True, chunks=((0, 1), (1, 1))))
  # folds of 0 .. 4 terms with mixed signs; recording 3 serves three folds, recording 4 (outside the total) two;
  # the last fold takes recording 2 with + and - and so equals the total; minibatches of 10 frames
  t.append(_case('terms', 12, 4, 3, (1e-3, 1.0), (120, 90, 100, 80, 60), n_total=4, batch_size=10, folds=(
      (), ((1, -1.0),), ((2, -1.0), (3, -1.0)), ((0, -1.0), (3, -1.0), (4, 1.0)),
      ((1, -1.0), (2, -1.0), (4, 1.0), (3, -1.0)), ((2, 1.0), (2, -1.0)))))
  t.append(_case('status_dup_x', 65, 3, 3, (0.0, 0.1), kind='dup_x', status=((1, 0), (1, 0)), rules=(1, 0)))
  t.append(_case('status_dup_x2_full_dim', 12, 4, 4, (0.0, 0.1), kind='dup_x2', status=((1, 1), (1, 1)), rules=(2, 3)))
  t.append(_case('status_dup_x2', 12, 4, 3, (0.0, 0.1), kind='dup_x2', status=((1, 0), (1, 0)), rules=(2, 0)))
  return t


CASES = _table()
STATUS_CASES = [c for c in CASES if c.kind is not None]
PLAIN_CASES = [c for c in CASES if c.kind is None]
# a NaN in one EEG channel of recording 2, which only the last fold adds: that fold's pairs report 1, the others are right
NAN_CASE = _case('nan_term', 12, 4, 3, (1e-3, 1.0), (120, 90, 70), n_total=2, folds=((), ((1, -1.0),), ((2, 1.0),)),
                 kind='nan')


def case_id(case):
  return case.name


def case_k(case):
  return case.c1 * case.l1, case.c2 * case.l2


def fold_frames(case):
  """Frames of every fold."""
  n = sum(case.parts[:case.n_total])
  return [n + sum(int(sg) * case.parts[p] for p, sg in fold) for fold in case.folds]


def fold_batches(case):
  frames = fold_frames(case)
  assert all(f % case.batch_size == 0 for f in frames)
  return [f // case.batch_size for f in frames]


def lags(case):
  """(pre1, post1, pre2, post2)"""
  return 0, case.l1 - 1, case.l2 // 2, case.l2 - 1 - case.l2 // 2


# ---- data -----------------------------------------------------------------------------------------------------------
def make_parts(case):
  """[(x [n, c1], x2 [n, c2])] float32: c2 latent sources; input_2's channel j is source j at a graded signal-to-noise
  ratio (the canonical correlations come out spread, not clustered), input_1 a random mixture of the sources plus
  noise; both with an offset, so that the means matter (a smaller one under a duplicated input_2 column: the rounding
  of S / denom - m^T m is what the zero eigenvalue of C_yy comes out as, and it has to stay 1e3 below eps_eig)."""
  rng = np.random.default_rng(1000 + case.seed)
  r = case.c2
  grade = np.linspace(0.95, 0.3, r) if r > 1 else np.array([0.8])
  mix = rng.standard_normal((r, case.c1)) / np.sqrt(r)
  offset_2 = -0.25 if case.kind == 'dup_x2' else -2.0
  out = []
  for i, n in enumerate(case.parts):
    s = rng.standard_normal((n, r))
    x = (s @ mix + 0.5 * rng.standard_normal((n, case.c1)) + 1.0).astype(np.float32)
    x2 = (grade * s + np.sqrt(1.0 - grade ** 2) * rng.standard_normal((n, r)) + offset_2).astype(np.float32)
    if case.kind == 'dup_x':
      x[:, 1] = x[:, 0]
    if case.kind == 'dup_x2':
      x2[:, -1] = x2[:, -2]
    if case.kind == 'nan' and i == 2:
      x[7, 1] = np.nan
    out.append((x, x2))
  return out


Mom = collections.namedtuple('Mom', 'sxx syy sxy sx sy frames')


def cpu_moments(case):
  """[Mom] of the total and of every recording, from the float64 sums of the materialised lag matrices
  (tests/host_cca_sweep.LagStats): (total, [part 0, part 1, ...])."""
  return _cpu_moments(case)


@functools.lru_cache(maxsize=None)
def _cpu_moments(case):
  from tests import host_cca_sweep as hc
  pre1, post1, pre2, post2 = lags(case)
  stats = []
  for x, x2 in make_parts(case):
    st = hc.LagStats(case.c1, pre1, post1, case.c2, pre2, post2, handle=object())
    st.accumulate(x, x2, None, [0, len(x)])
    stats.append(st)
  total = hc.LagStats(case.c1, pre1, post1, case.c2, pre2, post2, handle=object()).combine(stats[:case.n_total])
  mom = lambda st: Mom(st.sxx.copy(), st.syy.copy(), st.sxy.copy(), st.sx.copy(), st.sy.copy(), st.frames)
  return mom(total), [mom(st) for st in stats]


def device_moments(st):
  """Mom of a device.LagStats from its own float64 moments."""
  m = st.moments(want_xtx=True, want_xty=False, want_cca=True)
  k1 = st.k1
  xtx = m['xtx'].cpu().numpy()
  return Mom(xtx[:k1, :k1].copy(), m['x2tx2'].cpu().numpy(), m['xtx2'].cpu().numpy(), xtx[k1, :k1].copy(),
             m['sum_x2'].cpu().numpy(), st.counts()[0])


# ---- the reference --------------------------------------------------------------------------------------------------
def fold_sums(total, parts, fold, flip=None):
  """The fold's sums: the total's plus the signed terms in the fold's order (flip: the term whose sign a wrong kernel
  reverses; the frames stay the host's)."""
  s = [np.array(a, np.float64) for a in total[:5]]
  frames = total.frames
  for t, (p, sign) in enumerate(fold):
    sg = -sign if t == flip else sign
    for a, b in zip(s, parts[p][:5]):
      a += sg * b
    frames += int(sign) * parts[p].frames
  return Mom(s[0], s[1], s[2], s[3], s[4], frames)


def covariances(s, lam):
  inv_frames, inv_denom = 1.0 / s.frames, 1.0 / (s.frames - 1)
  mx, my = s.sx * inv_frames, s.sy * inv_frames
  cxx = s.sxx * inv_denom - np.outer(mx, mx) + lam * np.eye(len(mx))
  cyy = s.syy * inv_denom - np.outer(my, my) + lam * np.eye(len(my))
  cxy = s.sxy * inv_denom - np.outer(mx, my)
  return cxx, cyy, cxy, mx, my


def route_r1(cxx, cyy, cxy, dim, eps=EPS_EIG):
  """(rot_x, rot_y, e, every singular value) the reference project's way."""
  def inv_sqrt(c):
    vals, vecs = np.linalg.eigh(c)
    keep = vals > eps
    return (vecs[:, keep] / np.sqrt(vals[keep])) @ vecs[:, keep].T
  k11, k22 = inv_sqrt(cxx), inv_sqrt(cyy)
  u, e, vt = np.linalg.svd(k11 @ cxy @ k22, full_matrices=False)
  return k11 @ u[:, :dim], k22 @ vt.T[:, :dim], e[:dim], e


def _inv_sqrt_full(cyy):
  vals, vecs = np.linalg.eigh(cyy)
  return (vecs / np.sqrt(vals)) @ vecs.T


def route_r2(cxx, cyy, cxy, dim, m_of_w=None, k=None):
  """(rot_x, rot_y, e) by the kernel's algebra.  m_of_w: W -> W^T W of a wrong kernel; k: another C_yy^-1/2."""
  chol = np.linalg.cholesky(cxx)
  w = np.linalg.solve(chol, cxy)
  k = _inv_sqrt_full(cyy) if k is None else k
  b = k @ (w.T @ w if m_of_w is None else m_of_w(w)) @ k
  s2, v = np.linalg.eigh(0.5 * (b + b.T))
  order = np.argsort(-s2, kind='stable')[:dim]
  sig = np.sqrt(np.maximum(s2[order], 0.0))
  rot_y = k @ v[:, order]
  with np.errstate(divide='ignore', invalid='ignore'):
    rot_x = np.linalg.solve(chol.T, w @ (rot_y / sig))
  return rot_x, rot_y, sig


def smallest_pivot(cxx):
  """The smallest pivot L_ii^2 of the Cholesky factorisation, up to and including the first that is not positive."""
  try:
    return float(np.min(np.diag(np.linalg.cholesky(cxx)) ** 2))
  except np.linalg.LinAlgError:
    pass
  n = len(cxx)
  low = np.zeros((n, n))
  pmin = np.inf
  for j in range(n):
    d = cxx[j, j] - low[j, :j] @ low[j, :j]
    pmin = min(pmin, d)
    if not d > 0.0:
      break
    low[j, j] = np.sqrt(d)
    low[j + 1:, j] = (cxx[j + 1:, j] - low[j + 1:, :j] @ low[j, :j]) / low[j, j]
  return float(pmin)


Rules = collections.namedtuple('Rules', 'status rule margin')


def status_rules(cxx, cyy, cxy, dim, eps=EPS_EIG):
  """The device's three rules in its order of precedence here (any one marks the pair).  rule: 0 none, 1 no Cholesky
  factor (smallest L_ii^2 <= 64 k1 2^-52 max|diag|), 2 an eigenvalue of C_yy <= eps, 3 sigma_dim <= 1e-6 sigma_1.
  margin: the factor by which the deciding quantity is away from its threshold (status 0: the smallest of the
  three).  Rule 3 is stated on R1's singular values, which are good to a few 2^-53 sigma_1.  The device's sigma_dim is
  the root of an eigenvalue of B and so uncertain by about sqrt(K2 2^-52) sigma_1 < 3e-8 sigma_1, 30 times below the
  threshold: a reference ratio 1e3 away from 1e-6 on either side puts the device on the same side."""
  tol = 64.0 * len(cxx) * 2.0 ** -52 * np.max(np.abs(np.diag(cxx)))
  pmin = smallest_pivot(cxx)
  if not pmin > tol:
    return Rules(1, 1, np.inf if pmin <= 0.0 else tol / pmin)
  ymin = float(np.linalg.eigvalsh(cyy)[0])
  if not ymin > eps:
    return Rules(1, 2, np.inf if ymin <= 0.0 else eps / ymin)
  sig = route_r1(cxx, cyy, cxy, dim, eps)[2]
  if not sig[-1] > 1e-6 * sig[0]:
    return Rules(1, 3, np.inf if sig[-1] <= 0.0 else 1e-6 * sig[0] / sig[-1])
  return Rules(0, 0, min(pmin / tol, ymin / eps, sig[-1] / (1e-6 * sig[0])))


def _align(gx, gy, rx, ry):
  """The sign per component that brings (gx, gy) onto (rx, ry) jointly."""
  with np.errstate(invalid='ignore'):
    s = np.sign(np.sum(gx * rx, axis=0) / np.sum(rx * rx, axis=0) + np.sum(gy * ry, axis=0) / np.sum(ry * ry, axis=0))
  return np.where(s == 0, 1.0, s)


# one (fold, lambda) pair: R1's results, the uncertainty D and the gap
Pair = collections.namedtuple('Pair', 'rules rot_x rot_y e d_e d_x d_y g')
# mean_x / mean_y: float32, per fold
Reference = collections.namedtuple('Reference', 'pairs mean_x mean_y k1 k2 dim')


def reference(total, parts, folds, lambdas, dim, eps=EPS_EIG):
  """pairs[f][l] for every fold and lambda (rot_x .. g are None where the pair's status is 1, or where the fold's
  moments are not finite -- then the status is 1 by the NaN tests of the rules)."""
  k1, k2 = len(total.sx), len(total.sy)
  pairs, mean_x, mean_y = [], [], []
  for fold in folds:
    s = fold_sums(total, parts, fold)
    inv_frames = 1.0 / s.frames
    mean_x.append((s.sx * inv_frames).astype(np.float32))
    mean_y.append((s.sy * inv_frames).astype(np.float32))
    row = []
    for lam in lambdas:
      cxx, cyy, cxy, _, _ = covariances(s, lam)
      if not (np.all(np.isfinite(cxx)) and np.all(np.isfinite(cyy)) and np.all(np.isfinite(cxy))):
        row.append(Pair(Rules(1, 0, np.inf), None, None, None, None, None, None, None))
        continue
      rules = status_rules(cxx, cyy, cxy, dim, eps)
      if rules.status:
        row.append(Pair(rules, None, None, None, None, None, None, None))
        continue
      rx, ry, e, every = route_r1(cxx, cyy, cxy, dim, eps)
      qx, qy, qe = route_r2(cxx, cyy, cxy, dim)
      sign = _align(qx, qy, rx, ry)
      d_x = np.max(np.abs(qx * sign - rx), axis=0) / np.max(np.abs(rx), axis=0)
      d_y = np.max(np.abs(qy * sign - ry), axis=0) / np.max(np.abs(ry), axis=0)
      lead = every[:dim + 1]
      g = float(np.min(lead[:-1] - lead[1:]) / every[0]) if len(lead) > 1 else 1.0
      row.append(Pair(rules, rx, ry, e, float(np.max(np.abs(qe - e))), d_x, d_y, g))
    pairs.append(row)
  return Reference(pairs, mean_x, mean_y, k1, k2, dim)


def pair_bounds(p, k1, k2):
  """(bound of e [dim], of rot_x [k1, dim], of rot_y [k2, dim])"""
  floor = 64.0 * (k1 + k2) * U64
  be = U32 * np.abs(p.e) + 8.0 * p.d_e + floor
  bx = U32 * np.abs(p.rot_x) + (8.0 * p.d_x + floor / p.g) * np.max(np.abs(p.rot_x), axis=0)
  by = U32 * np.abs(p.rot_y) + (8.0 * p.d_y + floor / p.g) * np.max(np.abs(p.rot_y), axis=0)
  return be, bx, by


Report = collections.namedtuple('Report', 'status_ok means_ok bias_ok err_e err_rot ratio_e ratio_rot bound_e '
                                          'bound_rot d_e d_rot g pairs_checked failures')


def check(out, ref):
  """Every output of every pair of (rot_x [F, k1, L dim], rot_y, mean_x [F, k1], mean_y, bias_x [F, L dim], bias_y,
  e [F, L, dim], status [F, L]) against the reference.  err_*: the largest |gpu - ref| (rotations: relative to the
  column's largest entry); ratio_*: the largest |gpu - ref| / bound, <= 1 inside; bound_*: the smallest bound met
  (rotations: relative likewise).  Of a status-1 pair only the status is looked at."""
  rot_x, rot_y, mean_x, mean_y, bias_x, bias_y, e, status = (np.asarray(a) for a in out)
  dim, k1, k2 = ref.dim, ref.k1, ref.k2
  fails = []
  status_ok = means_ok = bias_ok = True
  err_e = err_rot = ratio_e = ratio_rot = d_e = d_rot = 0.0
  bound_e = bound_rot = g = np.inf
  checked = 0
  for f, row in enumerate(ref.pairs):
    if not any(p.rules.status and p.rules.rule == 0 for p in row):       # (a fold of NaN moments has no means to hold)
      if not (np.array_equal(mean_x[f], ref.mean_x[f]) and np.array_equal(mean_y[f], ref.mean_y[f])):
        means_ok = False
        fails.append('fold %d: means differ by %.3g / %.3g' % (
            f, np.max(np.abs(mean_x[f].astype(np.float64) - ref.mean_x[f])),
            np.max(np.abs(mean_y[f].astype(np.float64) - ref.mean_y[f]))))
    for l, p in enumerate(row):
      if int(status[f, l]) != p.rules.status:
        status_ok = False
        fails.append('pair (%d, %d): status %d, not %d (rule %d)' % (f, l, status[f, l], p.rules.status, p.rules.rule))
        continue
      if p.rules.status:
        continue
      checked += 1
      cols = slice(l * dim, (l + 1) * dim)
      gx, gy = rot_x[f][:, cols].astype(np.float64), rot_y[f][:, cols].astype(np.float64)
      ge = e[f, l].astype(np.float64)
      be, bx, by = pair_bounds(p, k1, k2)
      sign = _align(gx, gy, p.rot_x, p.rot_y)
      with np.errstate(invalid='ignore'):
        de = np.abs(ge - p.e)
        dx, dy = np.abs(gx * sign - p.rot_x), np.abs(gy * sign - p.rot_y)
        de, dx, dy = (np.where(np.isfinite(a), a, np.inf) for a in (de, dx, dy))
      sx, sy = np.max(np.abs(p.rot_x), axis=0), np.max(np.abs(p.rot_y), axis=0)
      err_e, ratio_e = max(err_e, de.max()), max(ratio_e, (de / be).max())
      err_rot = max(err_rot, (dx / sx).max(), (dy / sy).max())
      ratio_rot = max(ratio_rot, (dx / bx).max(), (dy / by).max())
      bound_e, bound_rot = min(bound_e, be.min()), min(bound_rot, (bx / sx).max(axis=0).min(), (by / sy).max(axis=0).min())
      d_e, d_rot, g = max(d_e, p.d_e), max(d_rot, p.d_x.max(), p.d_y.max()), min(g, p.g)
      if (de / be).max() > 1.0 or (dx / bx).max() > 1.0 or (dy / by).max() > 1.0:
        fails.append('pair (%d, %d): e %.3g x bound, rot_x %.3g x, rot_y %.3g x' % (
            f, l, (de / be).max(), (dx / bx).max(), (dy / by).max()))
      # the biases: float32 roundings of the float64 -mean . rot
      for bias, mean, rot in ((bias_x, mean_x, gx), (bias_y, mean_y, gy)):
        want = -(mean[f].astype(np.float64) @ rot)
        scale = np.sum(np.abs(mean[f][:, None] * rot), axis=0) + 1e-30
        if not np.all(np.abs(bias[f][cols] - want) <= 1e-6 * scale):
          bias_ok = False
          fails.append('pair (%d, %d): bias off by %.3g of its scale' % (f, l, np.max(np.abs(bias[f][cols] - want) / scale)))
  return Report(status_ok, means_ok, bias_ok, float(err_e), float(err_rot), float(ratio_e), float(ratio_rot),
                float(bound_e), float(bound_rot), float(d_e), float(d_rot), float(g), checked, fails)


# ---- numpy models of the kernel, right and wrong ----------------------------------------------------------------------
WRONG = ('drop_last_block', 'ut_from_8_zero', 'chunk_state', 'flip_sign')


def model(total, parts, folds, lambdas, dim, wrong=None):
  """The call's eight outputs by the kernel's algebra (R2) in float64, rounded to float32.  wrong:
    'drop_last_block'  W^T W without the last 64-column block of W^T (np > 64)
    'ut_from_8_zero'   components >= 8 of the backward pass's right-hand sides zero: rot_x[:, 8:] = 0
    'chunk_state'      the folds of the second chunk take C_yy and the means of the first chunk's folds
    'flip_sign'        the first term of every fold with terms enters with the other sign
  Pairs the rules mark get status 1 and zeros."""
  assert wrong is None or wrong in WRONG
  k1, k2, n_f, n_l = len(total.sx), len(total.sy), len(folds), len(lambdas)
  pl = plan(k1, k2, dim, n_f, n_l)
  rot_x, rot_y = np.zeros((n_f, k1, n_l * dim)), np.zeros((n_f, k2, n_l * dim))
  mean_x, mean_y = np.zeros((n_f, k1)), np.zeros((n_f, k2))
  e, status = np.zeros((n_f, n_l, dim)), np.zeros((n_f, n_l), np.int32)
  sums = [fold_sums(total, parts, fold, flip=0 if wrong == 'flip_sign' else None) for fold in folds]
  for f, s in enumerate(sums):
    stale = sums[f - pl.chunk] if wrong == 'chunk_state' and f >= pl.chunk else s
    for l, lam in enumerate(lambdas):
      cxx, cyy, cxy, mx, my = covariances(s, lam)
      if stale is not s:
        _, cyy, _, mx, my = covariances(stale, lam)
      mean_x[f], mean_y[f] = mx, my
      if status_rules(cxx, cyy, cxy, dim).status:
        status[f, l] = 1
        continue
      m_of_w = None
      if wrong == 'drop_last_block':
        m_of_w = lambda w: w[:pl.np - NB].T @ w[:pl.np - NB]
      rx, ry, sig = route_r2(cxx, cyy, cxy, dim, m_of_w)
      if wrong == 'ut_from_8_zero':
        rx[:, 8:] = 0.0
      cols = slice(l * dim, (l + 1) * dim)
      rot_x[f][:, cols], rot_y[f][:, cols], e[f, l] = rx, ry, sig
  bias_x = -np.einsum('fk,fkc->fc', mean_x, rot_x)
  bias_y = -np.einsum('fk,fkc->fc', mean_y, rot_y)
  f32 = lambda a: np.ascontiguousarray(a, np.float32)
  return (f32(rot_x), f32(rot_y), f32(mean_x), f32(mean_y), f32(bias_x), f32(bias_y), f32(e), status)


# ---- end to end: a sweep whose lambda = 0 pairs the device call must refuse ---------------------------------------------
E2E = dict(pre=0, post=2, pre2=1, post2=1, dim=2, lambdas=(0.0, 0.1), batch=100)      # K1 = 18, K2 = 6


@functools.lru_cache(maxsize=None)
def e2e_files():
  """Three short recordings (every fold's training stream drops a remainder) whose second EEG channel repeats the
  first: without lambda C_xx has no Cholesky factor.  (x, x2, output, attended) float32; shared: not to be written."""
  rng = np.random.default_rng(11)
  mix = rng.standard_normal((2, 6)) / np.sqrt(2.0)
  files = []
  for n in (430, 380, 410):
    s = rng.standard_normal((n, 2))
    x = (s @ mix + 0.5 * rng.standard_normal((n, 6)) + 0.5).astype(np.float32)
    x[:, 1] = x[:, 0]
    x2 = (np.array([0.9, 0.6]) * s + 0.5 * rng.standard_normal((n, 2)) - 0.5).astype(np.float32)
    files.append((x, x2, x2[:, :1].copy(), np.zeros((n, 1), np.float32)))
  return tuple(files)


@functools.lru_cache(maxsize=None)
def e2e_oracle():
  """{(fold, lambda index): held-out r} by from-scratch float64 refits (tests/host_cca_sweep.oracle_refit)."""
  from tests import host_cca_sweep as hc
  c = E2E
  return {(f, li): hc.oracle_refit(e2e_files(), f, lam, c['dim'], c['pre'], c['post'], c['pre2'], c['post2'],
                                   batch=c['batch'])
          for f in range(3) for li, lam in enumerate(c['lambdas'])}
