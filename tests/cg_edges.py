"""The edge cases of the two one-launch conjugate-gradient ridge solvers of csrc/cg.hip (tests/test_gpu_cg_edges.py,
tests/test_cpu_cg_edges.py): the case tables of cg_resident_kernel<R = 1..8> and cg_toeplitz_kernel<kCpw = 1, 2>, the
data builder, the float64 reference with its derived bound, restatements of the integer arithmetic by which
td_cg_solve_dense and td_cg_solve_compact pick an instance and a grid, and numpy models of a wrong product.  A plain
module, not a conftest.

The reference isolates the solver: A = xtx / frames + lambda I WITH the bias row (brain_model.py:447-477), rhs =
xty / frames, both from the device's own float64 moments (LagStats.moments()), solved by np.linalg.solve.  For the
resident kernel that matrix is literally its input; for the compact kernel it comes from the expansion kernels of
stats_moments.hip, code independent of the kernel's own block-Toeplitz-plus-head-window product.

The bound, elementwise for w and for b:   |gpu - ref| <= 2^-24 |ref| + E,
  E = 4 cond(A) sqrt(accept) 1e-12 ||[w_ref; b_ref]||_2
2^-24 |ref| is the float32 rounding of the output.  The kernel reports status 0 only when the TRUE residual of the
reduced system is within sqrt(accept) tol of |rhs| (accept = 100 with set_solver('cg'), 4 on the automatic route, tol =
1e-12), an error of the solution of at most cond(A) times that, relative to its norm; the reduced system is a Schur
complement of A, whose condition number cond(A) bounds.  The factor 4 covers the float64 rounding of the residual's own
evaluation and of the bias elimination.  cond(A) comes from np.linalg.eigvalsh of the reference matrix."""
import collections
import functools

import numpy as np

from oracle import lag as o_lag

TOL = 1e-12            # kCgTol of solve.hip
ACCEPT_CHOICE = 100.0  # set_solver('cg'): the true residual may be sqrt(100) tol
ACCEPT_AUTO = 4.0      # the automatic route and asynchronous solves on an 'auto' handle
LAM = 0.1

# ---- the route arithmetic of cg.hip / solve.hip, restated -----------------------------------------------------------
THREADS = 512          # kCgThreads
WAVES = 8              # kCgWaves
MAX_COLS = 4           # kCgMaxCols: k <= 2048
MAX_Q = 512            # kCgtMaxQ
LDS_BYTES = 160 * 1024 - 64
AUTO_MIN_N = 128       # kCgAutoMinN1: the synchronous compact route starts here
DEFAULT_CUS = 256


def cg_rows(k, cus):
  """td_cg_rows: rows per workgroup of the resident kernel, 0 when it does not fit."""
  if k < 1 or cus < 1 or k > THREADS * MAX_COLS:
    return 0
  rows = -(-k // cus)
  if rows > 8:
    return 0
  lds = 8 * (rows * ((k + 1) & ~1) + 14 * WAVES + 16)
  return rows if lds <= LDS_BYTES else 0


def dense_plan(k, cus):
  """(R, workgroups) of td_cg_solve_dense, None when td_cg_rows refuses."""
  rows = cg_rows(k, cus)
  return (rows, -(-k // rows)) if rows else None


def compact_plan(c, post, files, cus, n_lambda=1, per_cu=1):
  """(kCpw, workgroups) of td_cg_solve_compact for statistics summed whole, None where it refuses.  per_cu: what the
  occupancy query answers -- every instance of cg.hip needs 182..256 VGPRs at 512 threads: one workgroup per CU."""
  lags = post + 1
  k, nq = c * lags, files * post
  if c < 2 or c > 64 or c & 1 or lags < 1 or lags > 32 or k > THREADS * MAX_COLS or nq > MAX_Q or n_lambda < 1:
    return None
  for cpw in (1, 2):
    wgs = -(-c // cpw)
    q_waves = nq if cpw == 1 else files * ((post + 1) // 2)
    if per_cu * cus >= wgs and q_waves <= WAVES * wgs:
      return cpw, wgs
  return None


def sync_takes_compact(k, cus):
  """A synchronous ridge_solve asks the compact solver exactly when the dense matrix does not fit the handle's CUs."""
  return cg_rows(k, cus) == 0 and k + 1 >= AUTO_MIN_N


# ---- the tables -----------------------------------------------------------------------------------------------------
# declared: the CU count the handle declares (td_set_cu_count) on an unmasked stream, None = the default handle
ResidentCase = collections.namedtuple('ResidentCase', 'c post frames files lams d declared rows workgroups')
# where: ('masked', n) a stream really masked to n CUs, ('declared', n), ('default',)
CompactCase = collections.namedtuple('CompactCase', 'c post frames files lams d where use_async cpw workgroups')
RefusedCase = collections.namedtuple('RefusedCase', 'c post frames files lams d where why')


def _resident_table():
  t = []
  for declared, wgs in zip((97, 49, 33, 25, 20, 17, 14, 13), (97, 49, 33, 25, 20, 17, 14, 13)):    # k = 97: odd, prime
    t.append(ResidentCase(97, 0, 300, 2, (LAM,), 1, declared, len(t) + 1, wgs))
  for r, (declared, wgs) in enumerate(zip((99, 50, 33, 25, 20, 17, 15, 13), (99, 50, 33, 25, 20, 17, 15, 13))):
    t.append(ResidentCase(9, 10, 300, 2, (LAM,), 1, declared, r + 1, wgs))                         # k = 99
  t.append(ResidentCase(9, 10, 300, 2, (0.05, 2.0), 2, 17, 6, 17))       # four systems in one launch
  t.append(ResidentCase(12, 7, 300, 2, (LAM,), 1, 12, 8, 12))            # k = 96: 12 full workgroups of 8 rows
  t.append(ResidentCase(41, 24, 3000, 2, (LAM,), 1, None, 5, 205))       # k = 1025: one column in the second pair group
  t.append(ResidentCase(33, 30, 3000, 2, (LAM,), 1, None, 4, 256))       # k = 1023
  t.append(ResidentCase(89, 22, 3000, 2, (LAM,), 1, None, 8, 256))       # k = 2047, row stride 2048
  t.append(ResidentCase(2, 0, 300, 2, (LAM,), 1, None, 1, 2))            # k = 2
  t.append(ResidentCase(1, 2, 300, 2, (LAM,), 1, None, 1, 3))            # k = 3
  return t


RESIDENT_CASES = _resident_table()

COMPACT_CASES = [
    CompactCase(64, 31, 400, 3, (LAM,), 1, ('masked', 32), False, 2, 32),    # odd post: the last pair of a recording is single
    CompactCase(64, 30, 400, 3, (LAM,), 1, ('masked', 32), False, 2, 32),    # every pair double; L = 31: 7 rows at a0 = 24
    CompactCase(64, 31, 400, 16, (LAM,), 1, ('masked', 32), False, 2, 32),   # 256 pairs = 256 waves
    CompactCase(64, 31, 400, 16, (LAM,), 1, ('masked', 64), False, 1, 64),   # 496 q numbers of 512
    CompactCase(34, 8, 400, 2, (LAM,), 1, ('declared', 17), False, 2, 17),   # lanes 34..63 masked, L = 9
    CompactCase(6, 31, 400, 1, (LAM,), 1, ('declared', 3), False, 2, 3),
    CompactCase(4, 31, 400, 1, (LAM,), 1, ('declared', 4), False, 1, 4),
    CompactCase(4, 31, 400, 1, (LAM,), 1, ('declared', 2), False, 2, 2),     # 16 pairs = 16 waves: q capacity full
    CompactCase(16, 20, 400, 2, (LAM,), 3, ('declared', 16), False, 1, 16),  # L = 21: one row in the last busy wave; 3 systems
    CompactCase(64, 0, 400, 2, (LAM,), 1, ('declared', 32), True, 2, 32),    # no q numbers at all
    CompactCase(2, 5, 400, 2, (LAM,), 1, ('default',), True, 1, 2),
]

REFUSED_CASES = [
    RefusedCase(33, 9, 400, 2, (LAM,), 1, ('declared', 16), 'odd C'),
    RefusedCase(8, 32, 400, 2, (LAM,), 1, ('declared', 16), 'L = 33'),
]


def case_id(case):
  where = getattr(case, 'where', None)
  if where is None:
    tag = 'cu%s' % (case.declared if case.declared else 'all')
  else:
    tag = where[0] + ('%d' % where[1] if len(where) > 1 else '')
  return 'c%d-post%d-f%d-d%d-l%d-%s%s' % (case.c, case.post, case.files, case.d, len(case.lams), tag,
                                          '-async' if getattr(case, 'use_async', False) else '')


def case_cus(case):
  """CUs the case's handle declares."""
  where = getattr(case, 'where', None)
  if where is None:
    return case.declared or DEFAULT_CUS
  return where[1] if len(where) > 1 else DEFAULT_CUS


def case_accept(case):
  """The `accept` the case's solve runs with: the resident cases choose the solver (set_solver('cg')), the compact
  cases leave the handle on 'auto' -- as a pipelined fit does."""
  return ACCEPT_CHOICE if isinstance(case, ResidentCase) else ACCEPT_AUTO


# ---- data -----------------------------------------------------------------------------------------------------------
def make_data(case, seed=3):
  """White-noise EEG, envelope 0.5 eeg[:, :d] + noise, float32; `files` recordings of equal length, summed whole."""
  rng = np.random.default_rng(seed)
  rows = case.files * case.frames
  eeg = rng.standard_normal((rows, case.c)).astype(np.float32)
  env = (eeg[:, :case.d] * 0.5 + rng.standard_normal((rows, case.d))).astype(np.float32)
  offs = np.arange(case.files + 1, dtype=np.int64) * case.frames
  return eeg, env, offs


def cpu_moments(case):
  """(xtx [n, n], xty [n, d], frames) of the case's data in float64 from the materialised lag matrix (oracle.lag), the
  bias column last: what LagStats.moments() holds up to the accumulate's rounding."""
  return _cpu_moments(case.c, case.post, case.frames, case.files, case.d)


@functools.lru_cache(maxsize=None)
def _cpu_moments(c, post, frames, files, d):
  case = ResidentCase(c, post, frames, files, (LAM,), d, None, 0, 0)
  eeg, env, offs = make_data(case)
  x = np.concatenate([o_lag.lag_matrix(eeg[offs[i]:offs[i + 1]].astype(np.float64), 0, post) for i in range(files)])
  x = np.concatenate((x, np.ones((len(x), 1))), axis=1)
  return x.T @ x, x.T @ env.astype(np.float64), len(x)


# ---- the reference and the bound ------------------------------------------------------------------------------------
Reference = collections.namedtuple('Reference', 'w b cond e')      # w [n_lambda, k, d], b [n_lambda, d], cond [n_lambda], e [n_lambda, d]


def reference(xtx, xty, frames, lams, accept):
  xtx, xty = np.asarray(xtx, np.float64), np.asarray(xty, np.float64)
  n, d = xty.shape
  w = np.empty((len(lams), n - 1, d))
  b = np.empty((len(lams), d))
  cond = np.empty(len(lams))
  e = np.empty((len(lams), d))
  for li, lam in enumerate(lams):
    a = xtx / frames + lam * np.eye(n)
    sol = np.linalg.solve(a, xty / frames)
    ev = np.linalg.eigvalsh(a)
    cond[li] = ev[-1] / ev[0]
    w[li], b[li] = sol[:-1], sol[-1]
    e[li] = 4.0 * cond[li] * np.sqrt(accept) * TOL * np.linalg.norm(sol, axis=0)
  return Reference(w, b, cond, e)


def bounds(ref):
  """The elementwise bounds of w and b."""
  return 2.0 ** -24 * np.abs(ref.w) + ref.e[:, None, :], 2.0 ** -24 * np.abs(ref.b) + ref.e


def distance(w, b, ref):
  """(largest |w - w_ref|, largest |b - b_ref|, the largest distance / bound over both): <= 1 is inside the bound."""
  bw, bb = bounds(ref)
  dw, db = np.abs(np.asarray(w, np.float64) - ref.w), np.abs(np.asarray(b, np.float64) - ref.b)
  return float(dw.max()), float(db.max()), float(max((dw / bw).max(), (db / bb).max()))


# ---- numpy models of a wrong product --------------------------------------------------------------------------------
def cg_model(product, rhs, max_iter=400, tol=TOL):
  """Conjugate gradients as the kernels run them (stop at a recurrence residual of tol |rhs|, max_iter at most) with
  `product` for A v.  Returns (x, converged)."""
  x = np.zeros_like(rhs)
  r = rhs.copy()
  p = r.copy()
  gamma = r @ r
  b2 = gamma
  for _ in range(max_iter):
    if gamma <= tol * tol * b2:
      return x, True
    v = product(p)
    denom = p @ v
    if not denom > 0.0 or not np.isfinite(denom):
      return x, False
    alpha = gamma / denom
    x = x + alpha * p
    r = r - alpha * v
    gamma_new = r @ r
    p = r + (gamma_new / gamma) * p
    gamma = gamma_new
  return x, bool(gamma <= tol * tol * b2)


def wrong_row_product(a, row):
  """A v with entry `row` taken from its neighbour's row (a lane-to-row map that is off by one for one row)."""
  other = row + 1 if row + 1 < len(a) - 1 else row - 1
  def product(v):
    out = a @ v
    out[row] = out[other]
    return out
  return product


def head_terms(case, eeg, offs):
  """The head-window part of the compact form: M = T - sum over (file f, s < post) of head_term[f, s], where T is the
  block-Toeplitz matrix of the lagged covariances G and head_term[f, s][(a, i), (b, j)] = x_f[s][i] x~_f[s + b - a][j]
  for a > s (x~ zero in front of the recording).  Yields ((f, s), term [k, k])."""
  c, lags = case.c, case.post + 1
  for f in range(case.files):
    x = eeg[offs[f]:offs[f + 1]].astype(np.float64)
    for s in range(case.post):
      term = np.zeros((lags, c, lags, c))
      for a in range(s + 1, lags):
        for bb in range(lags):
          u = s + bb - a
          if u >= 0:
            term[a, :, bb, :] = np.outer(x[s], x[u])
      yield (f, s), term.reshape(lags * c, lags * c)


def toeplitz_part(case, eeg, offs):
  """T[(a, i), (b, j)] = G[b - a][i][j], G[e][i][j] = sum over files and rows s of x_f[s][i] x~_f[s + e][j]."""
  c, lags = case.c, case.post + 1
  g = np.zeros((2 * lags - 1, c, c))
  for f in range(case.files):
    x = eeg[offs[f]:offs[f + 1]].astype(np.float64)
    for e in range(lags):
      g[lags - 1 + e] += x[:len(x) - e].T @ x[e:]
      g[lags - 1 - e] = g[lags - 1 + e].T
  t = np.empty((lags, c, lags, c))
  for a in range(lags):
    for bb in range(lags):
      t[a, :, bb, :] = g[lags - 1 + bb - a]
  return t.reshape(lags * c, lags * c)


# ---- handles --------------------------------------------------------------------------------------------------------
def masked_handle(dev, cus=64):
  """A handle on a stream masked to the first `cus` CUs (the solve partition of a pipelined fit)."""
  import ctypes
  import torch
  from telluride_decoding_amd import _lib
  lib = _lib.load()
  p = ctypes.c_void_p()
  assert lib.td_stream_create_masked(0, 0, cus, ctypes.byref(p)) == 0
  stream = torch.cuda.ExternalStream(p.value)
  with torch.cuda.stream(stream):
    h = dev.Handle()
  h.check(lib.td_set_cu_count(h.ptr, cus))
  return h, stream, (lib, p)
