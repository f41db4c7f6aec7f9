"""NumPy stand-in for the device layer of the CCA sweep (telluride_decoding_amd.cca_sweep).  Test infrastructure.

The sweep's orchestration (which recordings enter which fold, the signed terms, the remainder batching drops, the
held-out evaluation, the fallback rule) is host code around the device layer; with this module injected as that
layer it runs without a GPU, the way tests/host_device.py serves the ridge sweep.  Statistics are the raw float64
sums of the materialised lag matrices (what the reference accumulates, cca.py:304-332); cca_solve_loso_terms restates
the arithmetic of td_cca_solve_loso_terms in float64 NumPy.  Never imported by the product.
"""
import functools

import numpy as np
import torch

from oracle import cca as o_cca
from oracle import lag as o_lag
from oracle import pearson as o_pearson
from tests.host_device import default_handle, predict_fir, window_scores, window_sums   # noqa: F401 (the interface)

MAX_K2 = 64
CALLS = {'cca_solve_loso_terms': 0, 'cca_solve': 0}     # (what a test asserts the sweep went through)


class LagStats(object):
  """Raw sums of [lagged x] and [lagged x2]: the interface of device.LagStats that the CCA sweep uses."""

  def __init__(self, c1, pre1=0, post1=0, c2=0, pre2=0, post2=0, d=0, handle=None):
    assert c2 > 0 and d == 0, 'the stand-in covers the CCA statistics'
    self.c1, self.pre1, self.post1 = int(c1), int(pre1), int(post1)
    self.c2, self.pre2, self.post2 = int(c2), int(pre2), int(post2)
    self.k1 = self.c1 * (self.pre1 + 1 + self.post1)
    self.k2 = self.c2 * (self.pre2 + 1 + self.post2)
    self.h = handle or default_handle()
    self.reset()

  def reset(self):
    self.sxx = np.zeros((self.k1, self.k1))
    self.syy = np.zeros((self.k2, self.k2))
    self.sxy = np.zeros((self.k1, self.k2))
    self.sx = np.zeros(self.k1)
    self.sy = np.zeros(self.k2)
    self.frames = 0

  def accumulate(self, x, x2=None, y=None, file_offsets=None, input_offset=0, rows_used=None, handle=None):
    x, x2 = np.asarray(x, np.float64), np.asarray(x2, np.float64)
    offs = [0, x.shape[0]] if file_offsets is None else [int(v) for v in file_offsets]
    for f in range(len(offs) - 1):
      xf, x2f = x[offs[f]:offs[f + 1]], x2[offs[f]:offs[f + 1]]
      xl, x2l, _, _ = o_lag.window_streams(xf, x2f, np.zeros((xf.shape[0], 1)), np.zeros((xf.shape[0], 1)),
                                           pre=self.pre1, post=self.post1, pre2=self.pre2, post2=self.post2,
                                           input_offset=input_offset)
      n = xl.shape[0] if rows_used is None else int(rows_used[f])
      assert 0 <= n <= xl.shape[0]
      xl, x2l = xl[:n], x2l[:n]
      self.sxx += xl.T @ xl
      self.syy += x2l.T @ x2l
      self.sxy += xl.T @ x2l
      self.sx += xl.sum(0)
      self.sy += x2l.sum(0)
      self.frames += n

  def counts(self):
    return self.frames, 1

  def combine(self, parts):
    self.reset()
    for p in parts:
      self._add(p, 1.0)
    return self

  def _add(self, p, sign):
    self.sxx += sign * p.sxx
    self.syy += sign * p.syy
    self.sxy += sign * p.sxy
    self.sx += sign * p.sx
    self.sy += sign * p.sy
    self.frames += int(sign) * p.frames

  def _covariances(self, denom, lam):
    mx, my = self.sx / self.frames, self.sy / self.frames
    cxx = self.sxx / denom - np.outer(mx, mx) + lam * np.eye(self.k1)
    cyy = self.syy / denom - np.outer(my, my) + lam * np.eye(self.k2)
    cxy = self.sxy / denom - np.outer(mx, my)
    return cxx, cyy, cxy, mx, my

  def cca_solve(self, denom, regularization, dim, eps_eig=1e-12, handle=None):
    """The reference's own route (two eigen-decompositions, an SVD): what the fallback calls."""
    CALLS['cca_solve'] += 1
    cxx, cyy, cxy, mx, my = self._covariances(denom, regularization)

    def inv_sqrt(c):
      vals, vecs = np.linalg.eigh(c)
      keep = vals > eps_eig
      return (vecs[:, keep] / np.sqrt(vals[keep])) @ vecs[:, keep].T

    k11, k22 = inv_sqrt(cxx), inv_sqrt(cyy)
    u, e, vt = np.linalg.svd(k11 @ cxy @ k22, full_matrices=False)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return (f32(k11 @ u[:, :dim]), f32(k22 @ vt.T[:, :dim]), f32(mx[None]), f32(my[None]), f32(e[:dim]), (0, 0, 0))

  @staticmethod
  def cca_solve_loso_terms(total, fold_terms, fold_batches, batch_size, lambdas, dim, eps_eig=1e-12, handle=None):
    """td_cca_solve_loso_terms in float64: fold = total + signed terms; Z = C_xx^-1 C_xy by Cholesky,
    K = C_yy^-1/2, B = K C_xy^T Z K = V sigma^2 V^T, rot_y = K V, rot_x = Z K V / sigma."""
    CALLS['cca_solve_loso_terms'] += 1
    if total.k2 > MAX_K2 or any(len(t) > 4 for t in fold_terms):
      raise ValueError('td_cca_solve_loso_terms: out of range')
    n_f, n_l, k1, k2 = len(fold_terms), len(lambdas), total.k1, total.k2
    rot_x, rot_y = np.zeros((n_f, k1, n_l * dim)), np.zeros((n_f, k2, n_l * dim))
    mean_x, mean_y = np.zeros((n_f, k1)), np.zeros((n_f, k2))
    e = np.zeros((n_f, n_l, dim))
    status = np.zeros((n_f, n_l), np.int32)
    for f, terms in enumerate(fold_terms):
      st = LagStats(total.c1, total.pre1, total.post1, total.c2, total.pre2, total.post2)
      st._add(total, 1.0)
      for term, sign in terms:
        assert sign in (1.0, -1.0)
        st._add(term, sign)
      assert st.frames == int(fold_batches[f]) * int(batch_size), 'the fold holds other frames than its minibatches'
      for li, lam in enumerate(lambdas):
        cxx, cyy, cxy, mx, my = st._covariances(st.frames - 1, float(lam))
        mean_x[f], mean_y[f] = mx, my
        cols = slice(li * dim, (li + 1) * dim)
        try:
          chol = np.linalg.cholesky(cxx)
        except np.linalg.LinAlgError:
          status[f, li] = 1
          continue
        # (the device's pivot rule: LAPACK accepts a pivot of rounding noise that happens to come out positive)
        if not np.min(np.diag(chol)) ** 2 > 64.0 * k1 * 2.0 ** -52 * np.max(np.abs(np.diag(cxx))):
          status[f, li] = 1
          continue
        z = np.linalg.solve(chol.T, np.linalg.solve(chol, cxy))
        vals, vecs = np.linalg.eigh(cyy)
        if np.any(vals <= eps_eig):
          status[f, li] = 1
          continue
        k = (vecs / np.sqrt(vals)) @ vecs.T
        b = k @ (cxy.T @ z) @ k
        s2, v = np.linalg.eigh(0.5 * (b + b.T))
        order = np.argsort(-s2)[:dim]
        sig = np.sqrt(np.maximum(s2[order], 0.0))
        if not sig[-1] > 1e-6 * sig[0]:
          status[f, li] = 1
          continue
        rot_y[f][:, cols] = k @ v[:, order]
        rot_x[f][:, cols] = z @ rot_y[f][:, cols] / sig
        e[f, li] = sig
    bias_x = -np.einsum('fk,fkc->fc', mean_x, rot_x)
    bias_y = -np.einsum('fk,fkc->fc', mean_y, rot_y)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return (f32(rot_x), f32(rot_y), f32(mean_x), f32(mean_y), f32(bias_x), f32(bias_y), f32(e),
            torch.from_numpy(status))


def cca_transform(x, x2, file_offsets, mean1, rot1, mean2, rot2, pre1, post1, pre2, post2, handle=None,
                  input_offset=0):
  """[(lagged x - mean1) rot1 | (lagged x2 - mean2) rot2]; row file_offsets[f] + t = frame t of file f's streams."""
  x, x2 = np.asarray(x, np.float64), np.asarray(x2, np.float64)
  offs = [int(v) for v in file_offsets]
  dims = int(rot1.shape[1])
  out = np.zeros((x.shape[0], 2 * dims))
  for f in range(len(offs) - 1):
    xf, x2f = x[offs[f]:offs[f + 1]], x2[offs[f]:offs[f + 1]]
    xl, x2l, _, _ = o_lag.window_streams(xf, x2f, np.zeros((xf.shape[0], 1)), np.zeros((xf.shape[0], 1)), pre=pre1,
                                         post=post1, pre2=pre2, post2=post2, input_offset=input_offset)
    z = o_cca.cca_transform(xl, x2l, np.asarray(mean1, np.float64), np.asarray(mean2, np.float64),
                            np.asarray(rot1, np.float64), np.asarray(rot2, np.float64))
    out[offs[f]:offs[f] + z.shape[0]] = z
  return torch.from_numpy(out.astype(np.float32))



# ---- the two cases of the sweep's tests and their from-scratch oracle refits ---------------------------------------
BATCH = 100
CASE_A = dict(pre=1, post=4, pre2=2, post2=2, dim=3, lambdas=(1e-3, 0.1, 10.0))       # K1 = 48, K2 = 10
CASE_B = dict(pre=0, post=5, pre2=15, post2=15, dim=5,                                # K1 = 144, K2 = 31
              lambdas=tuple(float(v) for v in np.logspace(-2, 2, 7)))


@functools.lru_cache(maxsize=None)
def case_a_files(input_2_lags=None):
  """Five short recordings of unequal length (every fold's training stream drops a remainder), EEG with a large
  offset and noise (the means matter), two envelope channels + 0.5 as input_2.  float32; shared by the tests: not to be written."""
  from telluride_decoding_amd import synth
  del input_2_lags
  rng = np.random.default_rng(3)
  files = []
  for (eeg, env, att), n in zip(synth.make_trials(77, 5, 1300, 8), (1200, 1130, 1275, 1210, 1190)):
    x = (eeg[:n] + 4.0 * rng.standard_normal((n, eeg.shape[1])) + 2.0).astype(np.float32)
    x2 = (env[:n, :2] + 0.5).astype(np.float32)
    files.append((x, x2, env[:n, :1].astype(np.float32), att[:n]))
  return tuple(files)


@functools.lru_cache(maxsize=None)
def case_b_files():
  """Four recordings of 24 channels: K1 = 144 (above 128, no multiple of 64), one envelope x 31 lags."""
  from telluride_decoding_amd import synth
  files = []
  for (eeg, env, att), n in zip(synth.make_trials(77, 4, 3100, 24), (3000, 2950, 3075, 3010)):
    files.append((eeg[:n].astype(np.float32), env[:n, :1].astype(np.float32), env[:n, :1].astype(np.float32), att[:n]))
  return tuple(files)


def _files64(files):
  return [tuple(np.asarray(a, np.float64) for a in f) for f in files]


def oracle_refit(files, f, lam, dim, pre, post, pre2, post2, input_offset=0, batch=BATCH):
  """Held-out cca_pearson_correlation_first of fold f at lambda from scratch, in float64: the reference's CCA fit on
  the minibatches of the training files, the Keras mean of the metric over the held-out file's minibatches."""
  f64 = _files64(files)
  ctx = dict(pre=pre, post=post, pre2=pre2, post2=post2, input_offset=input_offset)
  train = [g for i, g in enumerate(f64) if i != f]
  rot_x, rot_y, mean_x, mean_y, _ = o_cca.cca_parameters_from_batches(o_lag.minibatches(train, batch, **ctx), dim,
                                                                      regularization=lam, mini_batch_count=0)
  vals = []
  for feats, _ in o_lag.minibatches([f64[f]], batch, **ctx):
    z = o_cca.cca_transform(feats['input_1'], feats['input_2'], mean_x, mean_y, rot_x, rot_y)
    vals.append(o_pearson.cca_pearson_correlation(None, z)[0])
  return float(np.mean(np.real(vals)))


@functools.lru_cache(maxsize=None)
def case_a_oracle(input_offset=0, input_2_lags=None):
  """[Lambda, F] oracle refits of case A (input_2_lags: pre2 = post2 = that instead of the case's 2)."""
  c = dict(CASE_A)
  if input_2_lags is not None:
    c['pre2'] = c['post2'] = int(input_2_lags)
  files = case_a_files()
  return np.array([[oracle_refit(files, f, lam, c['dim'], c['pre'], c['post'], c['pre2'], c['post2'], input_offset)
                    for f in range(len(files))] for lam in c['lambdas']])


CASE_B_PAIRS = ((0, 0), (1, 2), (2, 3), (3, 6), (0, 5), (2, 1))          # (fold, lambda index): every fold, both ends


@functools.lru_cache(maxsize=None)
def case_b_oracle():
  """{(fold, lambda index): r} of the six sampled pairs of case B."""
  c, files = CASE_B, case_b_files()
  return {(f, li): oracle_refit(files, f, c['lambdas'][li], c['dim'], c['pre'], c['post'], c['pre2'], c['post2'])
          for f, li in CASE_B_PAIRS}
