"""Leave-one-file-out x lambda sweep of the CCA model (the codelab's CCA jackknife).

Reference: doc/DecodingCodelab.md:344-411 and regression.RegressionCCA / Telluride4CCA / JensMemoryCCA / TFRecordsCCA
train a CCA model (cca.calculate_cca_parameters_from_dataset, cca.py:272-369) on all files but one, test on the
held-out file with 'cca_pearson_correlation_first', and repeat for every file and every regularisation value:
F x Lambda passes over the data, two K1-sized eigen-decompositions each.  The CCA statistics (sums of x^T x, y^T y,
x^T y, x, y) are additive over files and independent of lambda, so here:

  1. every recording is read ONCE: one accumulate per file gives its CCA statistics,
  2. fold f's training statistics are the total's plus a few signed terms: minus the held-out recording, and -- when
     batching drops a remainder from the end of the training stream (brain_data.py:369-370) -- minus the last training
     recordings plus the same accumulated without the frames that fall off (at most four terms),
  3. ALL (fold, lambda) dense stages are solved in batches on the device (device.LagStats.cca_solve_loso_terms: the
     fold covariances straight into the batched float64 Cholesky, the K2-sized stages in one workgroup per pair),
  4. a fold's held-out file is projected by ALL of the fold's models together -- the rotations come k-major, a fold's
     models as the output columns of one filter with bias = -mean . rot, so (x - mean_x) rot_x is one FIR prediction of
     input_1 and (y - mean_y) rot_y one of input_2 -- and scored by one window-sums and one window-scores launch
     (Keras `evaluate` = the unweighted mean of the per-minibatch metric over the held-out stream's full minibatches;
     the Pearson zero rule over that model's own `dim` columns).

The arithmetic (cca.py:337-367): with nb minibatches of B frames in a fold's training stream, mean = sum / (nb B),
C_xx = S_xx / (nb B - 1) - m^T m + lambda I, C_yy likewise (lambda on BOTH sides), C_xy = S_xy / (nb B - 1) - m_x^T m_y.
The reference whitens both sides by eigen-decomposition and takes svd(K11 C_xy K22); the sweep's route
(Z = C_xx^-1 C_xy by Cholesky, K = C_yy^-1/2, B = K C_xy^T Z K = V sigma^2 V^T, rot_y = K V, rot_x = Z K V / sigma) gives the
same model when no eigenvalue of C_xx is dropped, i.e. when the Cholesky factor exists.

Fallback (existing calls only): a (fold, lambda) pair the device call marks (no Cholesky factor, an eigenvalue of
C_yy dropped, a vanishing canonical correlation), or the whole sweep when input_2 is wider than 64 lagged columns or a
fold needs more than four terms, sums the fold's statistics (combine), solves with LagStats.cca_solve, projects with
cca_transform and scores like BrainModelCCA.evaluate.

One rank only: the multi-rank CCA sweep is out of scope.
"""
import collections

import numpy as np

from telluride_decoding_amd import device as _device

MAX_K2 = 64          # lagged columns of input_2 the batched dense stage holds (td_cca_solve_loso_terms)
MAX_TERMS = 4        # signed terms per fold


def sweep(dataset, lambdas, cca_dims=5, device=None, folds=None, route=None, eps_eig=1e-12):
  """The [Lambda, F] matrix of held-out cca_pearson_correlation_first and how it was computed.

  dataset: brain_data.Dataset whose files are the jackknife units; lambdas: the regularisation values; folds: the
  held-out files to run (default: all).  route: None (the batched dense stage, the fallback where it is needed) or
  'per_fold' (the fallback everywhere: what the calls that predate the sweep can do).  Returns (results, info):
  results = OrderedDict {lambda: (mean, std)} plus 'all_runs' [Lambda, F]; info = {'cca_route': 'batched' | 'per_fold'
  | 'batched+per_fold', 'cca_pairs': {'batched': n, 'per_fold': m}}.
  """
  dev = device or _device
  if route not in (None, 'per_fold'):
    raise ValueError('route must be None or \'per_fold\', not %r' % (route,))
  if getattr(dataset, 'mixup_batch', False):
    raise ValueError('The CCA sweep needs statistics that add up per file: a mixup_batch dataset shuffles input_2 '
                     'inside the minibatches of the whole stream.')
  if dataset.c2 == 0:
    raise ValueError('Second input to CCA estimator must have more than 0 columns.')
  keys = list(lambdas)                                   # (the results are keyed by the caller's values)
  lambdas = [float(v) for v in keys]
  if any(v < 0.0 for v in lambdas):
    raise ValueError('regularization lambda must be >= 0')
  n_files = len(dataset.files)
  if n_files < 2:
    raise ValueError('Need at least two files for a jackknife test.')
  fold_list = list(range(n_files)) if folds is None else sorted(set(int(f) for f in folds))
  if not fold_list or fold_list[0] < 0 or fold_list[-1] >= n_files:
    raise ValueError('folds must name files of the dataset (0..%d), not %s' % (n_files - 1, folds))
  h = dev.default_handle()
  off, bsz = dataset.input_offset, dataset.batch_size
  dy = max(-off, 0)
  lengths = dataset.file_lengths()
  zipped = dataset.zipped_lengths()                      # frames a file contributes to a stream
  held_used = [(n // bsz) * bsz for n in zipped]         # a held-out file is its own stream
  total_zipped = sum(zipped)
  n_lam = len(lambdas)
  x_all, x2_all, _, offs = dataset.device_arrays(h)
  offs = [int(v) for v in offs]

  def file_arrays(i):
    return x_all[offs[i]:offs[i + 1]], x2_all[offs[i]:offs[i + 1]]

  def new_stats():
    return dev.LagStats(dataset.c1, dataset.pre, dataset.post, dataset.c2, dataset.pre2, dataset.post2, 0, handle=h)

  def file_stats(i, rows):
    st = new_stats()
    x, x2 = file_arrays(i)
    st.accumulate(x, x2, None, [0, lengths[i]], input_offset=off, rows_used=[rows])
    return st

  # 1. every recording once
  stats = [file_stats(i, zipped[i]) for i in range(n_files)]
  k1, k2 = stats[0].k1, stats[0].k2
  dim = max(1, min(int(cca_dims), k1, k2))               # (u[:, 0:dim] of the reference slices to what exists)
  truncated = {}                                         # (file, frames dropped from its end) -> statistics

  def cut_stats(g, cut):
    if (g, cut) not in truncated:
      truncated[(g, cut)] = file_stats(g, zipped[g] - cut)
    return truncated[(g, cut)]

  def fold_batches(f):
    return (total_zipped - zipped[f]) // bsz

  def fold_cuts(f):
    """[(recording, frames dropped from its end)] of fold f: batching drops the remainder of the training stream from
    the end of its last recordings (normally just the last one)."""
    members = [g for g in range(n_files) if g != f]
    rem = (total_zipped - zipped[f]) % bsz
    cuts = []
    g = len(members) - 1
    while rem > 0 and g >= 0:
      cut = min(rem, zipped[members[g]])
      cuts.append((members[g], cut))
      rem -= cut
      g -= 1
    return cuts

  def fold_terms(f):
    """Fold f's training statistics as signed terms of the total of ALL recordings."""
    terms = [(stats[f], -1.0)]
    for g, cut in fold_cuts(f):
      terms.append((stats[g], -1.0))
      if cut < zipped[g]:
        terms.append((cut_stats(g, cut), 1.0))
    return terms

  def fold_sum(f):
    """The same as one summed statistics object (the fallback's)."""
    cuts = dict(fold_cuts(f))
    parts = []
    for g in range(n_files):
      if g == f:
        continue
      if g not in cuts:
        parts.append(stats[g])
      elif cuts[g] < zipped[g]:
        parts.append(cut_stats(g, cuts[g]))
    return new_stats().combine(parts)

  def minibatch_scores(a, b, u, group):
    """[minibatches, columns / group]: Pearson's r of column 0 of every group of `group` columns of a against b over
    the windows of bsz frames, with the zero rule over the group."""
    sums = dev.window_sums(a[:u], b[:u], [0, u], bsz, bsz, handle=h)
    return dev.window_scores(sums, bsz, mode=1, handle=h, group=group)[:, ::group]

  all_runs = np.full((n_lam, len(fold_list)), np.nan)
  counts = {'batched': 0, 'per_fold': 0}

  def refit(fi, f, lam_indices, train=None):
    """The fallback for the pairs (f, lambdas[li]): existing calls only."""
    u = held_used[f]
    if u == 0 or not lam_indices:
      return
    if fold_batches(f) < 1:
      raise ValueError('No minibatches in dataset, can\'t compute CCA model.')
    train = train or fold_sum(f)
    xf, x2f = file_arrays(f)
    for li in lam_indices:
      rot_x, rot_y, mean_x, mean_y = train.cca_solve(fold_batches(f) * bsz - 1, lambdas[li], dim, eps_eig, handle=h)[:4]
      z = dev.cca_transform(xf, x2f, [0, lengths[f]], mean_x, rot_x, mean_y, rot_y, dataset.pre, dataset.post,
                            dataset.pre2, dataset.post2, handle=h, input_offset=off)
      r = minibatch_scores(z[:, :dim].contiguous(), z[:, dim:].contiguous(), u, dim)
      all_runs[li, fi] = float(np.mean(np.asarray(r.cpu(), np.float64)[:, 0]))
      counts['per_fold'] += 1

  all_terms = None
  if route is None and k2 <= MAX_K2 and all(fold_batches(f) >= 1 for f in fold_list):
    all_terms = [fold_terms(f) for f in fold_list]
    if any(len(t) > MAX_TERMS for t in all_terms):
      all_terms = None
  if all_terms is None:
    for fi, f in enumerate(fold_list):
      refit(fi, f, list(range(n_lam)))
  else:
    # 2-3. every (fold, lambda) dense stage in batches on the device
    total = new_stats().combine(stats)
    out = dev.LagStats.cca_solve_loso_terms(total, all_terms, [fold_batches(f) for f in fold_list], bsz, lambdas, dim,
                                            eps_eig, handle=h)
    rot_x, rot_y, _, _, bias_x, bias_y, _, status = out
    # 4. a fold's held-out recording under all of the fold's models: two FIR predictions, one window-sums launch
    scores = []
    for fi, f in enumerate(fold_list):
      u = held_used[f]
      if u == 0:
        scores.append(None)
        continue
      xf, x2f = file_arrays(f)
      a = dev.predict_fir(xf, [0, lengths[f]], rot_x[fi], bias_x[fi], dataset.pre, dataset.post, handle=h,
                          input_offset=off)
      x2s = x2f[dy:] if dy else x2f
      b = dev.predict_fir(x2s, [0, int(x2s.shape[0])], rot_y[fi], bias_y[fi], dataset.pre2, dataset.post2, handle=h)
      scores.append(minibatch_scores(a, b, u, dim))          # [minibatches, Lambda], kept on the device
    st = np.asarray(status.cpu()).reshape(len(fold_list), n_lam)
    for fi, f in enumerate(fold_list):
      if scores[fi] is None:
        continue
      all_runs[:, fi] = np.asarray(scores[fi].cpu(), np.float64).mean(axis=0)
      bad = [li for li in range(n_lam) if st[fi, li] != 0]
      counts['batched'] += n_lam - len(bad)
      all_runs[bad, fi] = np.nan
      refit(fi, f, bad)
  results = collections.OrderedDict()
  for li, lam in enumerate(keys):
    results[lam] = (float(np.mean(all_runs[li])), float(np.std(all_runs[li])))
  results['all_runs'] = all_runs
  used = [name for name in ('batched', 'per_fold') if counts[name]]
  info = {'cca_route': '+'.join(used) if used else ('per_fold' if all_terms is None else 'batched'),
          'cca_pairs': dict(counts)}
  return results, info
