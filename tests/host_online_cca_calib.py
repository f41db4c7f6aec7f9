"""Shared by the online CCA calibration tests (CPU and GPU): labelled stretches with a separable attended class, bare
float32 projections for the closed form's sweep, the frame-order NumPy twin of td_ccacalib_online_push's sums, the
closed form td_ccacalib_online_finish evaluates, and the two-pass float64 route of infer_decoder.Decoder.train with a
CCADecoder restated from the oracle (one Correlator fed class 0 then class 1, average_data, scaled_lda_fit,
calculate_dprime).  The cuts and the walk of a cut are tests/host_online_calib's.  Everything is computed once per key
and shared: treat what these functions return as read-only."""
import numpy as np

from oracle import correlator as o_cor
from oracle import lda as o_lda
from tests import host_online_calib as hoc
from tests import host_online_cca as hcc

SEED = 40127
WIDTHS = (1, 2, 7, 100)
cuts = hoc.cuts
run = hoc.run

_STRETCHES = {}
_PROJECTIONS = {}


def sums_count(dims):
  return 9 * dims * dims + 20 * dims


def host_proj(rows, c, pre, post, mean, rot):
  """The float64 projection (x~ - mean) @ rot of every frame of a whole stretch, zero rows before and behind it, summed
  in (lag, channel) order as online._HostCcaSession sums it (so: the host calibration session's projection, bit for
  bit).  rows [frames, c]; mean [k], rot [k, dims] float32."""
  frames = rows.shape[0]
  padded = np.concatenate([np.zeros((pre, c)), np.asarray(rows, np.float64), np.zeros((post, c))])
  mean, rot = np.asarray(mean, np.float32).astype(np.float64), np.asarray(rot, np.float32).astype(np.float64)
  out = np.zeros((frames, rot.shape[1]), np.float64)
  for l in range(pre + 1 + post):
    for ch in range(c):
      k = l * c + ch
      out += (padded[l:l + frames, ch] - mean[k])[:, None] * rot[k][None, :]
  return out


def stretch(view1, view2, dims, frames, seed=0):
  """dict(eeg [frames, c1], att and unatt [frames, c2] float32, mean_x, rot_x, mean_y, rot_y float32 (rounded), a, b1,
  b0 [frames, dims] float64 host projections): white-noise EEG with an offset, seeded rotations of unit output scale
  -- the feature rotation led by the current frame's lag --, an attended feature block that carries the EEG view's
  projection into that lag (through the pseudo-inverse of the lag's rotation block) under its own noise, and an
  unattended block that does not.  The attended class is separable: at W = 7 the classes' window means along the
  two-pass LDA axis differ by at least one pooled standard deviation (asserted here, in float64, wherever the stretch
  has 2 dims windows of 7 per class)."""
  key = (tuple(view1), tuple(view2), dims, frames, seed)
  if key not in _STRETCHES:
    (c1, pre1, post1), (c2, pre2, post2) = view1, view2
    rng = np.random.default_rng(SEED + 7919 * seed + 131 * c1 + 17 * c2 + dims)
    k1, k2 = (pre1 + 1 + post1) * c1, (pre2 + 1 + post2) * c2
    rot_x = (rng.standard_normal((k1, dims)) / np.sqrt(k1)).astype(np.float32)
    lag_gain = np.where(np.arange(k2) // c2 == pre2, 2.0, 0.3)[:, None]   # the current frame's lag leads the others
    rot_y = (lag_gain * rng.standard_normal((k2, dims)) / np.sqrt(k2)).astype(np.float32)
    mean_x = (0.1 * rng.standard_normal((k1,))).astype(np.float32)
    mean_y = (0.1 * rng.standard_normal((k2,))).astype(np.float32)
    eeg = (rng.standard_normal((frames, c1)) + 0.2).astype(np.float32)
    a = host_proj(eeg, c1, pre1, post1, mean_x, rot_x)
    now = rot_y[pre2 * c2:(pre2 + 1) * c2].astype(np.float64)          # [c2, dims]: the current frame's lag
    carry = (a - a.mean(axis=0)) @ np.linalg.pinv(now)
    att = (carry + 0.1 * np.sqrt(k2) / np.sqrt(c2) * rng.standard_normal((frames, c2)) + 0.1).astype(np.float32)
    unatt = (np.std(att) * rng.standard_normal((frames, c2)) + 0.05).astype(np.float32)
    b1 = host_proj(att, c2, pre2, post2, mean_y, rot_y)
    b0 = host_proj(unatt, c2, pre2, post2, mean_y, rot_y)
    for v in (eeg, att, unatt, mean_x, rot_x, mean_y, rot_y, a, b1, b0):
      v.setflags(write=False)
    if frames // 7 >= 2 * dims:
      assert two_pass(a, b1, b0, 7)['dprime'] >= 1.0, key
    _STRETCHES[key] = dict(view1=tuple(view1), view2=tuple(view2), dims=dims, frames=frames, eeg=eeg, att=att,
                           unatt=unatt, mean_x=mean_x, rot_x=rot_x, mean_y=mean_y, rot_y=rot_y, a=a, b1=b1, b0=b0)
  return _STRETCHES[key]


def projections(dims, frames, seed=0):
  """(a, b1, b0) [frames, dims] float32: bare white-noise projections, means between 0 and 1 standard deviation, the
  attended one correlated with a column by column."""
  key = (dims, frames, seed)
  if key not in _PROJECTIONS:
    rng = np.random.default_rng(SEED + 104729 * seed + dims)
    a = (rng.standard_normal((frames, dims)) + rng.uniform(0.0, 1.0, dims)).astype(np.float32)
    b1 = (0.6 * (a - a.mean(axis=0)) + 0.8 * rng.standard_normal((frames, dims)) +
          rng.uniform(0.0, 1.0, dims)).astype(np.float32)
    b0 = (rng.standard_normal((frames, dims)) + rng.uniform(0.0, 1.0, dims)).astype(np.float32)
    for v in (a, b1, b0):
      v.setflags(write=False)
    _PROJECTIONS[key] = (a, b1, b0)
  return _PROJECTIONS[key]


def decoder_of(st, reduction='first', lda=None, stats=None):
  """An infer_decoder.CCADecoder around the stretch's model."""
  dims = st['dims']
  stats = np.stack([np.full(dims, 0.1), np.full(dims, -0.2), np.full(dims, 0.9)]) if stats is None else stats
  return hcc.cca_decoder(st['view1'], st['view2'], st['mean_x'], st['rot_x'], st['mean_y'], st['rot_y'], stats,
                         reduction, lda)


def twin_sums(a, b1, b0, width):
  """The 9 D^2 + 20 D float64 sums after the frames given, in td_ccacalib_online_sums' order, by the frame-order walk:
  every accumulator takes acc += float64(x) * float64(y) per frame; a frame that completes a window adds the window's
  z = (sum a b | sum a | sum b) to each class's sum z, np.outer(z, z) to its Gram (upper triangle kept), and clears
  the open window."""
  a, b1, b0 = (np.asarray(v).astype(np.float64) for v in (a, b1, b0))
  d = a.shape[1]
  corr = np.zeros((6, d), np.float64)                # sum a, a^2, b1, b1^2, b0, b0^2
  zsum = np.zeros((2, 3 * d), np.float64)
  gram = np.zeros((2, 3 * d, 3 * d), np.float64)
  win = np.zeros((5, d), np.float64)                 # sum a, b1, a b1, b0, a b0
  for t in range(a.shape[0]):
    x, y1, y0 = a[t], b1[t], b0[t]
    corr += np.stack([x, x * x, y1, y1 * y1, y0, y0 * y0])
    win += np.stack([x, y1, x * y1, y0, x * y0])
    if (t + 1) % width == 0:
      for cls, z in ((0, np.concatenate([win[4], win[0], win[3]])), (1, np.concatenate([win[2], win[0], win[1]]))):
        zsum[cls] = zsum[cls] + z
        gram[cls] = gram[cls] + np.outer(z, z)
      win[:] = 0.0
  upper = np.triu_indices(3 * d)
  return np.concatenate([corr.reshape(-1), zsum[0], gram[0][upper], zsum[1], gram[1][upper], win.reshape(-1)])


def closed_form(sums, frames, width, dims):
  """dict(corr [3, D] (mean_a, mean_b, power), axis [D] = slope w, intercept, dprime) from the sums after `frames`
  frames: the issue's closed form, written out with dense matrices."""
  q = np.asarray(sums, np.float64)
  d = dims
  count = 2.0 * frames
  s = q[:6 * d].reshape(6, d)
  sum_x, sum_x2, sum_y, sum_y2 = 2.0 * s[0], 2.0 * s[1], s[4] + s[2], s[5] + s[3]
  mean_a, mean_b = sum_x / count, sum_y / count
  power = np.sqrt((sum_x2 - sum_x ** 2 / count) * (sum_y2 - sum_y ** 2 / count)) / count
  n_win = frames // width
  eye = np.eye(d)
  c = np.concatenate([eye, -np.diag(mean_b), -np.diag(mean_a)], axis=1) / (width * power)[:, None]
  c0 = mean_a * mean_b / power
  per_class = 3 * d + 3 * d * (3 * d + 1) // 2
  upper = np.triu_indices(3 * d)
  means, scatters = [], []
  for cls in (0, 1):
    base = 6 * d + cls * per_class
    g = np.zeros((3 * d, 3 * d))
    g[upper] = q[base + 3 * d:base + per_class]
    g = g + np.triu(g, 1).T
    cz = c @ q[base:base + 3 * d]
    sm = cz + n_win * c0
    smm = c @ g @ c.T + np.outer(cz, c0) + np.outer(c0, cz) + n_win * np.outer(c0, c0)
    mu = sm / n_win
    means.append(mu)
    scatters.append(smm - n_win * np.outer(mu, mu))
  delta = means[1] - means[0]
  factor = np.linalg.cholesky(scatters[0] + scatters[1])
  v = np.linalg.solve(factor.T, np.linalg.solve(factor, delta))
  w = np.ones(1) if d == 1 else v / np.linalg.norm(v)
  slope = 1.0 / (delta @ w)
  return dict(corr=np.stack([mean_a, mean_b, power]), axis=slope * w, intercept=-slope * (means[0] @ w),
              dprime=abs(delta @ w) / np.sqrt((w @ scatters[0] @ w + w @ scatters[1] @ w) / (2.0 * n_win)))


def two_pass(a, b1, b0, width):
  """Decoder.train(data0 = (a, b0), data1 = (a, b1), window_size = width) with a CCADecoder, in float64 from the
  oracle: one Correlator fed class 0 then class 1, the per-frame correlations with its FINAL statistics, average_data,
  the scaled LDA between the classes, d' of the projections.  The same dict as closed_form (axis = slope w: the
  eigenvector's sign is arbitrary, the product is not)."""
  a, b1, b0 = (np.asarray(v).astype(np.float64) for v in (a, b1, b0))
  cor = o_cor.Correlator()
  cor.add(a, b0)
  cor.add(a, b1)
  d0 = o_cor.average_data(cor.correlate(a, b0), width)
  d1 = o_cor.average_data(cor.correlate(a, b1), width)
  data = np.concatenate([d0, d1])
  labels = np.concatenate([np.ones(d0.shape[0]), 2 * np.ones(d1.shape[0])])
  w, _, _, slope, intercept = o_lda.scaled_lda_fit(data, labels)
  proj = o_lda.scaled_lda_transform(data, w, slope, intercept)
  dprime = o_cor.calculate_dprime(proj[labels == 1, 0], proj[labels == 2, 0])
  return dict(corr=np.stack([cor.mean_x, cor.mean_y, cor.power]), axis=np.real(slope * w[:, 0]),
              intercept=float(np.real(intercept)), dprime=float(dprime))


def distances(got, want):
  """(the largest relative error over the statistics, slope w -- relative to its largest entry -- and the intercept;
  the relative error of d')."""
  ga, wa = np.asarray(got['axis'], np.float64), np.asarray(want['axis'], np.float64)
  errs = [np.max(np.abs(np.asarray(got['corr']) - want['corr']) / np.abs(want['corr'])),
          np.max(np.abs(ga - wa)) / np.max(np.abs(wa)),
          abs(got['intercept'] - want['intercept']) / abs(want['intercept'])]
  return float(max(errs)), float(abs(got['dprime'] - want['dprime']) / abs(want['dprime']))


def result_of(corr, lda, dprime):
  """finish's (corr [2, 3, D], lda [D + 2], dprime) of one session as closed_form's dict."""
  corr, lda = np.asarray(corr, np.float64), np.asarray(lda, np.float64)
  return dict(corr=corr[0], axis=lda[-2] * lda[:-2], intercept=float(lda[-1]), dprime=float(dprime))
