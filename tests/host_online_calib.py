"""Shared by the online calibration tests (CPU and GPU): labelled white-noise stretches, the cuts of a stretch into
pushes, the frame-order NumPy twin of td_calib_online_push's sums, the closed form td_calib_online_finish evaluates,
and the two-pass float64 route of infer_decoder.Decoder.train restated from the oracle (Correlator, average_data,
scaled_lda_fit, calculate_dprime).  Everything is computed once per key and shared: treat what these functions return
as read-only."""
import numpy as np

from oracle import correlator as o_cor
from oracle import lda as o_lda

SEED = 9176
SUMS = 29
WIDTHS = (1, 2, 7, 100)

_STRETCHES = {}


def stretch(c, pre, post, frames, seed=0, offset=0.0):
  """dict(eeg [frames, c], att [frames], unatt [frames] float32, w [lags c] float32, b float32): white-noise EEG, a
  random model, an attended envelope that follows the model's prediction and an unattended one that does not; both
  envelopes and the prediction have a mean of `offset` standard deviations (about: the streams have unit scale)."""
  key = (c, pre, post, frames, seed, offset)
  if key not in _STRETCHES:
    rng = np.random.default_rng(SEED + 7919 * seed + 31 * c + 5 * pre + post)
    k = (pre + 1 + post) * c
    eeg = rng.standard_normal((frames, c)).astype(np.float32)
    w = (rng.standard_normal((k,)) / np.sqrt(k)).astype(np.float32)
    b = np.float32(offset + 0.25)
    pred = host_pred(eeg, w, b, pre, post)
    att = (0.6 * (pred - float(b)) + 0.8 * rng.standard_normal((frames,)) + offset).astype(np.float32)
    unatt = (rng.standard_normal((frames,)) + 0.5 * offset).astype(np.float32)
    for a in (eeg, w, att, unatt):
      a.setflags(write=False)
    _STRETCHES[key] = dict(eeg=eeg, att=att, unatt=unatt, w=w, b=b, c=c, pre=pre, post=post, frames=frames)
  return _STRETCHES[key]


def host_pred(eeg, w, b, pre, post):
  """The float64 prediction of every frame of a whole stretch, zero rows before and behind it, summed in (lag, channel)
  order as online._HostSession sums it (so: the host calibration session's prediction, bit for bit)."""
  frames, c = eeg.shape
  rows = np.concatenate([np.zeros((pre, c)), np.asarray(eeg, np.float64), np.zeros((post, c))])
  w = np.asarray(w, np.float32).astype(np.float64)
  pred = np.zeros((frames,), np.float64)
  for l in range(pre + 1 + post):
    for ch in range(c):
      pred += rows[l:l + frames, ch] * w[l * c + ch]
  return pred + float(b)


def twin_sums(pred, att, unatt, width):
  """The 29 float64 sums after the frames given, in td_calib_online_sums' order, by the frame-order walk: every
  accumulator takes acc += float64(x) * float64(p) per frame; a frame that completes a window adds the window's
  z = (sum x p, sum x, sum p) to each class's sum z, np.outer(z, z) to its Gram (upper triangle kept), and clears the
  open window."""
  pred, att, unatt = (np.asarray(v).astype(np.float64) for v in (pred, att, unatt))
  corr = np.zeros((6,), np.float64)                  # sum p, p^2, a, a^2, u, u^2
  zsum = np.zeros((2, 3), np.float64)
  gram = np.zeros((2, 3, 3), np.float64)
  win = np.zeros((5,), np.float64)                   # sum p, a, a p, u, u p
  for t in range(pred.shape[0]):
    p, a, u = pred[t], att[t], unatt[t]
    corr += np.array([p, p * p, a, a * a, u, u * u])
    win += np.array([p, a, a * p, u, u * p])
    if (t + 1) % width == 0:
      for cls, z in ((0, np.array([win[4], win[3], win[0]])), (1, np.array([win[2], win[1], win[0]]))):
        zsum[cls] = zsum[cls] + z
        gram[cls] = gram[cls] + np.outer(z, z)
      win[:] = 0.0
  upper = np.triu_indices(3)
  return np.concatenate([corr, zsum[0], gram[0][upper], zsum[1], gram[1][upper], win])


def closed_form(sums, frames, width):
  """dict(corr (mean_x, mean_y, power), lda (1, slope, intercept), dprime) from the sums after `frames` frames: the
  issue's closed form, written out from the 3 x 3 Grams."""
  q = np.asarray(sums, np.float64)
  count = 2.0 * frames
  sum_x, sum_x2, sum_y, sum_y2 = q[4] + q[2], q[5] + q[3], q[0] + q[0], q[1] + q[1]
  mean_x, mean_y = sum_x / count, sum_y / count
  power = np.sqrt((sum_x2 - sum_x ** 2 / count) * (sum_y2 - sum_y ** 2 / count)) / count
  n_win = frames // width
  cv = np.array([1.0, -mean_y, -mean_x]) / (width * power)
  c0 = mean_x * mean_y / power
  upper = np.triu_indices(3)
  means, variances = [], []
  for base in (6, 15):
    z = q[base:base + 3]
    g = np.zeros((3, 3))
    g[upper] = q[base + 3:base + 9]
    g = g + np.triu(g, 1).T
    sm = cv @ z + n_win * c0
    sm2 = cv @ g @ cv + 2.0 * c0 * (cv @ z) + n_win * c0 * c0
    means.append(sm / n_win)
    variances.append(sm2 / n_win - means[-1] ** 2)
  slope = 1.0 / (means[1] - means[0])
  return dict(corr=(mean_x, mean_y, power), lda=(1.0, slope, -slope * means[0]),
              dprime=abs(means[1] - means[0]) / np.sqrt((variances[0] + variances[1]) / 2.0))


def two_pass(pred, att, unatt, width):
  """Decoder.train(data0 = (unatt, pred), data1 = (att, pred), window_size = width) in float64 from the oracle: one
  Correlator fed class 0 then class 1, the per-frame correlations with its FINAL statistics, average_data, the scaled
  LDA between the classes, d' of the projections.  The same dict as closed_form."""
  col = lambda v: np.asarray(v).astype(np.float64).reshape(-1, 1)
  pred, att, unatt = col(pred), col(att), col(unatt)
  cor = o_cor.Correlator()
  cor.add(unatt, pred)
  cor.add(att, pred)
  d0 = o_cor.average_data(cor.correlate(unatt, pred), width)
  d1 = o_cor.average_data(cor.correlate(att, pred), width)
  data = np.concatenate([d0, d1])
  labels = np.concatenate([np.ones(d0.shape[0]), 2 * np.ones(d1.shape[0])])
  w, _, _, slope, intercept = o_lda.scaled_lda_fit(data, labels)
  proj = o_lda.scaled_lda_transform(data, w, slope, intercept)
  dprime = o_cor.calculate_dprime(proj[labels == 1, 0], proj[labels == 2, 0])
  return dict(corr=(float(cor.mean_x[0]), float(cor.mean_y[0]), float(cor.power[0])),
              lda=(float(np.real(w[0, 0])), float(slope), float(intercept)), dprime=float(dprime))


def distances(got, want):
  """(the largest relative error over corr and lda, the relative error of d')."""
  a = np.array(list(got['corr']) + list(got['lda']), np.float64)
  b = np.array(list(want['corr']) + list(want['lda']), np.float64)
  return float(np.max(np.abs(a - b) / np.abs(b))), float(abs(got['dprime'] - want['dprime']) / abs(want['dprime']))


def cuts(frames, width, seed=0):
  """{name: list of push sizes summing to frames}: ones, width - 1, width, width + 1, random 0 .. 40, whole, and two
  halves with an empty push between them."""
  rng = np.random.default_rng(SEED + seed)

  def fill(size):
    size = max(1, size)
    return [size] * (frames // size) + ([frames % size] if frames % size else [])

  random = []
  while sum(random) < frames:
    random.append(int(min(rng.integers(0, 41), frames - sum(random))))
  half = frames // 2
  return {'ones': fill(1), 'width-1': fill(width - 1), 'width': fill(width), 'width+1': fill(width + 1),
          'random': random, 'whole': [frames], 'empty-middle': [half, 0, frames - half]}


def run(calib, eeg, att, unatt, sizes, flush_last=False, convert=None, after_push=None):
  """Walks one cut of a stretch (eeg [frames, c] / [S, frames, c] with its envelopes) through `calib` from a reset:
  every push in turn, then the flush on its own (an empty flushing push) -- or, flush_last, the last piece carried by
  the flush itself (a flushing last push).  convert: what turns a host piece into what push takes; after_push(rows
  pushed so far): called behind every push that is not the flush.  Returns the frames counted."""
  calib.reset()
  convert = convert or (lambda a: a)
  banked = len(eeg.shape) == 3
  at = 0
  for i, n in enumerate(sizes):
    pieces = [convert(a[:, at:at + n] if banked else a[at:at + n]) for a in (eeg, att, unatt)]
    at += n
    if flush_last and i == len(sizes) - 1:
      frames = calib.flush(*pieces)
      assert frames == at == calib.frames_emitted
      return frames
    got = calib.push(*pieces)
    assert got == max(0, at - calib.delay) == calib.frames_emitted
    if after_push:
      after_push(at)
  frames = calib.flush()
  assert frames == at == calib.frames_emitted
  return frames
