"""Shared by tests/test_cpu_online.py and tests/test_gpu_online.py: a brute-force count of what a push emits,
the seeded recording and model of the online decoder's oracle comparisons, the oracle chain itself, and
decoders built around given weights without a dataset.  Test infrastructure."""
import numpy as np

from oracle import attention as o_att
from oracle import correlator as o_cor
from oracle import lag as o_lag
from oracle import regression as o_reg

FRAMES = 1500
SWITCH = 750
SEED = 2501


def brute_plan(frames_before, n, post, width, hop, flush):
  """(emitted_before, emitted_after, first_window, new_windows) by counting: a frame is emitted once `post`
  later rows are there (or the recording has ended), a window once its last frame is."""
  def emitted(pushed, ended):
    return sum(1 for t in range(pushed) if ended or t + post < pushed)

  def windows(frames):
    count, start = 0, 0
    while start + width <= frames:
      count, start = count + 1, start + hop
    return count
  before = emitted(frames_before, False)
  after = emitted(frames_before + n, bool(flush))
  return before, after, windows(before), windows(after) - windows(before)


_RECIPES = {}


def recipe(c, pre, post):
  """The recording and model of the oracle comparisons: rng 2501, synth.impulse_responses, one synth.trial
  of 1500 frames whose attention switches to speaker 2 at frame 750, weights from
  oracle.regression.linear_regressor_from_batches on the float64 lag matrix against the attended envelope
  (lamb 0.1) rounded to float32, one Correlator fed both speakers' (envelope, prediction) pairs.  Computed
  once per shape and shared: treat as read-only."""
  key = (c, pre, post)
  if key not in _RECIPES:
    from telluride_decoding_amd import synth
    rng = np.random.default_rng(SEED)
    h_att, h_unatt = synth.impulse_responses(rng, c)
    att = np.zeros((FRAMES,), np.float32)
    att[SWITCH:] = 1.0
    eeg, env, att = synth.trial(rng, FRAMES, c, h_att, h_unatt, att)
    xl = o_lag.lag_matrix(eeg.astype(np.float64), pre, post)
    attended = np.where(att > 0.5, env[:, 1:2], env[:, 0:1]).astype(np.float64)
    w, b = o_reg.linear_regressor_from_batches([({'input_1': xl}, attended)], lamb=0.1)[:2]
    w, b = np.asarray(w, np.float32).reshape(-1), np.float32(np.reshape(b, -1)[0])
    pred = o_reg.dense_forward(xl, w.astype(np.float64).reshape(-1, 1), np.float64(b))
    cor = o_cor.Correlator()
    for spk in (0, 1):
      cor.add(env[:, spk:spk + 1].astype(np.float64), pred)
    stats = [float(cor.mean_x[0]), float(cor.mean_y[0]), float(cor.power[0])]
    _RECIPES[key] = dict(c=c, pre=pre, post=post, eeg=eeg, env=env, att=att, w=w, b=b, xl=xl, pred64=pred,
                         cor=cor, corr=np.array([stats, stats], np.float64))
  return _RECIPES[key]


def oracle_chain(rec, width, hop, reduction='first', lda=None):
  """lag_matrix -> dense_forward -> Correlator.correlate -> reduction -> windowed_means -> wta_sequence /
  step_sequence, all float64: (scores [windows, 2], wta decisions, stepped decisions)."""
  lda_map = None if lda is None else (lambda c: lda[1] * (c * lda[0]) + lda[2])
  scores = []
  for spk in (0, 1):
    cols = rec['cor'].correlate(rec['env'][:, spk:spk + 1].astype(np.float64), rec['pred64'])
    reduced = o_cor.reduce_correlations(cols, reduction, lda_map)
    scores.append(o_cor.windowed_means(reduced, rec['att'], width, hop)[0])
  scores = np.stack(scores, axis=1).reshape(-1, 2)
  return (scores, o_att.wta_sequence(scores[:, 0], scores[:, 1]),
          o_att.step_sequence(scores[:, 0], scores[:, 1])[0])


def chunkings(total, pre, post, width, seed=0):
  """The cuts of a recording the chunk-invariance tests walk: {name: list of push sizes summing to total}."""
  rng = np.random.default_rng(seed)

  def fill(size, frames=total):
    size = max(1, size)
    return [size] * (frames // size) + ([frames % size] if frames % size else [])
  random = []
  while sum(random) < total:
    random.append(int(min(rng.integers(0, 301) * (rng.random() > 0.2), total - sum(random))))
  random.insert(1, 0)
  first = min(width + 1, total)
  return {'ones': fill(1), 'sevens': fill(7), 'tail-1': fill(pre + post - 1),
          'width+1': [first] + fill(13, total - first), 'random': random, 'whole': [total]}


def linear_decoder(c, pre, post, w, b, stats, reduction='first', lda=None):
  """An infer_decoder.LinearRegressionDecoder around a BrainModelLinearRegression with the given weights
  [lags c] and bias, the trained statistics stats = (mean_truth, mean_pred, power) and, for reduction 'lda',
  lda = (lda_w, slope, intercept) -- built without a dataset and without a device."""
  from telluride_decoding_amd import brain_model, infer_decoder, scaled_lda
  model = brain_model.BrainModelLinearRegression(brain_model._shape_dataset(c, 1, 1, pre, post))
  model.set_weights([np.asarray(w, np.float32).reshape(-1, 1), np.asarray([b], np.float32)])
  decoder = infer_decoder.LinearRegressionDecoder(model, reduction=reduction)
  decoder._set_correlation_params((1, 0.0, 0.0, 0.0, 0.0, np.array([stats[0]]), np.array([stats[1]]),
                                   np.array([stats[2]])))
  if lda is not None:
    decoder._lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    decoder._lda._w = np.array([[float(lda[0])]])
    decoder._lda._slope, decoder._lda._intercept = float(lda[1]), float(lda[2])
  return decoder
