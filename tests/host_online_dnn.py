"""Shared by tests/test_cpu_online_dnn.py and tests/test_gpu_online_dnn.py: the shapes of the online DNN decoder's
tests, models on the recordings of tests/host_online.py (1500 frames), the recipe of the oracle comparisons and
decoders built around given weights without a dataset.  Test infrastructure."""
import numpy as np

from oracle import correlator as o_cor
from oracle import lag as o_lag
from tests import host_dnn
from tests import host_online

FRAMES = host_online.FRAMES
# (c, pre, post), hidden: what each exercises is K = c (pre + 1 + post), the rows per slice of W1
# ks = min(64, round_up(ceil(K / 64), 4)) and the slices ceil(K / ks)
SHAPES = [((5, 2, 9), [16]),                  # K 60: ks 4, 15 slices
          ((64, 0, 31), [33, 7]),             # K 2048: ks 32, 64 slices; w1 33 is not a multiple of 4
          ((63, 40, 5), [64, 64, 64, 64]),    # K 2898: ks 48, 61 slices, the last of 18 rows; the largest head
          ((128, 31, 32), [64]),              # K 8192: ks 64, 128 slices; the 2 MB W1
          ((3, 31, 32), [5]),                 # 64 lags
          ((5, 2, 9), []),                    # no hidden layer: w1 = d = 1, no ReLU
          ((1, 0, 0), [63, 1, 63])]           # K 1, no tails, a one-unit layer
WINDOWS = [(100, 50), (10, 5), (37, 11), (1, 1), (5, 9)]
LDA = (1.7, -0.8, 0.25)


def slices_of(k):
  """(rows per slice, slices) of a W1 of k rows: mlp_check_and_plan's rule."""
  ks = min(64, -(-(-(-k // 64)) // 4) * 4)
  return ks, -(-k // ks)


def packed(weights):
  """[W1, b1, W2, b2, ...] as the packed float32 vector td_mlp_* reads."""
  return np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in weights])


def glorot_model(c, pre, post, hidden, seed=5):
  """host_dnn.glorot weights on c (pre + 1 + post) inputs and one output; the biases, which glorot leaves at zero,
  are 0.01 N(0, 1) so that every `+ b` of the contract changes bits."""
  ws = host_dnn.glorot([c * (pre + 1 + post)] + list(hidden) + [1], seed)
  rng = np.random.default_rng(seed + 1000)
  for i in range(1, len(ws), 2):
    ws[i] = (0.01 * rng.standard_normal(ws[i].shape)).astype(np.float32)
  return ws


def trained_statistics(rec, weights):
  """(float64 predictions [frames, 1], Correlator, corr [2, 3]) of a model on a host_online.recipe: one Correlator
  fed both speakers' (envelope, prediction) pairs, as the linear recipe's."""
  pred = host_dnn.forward(weights, rec['xl'])[0]
  cor = o_cor.Correlator()
  for spk in (0, 1):
    cor.add(rec['env'][:, spk:spk + 1].astype(np.float64), pred)
  stats = [float(cor.mean_x[0]), float(cor.mean_y[0]), float(cor.power[0])]
  return pred, cor, np.array([stats, stats], np.float64)


_MODELS = {}


def recording(c):
  """(eeg [1500, c], env [1500, 2], att) of host_online.recipe for c channels -- its generator, call for call --
  without the ridge regression behind it (8192 lagged inputs would make that a long solve)."""
  from telluride_decoding_amd import synth
  rng = np.random.default_rng(host_online.SEED)
  h_att, h_unatt = synth.impulse_responses(rng, c)
  att = np.zeros((FRAMES,), np.float32)
  att[host_online.SWITCH:] = 1.0
  return synth.trial(rng, FRAMES, c, h_att, h_unatt, att)


def model(shape, hidden, seed=5):
  """The recording of host_online.recipe for the shape with a glorot_model on it and its trained statistics:
  dict(c, pre, post, eeg, env, att, weights, hidden, pred64, cor, corr).  Computed once and shared: read-only."""
  key = (tuple(shape), tuple(hidden), seed)
  if key not in _MODELS:
    c, pre, post = shape
    eeg, env, att = recording(c)
    rec = dict(c=c, pre=pre, post=post, eeg=eeg, env=env, att=att,
               xl=o_lag.lag_matrix(eeg.astype(np.float64), pre, post))
    ws = glorot_model(c, pre, post, hidden, seed)
    pred, cor, corr = trained_statistics(rec, ws)
    del rec['xl']
    _MODELS[key] = dict(rec, weights=ws, hidden=list(hidden), pred64=pred, cor=cor, corr=corr)
  return _MODELS[key]


def dnn_recipe(rec, hidden, seed=11):
  """A non-linear model that decodes like the linear recipe, without training: glorot weights with every W scaled
  by 0.25 and hidden biases 0.01 N(0, 1); unit 0 / unit 1 of the first layer = +w / -w of the linear recipe with
  biases +b / -b, carried by identity through the later layers with their other couplings zeroed; output weights
  (+1, -1) on them (relu(z) - relu(-z) = z) and output bias 0.01; trained statistics from one Correlator fed both
  speakers against the float64 forward.  Returns the recipe's dict with weights, hidden, pred64, cor, corr."""
  hidden = list(hidden)
  assert hidden and min(hidden) >= 2
  k = rec['w'].size
  rng = np.random.default_rng(seed)
  ws = host_dnn.glorot([k] + hidden + [1], seed)
  for l in range(len(hidden)):
    ws[2 * l] *= np.float32(0.25)
    ws[2 * l + 1] = (rng.standard_normal(hidden[l]) * 0.01).astype(np.float32)
    if l == 0:
      ws[0][:, 0], ws[0][:, 1] = rec['w'], -rec['w']
      ws[1][0], ws[1][1] = rec['b'], -rec['b']
    else:
      ws[2 * l][:, :2] = 0
      ws[2 * l][:2, :] = 0
      ws[2 * l][0, 0] = ws[2 * l][1, 1] = 1
      ws[2 * l + 1][:2] = 0
  last = 2 * len(hidden)
  ws[last] *= np.float32(0.25)
  ws[last][0, 0], ws[last][1, 0] = 1, -1
  ws[last + 1][:] = 0.01
  pred, cor, corr = trained_statistics(rec, ws)
  return dict(rec, weights=ws, hidden=hidden, pred64=pred, cor=cor, corr=corr)


def linear_as_dnn(rec):
  """The linear recipe's model as a hidden [2] network holding exactly +-w: relu(w x + b) - relu(-(w x + b))."""
  w, b = rec['w'].astype(np.float32), np.float32(rec['b'])
  return [np.stack([w, -w], axis=1), np.array([b, -b], np.float32), np.array([[1.0], [-1.0]], np.float32),
          np.zeros((1,), np.float32)]


def dnn_decoder(c, pre, post, hidden, weights, stats, reduction='first', lda=None, carry='params', outputs=1,
                input_offset=None):
  """An infer_decoder.LinearRegressionDecoder around a BrainModelDNN with the given weights, the trained statistics
  stats = (mean_truth, mean_pred, power) and, for reduction 'lda', lda = (lda_w, slope, intercept) -- built
  without a dataset and without a device.  carry: where the context lives -- 'params' (the decoder's
  decoding_model_params), 'metadata' (the model's add_metadata entry) or None (nowhere: the caller passes
  pre_context= / post_context=)."""
  from telluride_decoding_amd import brain_model, infer_decoder, scaled_lda
  net = brain_model.BrainModelDNN(brain_model._shape_dataset(c * (pre + 1 + post), 1, outputs), list(hidden))
  net.set_weights([np.asarray(w, np.float32) for w in weights])
  decoder = infer_decoder.LinearRegressionDecoder(net, reduction=reduction)
  context = dict(pre_context=pre, post_context=post)
  if input_offset is not None:
    context['input_offset'] = input_offset
  if carry == 'params':
    decoder.decoding_model_params = context
  elif carry == 'metadata':
    net.add_metadata(context)
  decoder._set_correlation_params((1, 0.0, 0.0, 0.0, 0.0, np.array([stats[0]]), np.array([stats[1]]),
                                   np.array([stats[2]])))
  if lda is not None:
    decoder._lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    decoder._lda._w = np.array([[float(lda[0])]])
    decoder._lda._slope, decoder._lda._intercept = float(lda[1]), float(lda[2])
  return decoder


def decoder_of(rec, reduction='first', lda=None, carry='params'):
  return dnn_decoder(rec['c'], rec['pre'], rec['post'], rec['hidden'], rec['weights'], rec['corr'][0], reduction, lda,
                     carry)
