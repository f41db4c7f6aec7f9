"""Shared by tests/test_cpu_online_cca.py and tests/test_gpu_online_cca.py: the seeded recording and CCA model of
the online CCA decoder's oracle comparisons, the oracle chain itself, the cuts of the recording and CCADecoders
built around given rotations without a dataset.  Test infrastructure."""
import numpy as np

from oracle import attention as o_att
from oracle import cca as o_cca
from oracle import correlator as o_cor
from oracle import lag as o_lag
from tests import host_online

FRAMES = host_online.FRAMES
SWITCH = host_online.SWITCH
SEED = 2601
CONTEXT_KEYS = ('pre_context', 'post_context', 'input2_pre_context', 'input2_post_context')

# (c1, pre1, post1 | c2, pre2, post2 | dims) and the windows they are paired with
SHAPES = [((5, 2, 9), (3, 1, 4), 2), ((64, 0, 20), (8, 0, 15), 5), ((63, 40, 5), (2, 0, 12), 2),
          ((128, 3, 12), (32, 0, 0), 8), ((3, 31, 32), (1, 5, 2), 1), ((5, 0, 0), (16, 0, 0), 16)]
WINDOWS = [(100, 50), (10, 5), (37, 11), (1, 1), (5, 9), (100, 50)]
REDUCTIONS = ('first', 'second', 'mean', 'mean-squared', 'lda')

_RECIPES = {}


def features(rng, env, c2):
  """One block of c2 audio features per speaker from the two envelopes [n, 2]: band j of a speaker is its
  envelope at a gain that falls with j plus the band's own noise -- [2, n, c2] float32."""
  n = env.shape[0]
  gains = 1.0 / (1.0 + 0.5 * np.arange(c2))
  noise = rng.standard_normal((2, n, c2))
  return (env.T[:, :, None] * gains[None, None, :] + 0.3 * noise).astype(np.float32)


def recipe(view1, view2, dims):
  """The recording and model of the oracle comparisons: rng 2601, synth.impulse_responses, one synth.trial of
  1500 frames whose attention switches to speaker 2 at frame 750, c2 feature bands per speaker (`features`), a
  CCA fit by oracle.cca.cca_parameters_from_batches on the float64 lag matrices of the EEG against the attended
  speaker's features (regularization 0.1) rounded to float32, one oracle.correlator.Correlator fed both
  speakers' (a, b_s) projections, and a seeded LDA (weights, slope, intercept).  A fit has no more than
  min(k1, k2) dims: where the shape asks for more (5 x 1 lags against 16 x 1 in 16 dims) the columns behind the
  fit's are seeded random rotations of the fitted ones' scale -- the session does not care where a rotation
  comes from.  Computed once per shape and shared: treat as read-only."""
  key = (tuple(view1), tuple(view2), dims)
  if key not in _RECIPES:
    from telluride_decoding_amd import synth
    (c1, pre1, post1), (c2, pre2, post2) = view1, view2
    rng = np.random.default_rng(SEED)
    h_att, h_unatt = synth.impulse_responses(rng, c1)
    att = np.zeros((FRAMES,), np.float32)
    att[SWITCH:] = 1.0
    eeg, env, att = synth.trial(rng, FRAMES, c1, h_att, h_unatt, att)
    feat = features(rng, env, c2)
    xl = o_lag.lag_matrix(eeg.astype(np.float64), pre1, post1)
    yl = [o_lag.lag_matrix(feat[k].astype(np.float64), pre2, post2) for k in (0, 1)]
    attended = np.where(att.reshape(-1, 1) > 0.5, yl[1], yl[0])
    rot_x, rot_y, mean_x, mean_y, _ = o_cca.cca_parameters_from_batches(
        [({'input_1': xl, 'input_2': attended}, None)], dims, regularization=0.1, mini_batch_count=0)
    rot_x, rot_y = np.real(rot_x), np.real(rot_y)
    fitted = rot_x.shape[1]
    if fitted < dims:
      extra = dims - fitted
      rot_x = np.concatenate([rot_x, rng.standard_normal((rot_x.shape[0], extra)) * np.std(rot_x)], axis=1)
      rot_y = np.concatenate([rot_y, rng.standard_normal((rot_y.shape[0], extra)) * np.std(rot_y)], axis=1)
    rot_x, rot_y = rot_x.astype(np.float32), rot_y.astype(np.float32)
    mean_x, mean_y = mean_x.astype(np.float32).reshape(-1), mean_y.astype(np.float32).reshape(-1)
    f64 = lambda a: a.astype(np.float64)
    proj = [o_cca.cca_transform(xl, yl[k], f64(mean_x), f64(mean_y), f64(rot_x), f64(rot_y)) for k in (0, 1)]
    a64, b64 = proj[0][:, :dims], [proj[k][:, dims:] for k in (0, 1)]
    cor = o_cor.Correlator()
    for k in (0, 1):
      cor.add(a64, b64[k])
    stats = np.stack([np.broadcast_to(v, (dims,)) for v in (cor.mean_x, cor.mean_y, cor.power)]).astype(np.float64)
    lda = np.concatenate([rng.standard_normal(dims) + 1.0, [-0.8, 0.25]])
    _RECIPES[key] = dict(view1=tuple(view1), view2=tuple(view2), dims=dims, eeg=eeg, env=env, att=att, feat=feat,
                         xl=xl, yl=yl, mean_x=mean_x, rot_x=rot_x, mean_y=mean_y, rot_y=rot_y, a64=a64, b64=b64,
                         cor=cor, corr=np.stack([stats, stats]), lda=lda)
  return _RECIPES[key]


def lda_map(lda):
  """The oracle's lda_transform of a decoder's {weights, slope, intercept}: [frames, dims] -> [frames, 1]."""
  lda = np.asarray(lda, np.float64)
  return lambda c: (lda[-2] * (c @ lda[:-2]) + lda[-1]).reshape(-1, 1)


def oracle_chain(rec, width, hop, reduction='lda'):
  """lag_matrix -> cca_transform -> Correlator.correlate -> reduce_correlations -> windowed_means ->
  wta_sequence / step_sequence, all float64: (scores [windows, 2], wta decisions, stepped decisions)."""
  scores = []
  for k in (0, 1):
    cols = rec['cor'].correlate(rec['a64'], rec['b64'][k])
    reduced = o_cor.reduce_correlations(cols, reduction, lda_map(rec['lda']))
    scores.append(o_cor.windowed_means(reduced, rec['att'], width, hop)[0])
  scores = np.stack(scores, axis=1).reshape(-1, 2)
  return (scores, o_att.wta_sequence(scores[:, 0], scores[:, 1]),
          o_att.step_sequence(scores[:, 0], scores[:, 1])[0])


def chunkings(view1, view2, width, seed=0):
  """The cuts of the recording the chunk-invariance tests walk, {name: push sizes summing to FRAMES}:
  host_online.chunkings' (ones, sevens, one push of width + 1, seeded random sizes with zeros, the whole
  recording) with pushes one row short of EACH view's tail (pre + max(post1, post2) rows)."""
  (_, pre1, post1), (_, pre2, post2) = view1, view2
  delay = max(post1, post2)
  cuts = host_online.chunkings(FRAMES, pre1, delay, width, seed=seed)
  cuts['tail1-1'] = cuts.pop('tail-1')
  cuts['tail2-1'] = host_online.chunkings(FRAMES, pre2, delay, width, seed=seed)['tail-1']
  for name in ('tail1-1', 'tail2-1'):          # (a view without a tail: pushes of one frame, which 'ones' walks)
    if name in cuts and cuts[name] == cuts['ones']:
      del cuts[name]
  if 'tail1-1' in cuts and cuts.get('tail2-1') == cuts['tail1-1']:
    del cuts['tail2-1']
  return cuts


def context_of(view1, view2):
  return dict(zip(CONTEXT_KEYS, (view1[1], view1[2], view2[1], view2[2])))


def cca_decoder(view1, view2, mean_x, rot_x, mean_y, rot_y, stats, reduction='first', lda=None, carry=True):
  """An infer_decoder.CCADecoder around a cca.BrainModelCCA with the given means and rotations, the trained
  statistics stats [3, dims] = (mean_a, mean_b, power) and, for reduction 'lda', lda = (weights..., slope,
  intercept) -- built without a dataset and without a device.  carry: the decoder's decoding_model_params hold
  the two views' contexts (else the caller gives them to OnlineDecoder by keyword)."""
  from telluride_decoding_amd import brain_model, cca, infer_decoder, scaled_lda
  rot_x, rot_y = np.asarray(rot_x, np.float32), np.asarray(rot_y, np.float32)
  dims = int(rot_x.shape[1])
  model = cca.BrainModelCCA(brain_model._shape_dataset(rot_x.shape[0], rot_y.shape[0], 1), cca_dims=dims)
  model.set_weights([np.asarray(mean_x, np.float32).reshape(1, -1), np.asarray(mean_y, np.float32).reshape(1, -1),
                     rot_x, rot_y])
  decoder = infer_decoder.CCADecoder(model, reduction=reduction)
  stats = np.asarray(stats, np.float64).reshape(3, dims)
  zeros = np.zeros(dims)
  decoder._set_correlation_params((1, zeros, zeros, zeros, zeros, stats[0].copy(), stats[1].copy(),
                                   stats[2].copy()))
  if lda is not None:
    lda = np.asarray(lda, np.float64)
    decoder._lda = scaled_lda.ScaledLinearDiscriminantAnalysis()
    decoder._lda._w = lda[:-2].reshape(-1, 1).copy()
    decoder._lda._slope, decoder._lda._intercept = float(lda[-2]), float(lda[-1])
  if carry:
    decoder.decoding_model_params = context_of(view1, view2)
  return decoder


def decoder_of(rec, reduction='first', carry=True):
  return cca_decoder(rec['view1'], rec['view2'], rec['mean_x'], rec['rot_x'], rec['mean_y'], rec['rot_y'],
                     rec['corr'][0], reduction, rec['lda'] if reduction == 'lda' else None, carry=carry)
