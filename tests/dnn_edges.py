"""The edge cases of the td_mlp_* family (tests/test_gpu_dnn_edges.py, tests/test_cpu_dnn_edges.py): shapes at which
the tiles of csrc/mlp.hip are partly filled -- first-layer widths between the slab kernel's instantiations, batches
that are no multiple of the 64-row chunks, W1 slices whose last one is short -- with their host-side builders (no GPU
needed) and a restatement of the integer arithmetic of mlp_check_and_plan.  A plain module, not a conftest.

The recipes are those of tests/test_gpu_dnn.py, tests/test_gpu_dnn_pearson.py and tests/test_gpu_classifier.py, with
the shape as an argument: the same draws in the same order, the same redraw rules and the same caps on the redraws."""
import functools

import numpy as np

from tests import host_classifier as hc
from tests import host_dnn
from tests import host_dnn_pearson
from tests.dnn_common import KINK, make_files
from tests.test_gpu_classifier import MARGIN_TRAJ, MAX_DRAWS, grad_case as classifier_grad_case

REGRESSOR_DRAWS = 8      # the regressors' cap on the redraws (gradients and trajectories alike)
KINK_TRAJ = 1e-5         # a regressor's trajectory: redraw below this
SHUFFLE = 12345

# ---- 1. gradients ---------------------------------------------------------------------------------------------
# (hidden, channels, pre, post, batch, outputs, input_offset); NJ is the slab kernel's tile width (plan() below)
MSE_GRID = [
    ([16], 3, 1, 2, 70, 1, 0),                  # NJ 16 full; B = 64 + 6
    ([9, 3], 5, 0, 3, 65, 3, 1),                # NJ 16 with 7 dead columns; B = 64 + 1
    ([13], 7, 2, 2, 1, 2, 0),                   # a batch of one row (the recipe's minibatch is step 7)
    ([32], 63, 3, 4, 100, 5, -1),               # NJ 32 full; odd c; K = 504: ks = 8, 63 slices
    ([25, 7], 2, 30, 33, 63, 7, 0),             # NJ 32, w1 = 25; 64 lags; one short head workgroup
    ([17], 130, 0, 0, 130, 1, 0),               # c > 128 context-free; NJ 24; K = 130: last slice 2 rows; B = 128 + 2
    ([33], 1, 0, 0, 191, 8, 0),                 # NJ 48, w1 = 33; K = 1
    ([5], 3, 1, 2, 70, 2, 1),                   # the shape of tests/test_gpu_dnn_strides.py
    ([63, 1, 63], 4, 1, 1, 129, 3, 0),          # NJ 64 with one dead column; a hidden layer of one unit
    ([12, 28, 3, 50], 11, 5, 0, 127, 6, 0),     # four unequal hidden layers (the widest is not the first); B = 128 - 1
    ([], 9, 2, 2, 200, 3, 0),                   # no hidden layer: w1 = d = 3
    ([], 6, 1, 0, 33, 5, -1),                   # no hidden layer: w1 = d = 5
]
PEARSON_GRID = [
    ([16], 3, 1, 2, 70, 2, 0),
    ([27, 3], 5, 0, 3, 65, 3, 1),
    ([13], 130, 0, 0, 130, 1, 0),
]
# (hidden, c1, pre, post, c2, pre2, post2, batch, outputs, input_offset): every one has a slice across both views
CLASSIFIER_GRID = [
    ([16], 3, 1, 1, 2, 0, 2, 70, 1, 0),
    ([29, 5], 5, 2, 0, 3, 1, 1, 100, 3, 1),
    ([11], 7, 0, 0, 1, 3, 2, 65, 2, -1),
    ([32], 130, 0, 0, 3, 0, 1, 33, 5, 0),
]


def regressor_id(c):
  return '%s-c%d-l%d-B%d-D%d-o%d' % ('x'.join(map(str, c[0])) or 'none', c[1], c[2] + c[3] + 1, c[4], c[5], c[6])


def classifier_id(c):
  return '%s-c%d-l%d-c2_%d-l2_%d-B%d-D%d-o%d' % ('x'.join(map(str, c[0])) or 'none', c[1], c[2] + c[3] + 1, c[4],
                                                  c[5] + c[6] + 1, c[7], c[8], c[9])


def regressor_grad_case(loss, hidden, c, pre, post, batch, d, off):
  """Host only: the recipe of test_gpu_dnn._grad_case / test_gpu_dnn_pearson._grad_case up to the device call.  The
  dataset, the tested minibatch (the one across the first file boundary), the weights and the float64 results of the
  first draw of REGRESSOR_DRAWS whose ReLU inputs stay KINK away from 0, or None."""
  from telluride_decoding_amd import brain_data
  grads = host_dnn_pearson.loss_and_grads if loss == 'pearson' else host_dnn.loss_and_grads
  widths = [c * (pre + 1 + post)] + hidden + [d]
  for seed in range(REGRESSOR_DRAWS):
    rng = np.random.default_rng(1000 + seed)
    lengths = [int(batch * f) + 7 for f in (0.6, 1.3, 0.45, 1.9)]          # ragged files
    files = make_files(rng, lengths, c, d)
    ds = brain_data.Dataset(files, batch, pre, post, input_offset=off, mixup_batch=False, mixup_seed=seed)
    batches = list(ds)
    first = max(lengths[0] - abs(off), 0)                                  # the first file's rows of the stream
    s = min(first // batch, len(batches) - 1)
    weights = host_dnn.glorot(widths, seed)
    weights = [w + np.float32(0.05) * rng.standard_normal(w.shape).astype(np.float32) for w in weights]
    x64 = np.asarray(batches[s][0]['input_1'], np.float64)
    y64 = np.asarray(batches[s][1], np.float64)
    loss64, g64, p64, kink = grads(weights, x64, y64)
    if kink >= KINK:
      return dict(ds=ds, s=s, first=first, weights=weights, widths=widths, loss=loss64, g64=g64, p64=p64, y64=y64,
                  kink=kink, draws=seed + 1)
  return None


# ---- 2. trajectories ------------------------------------------------------------------------------------------
# K = 30: eight W1 slices, the last of 2 rows; two head workgroups and two row chunks (64 + 6); NJ 16 with three
# dead columns; six steps an epoch
TRAJ_A = dict(c=5, pre=3, post=2, d=3, batch=70, hidden=[13, 6], lengths=[150, 97, 201], epochs=3)
# K = 81: 21 slices, the last of 1 row; three head workgroups; NJ 32.  (Pearson: d = 2, the output layer's fan-in)
TRAJ_B = dict(c=9, pre=4, post=4, d=1, batch=130, hidden=[30], lengths=[300, 275], epochs=3)
TRAJ_B_PEARSON = dict(TRAJ_B, d=2)
TRAJ_C = dict(c=20, pre=6, post=7, d=2, batch=96, hidden=[20, 20], lengths=[250, 180], epochs=2)   # K = 280: ks = 8
TRAJ_CA = dict(c=5, pre=1, post=1, c2=3, pre2=2, post2=1, d=2, batch=70, hidden=[13, 6], lengths=[150, 97, 201],
               epochs=3)                                                                           # K = 27
TRAJ_CB = dict(c=9, pre=4, post=4, c2=2, pre2=0, post2=3, d=1, batch=130, hidden=[30], lengths=[300, 275],
               epochs=3)                                                                           # K = 89
REGRESSOR_TRAJ = {('mse', 'A'): TRAJ_A, ('mse', 'B'): TRAJ_B, ('mse', 'C'): TRAJ_C,
                  ('pearson', 'A'): TRAJ_A, ('pearson', 'B'): TRAJ_B_PEARSON}
CLASSIFIER_TRAJ = {'A': TRAJ_CA, 'B': TRAJ_CB}


def widths_of(t):
  k = t['c'] * (t['pre'] + 1 + t['post'])
  if 'c2' in t:
    k += t['c2'] * (t['pre2'] + 1 + t['post2'])
  return [k] + t['hidden'] + [t['d']]


@functools.lru_cache(maxsize=None)
def regressor_trajectory_case(loss, name, shuffle_seed):
  """Host only: the recipe of test_gpu_dnn._trajectory / test_gpu_dnn_pearson._trajectory_data at a shape of
  REGRESSOR_TRAJ.  The first draw of REGRESSOR_DRAWS whose float64 trajectory stays KINK_TRAJ away from the ReLU kinks,
  or None.  (Cached: whoever reads it leaves it unchanged.)"""
  t = REGRESSOR_TRAJ[(loss, name)]
  train = host_dnn_pearson.train if loss == 'pearson' else host_dnn.train
  for seed in range(REGRESSOR_DRAWS):
    rng = np.random.default_rng(50 + seed)
    files = make_files(rng, t['lengths'], t['c'], t['d'])
    x64, y64 = host_dnn.stream(files, t['batch'], t['pre'], t['post'])
    w0 = host_dnn.glorot(widths_of(t), seed)
    w64, _, hist64, kink = train(w0, x64, y64, t['batch'], t['epochs'], 1e-3, shuffle_seed=shuffle_seed)
    if kink >= KINK_TRAJ:
      return dict(t=t, files=files, seed=seed, w64=w64, hist64=hist64, kink=kink, draws=seed + 1,
                  steps=x64.shape[0] // t['batch'])
  return None


@functools.lru_cache(maxsize=None)
def classifier_trajectory_case(name, shuffle_seed):
  """Host only: the recipe of test_gpu_classifier.trajectory_case at a shape of CLASSIFIER_TRAJ.  The first draw of
  MAX_DRAWS whose float64 trajectory stays MARGIN_TRAJ away from the kinks and the threshold, or None."""
  t = CLASSIFIER_TRAJ[name]
  for seed in range(MAX_DRAWS):
    rng = np.random.default_rng(60 + seed)
    files = make_files(rng, t['lengths'], t['c'], t['d'], c2=t['c2'])
    x64, y64 = hc.stream(files, t['batch'], t['pre'], t['post'], t['pre2'], t['post2'])
    w0 = host_dnn.glorot(widths_of(t), seed)
    w64, _, hist64, margin = hc.train(w0, x64, y64, t['batch'], t['epochs'], shuffle_seed=shuffle_seed)
    if margin >= MARGIN_TRAJ:
      return dict(t=t, files=files, seed=seed, w64=w64, hist64=hist64, margin=margin, draws=seed + 1,
                  steps=x64.shape[0] // t['batch'])
  return None


def dataset_of(t, files):
  from telluride_decoding_amd import brain_data
  if 'c2' in t:
    return brain_data.Dataset(files, t['batch'], t['pre'], t['post'], t['pre2'], t['post2'])
  return brain_data.Dataset(files, t['batch'], t['pre'], t['post'])


# ---- 3. the many-model kernels and the forward ------------------------------------------------------------------
MANY_EPOCHS = 2
MANY_HELD_A = [[], [0], [2]]          # nothing held out, the first recording, the last (shape A: three recordings)
MANY_HELD_CB = [[], [0], [1]]         # the same of shape B's two recordings
MANY_SEEDS = [31, 32, 33]
MANY_RATES = [1e-3, 3e-3, 2e-3]
# crosses the 4096-row chunks of td_mlp_forward with a ragged last one; NJ 32 with five dead columns
PREDICT = dict(c=5, pre=3, post=3, d=3, batch=64, hidden=[27, 5], lengths=[4100, 4200], offset=1)


# ---- the plan of mlp_check_and_plan, restated -------------------------------------------------------------------
SLAB_WIDTHS = (4, 8, 16, 24, 32, 48, 64)      # the instantiations of mlp_slab_kernel
ROW_TILE = 64                                 # kSlabRowChunk and kHeadRows


def plan(k, hidden, d, batch):
  """What the host derives from a shape: the rows of a W1 slice, the slices and the last one's rows, the slab
  kernel's tile width, the head workgroups and the last one's rows."""
  def ceil_div(a, b):
    return (a + b - 1) // b
  w1 = hidden[0] if hidden else d
  ks = min(64, 4 * ceil_div(ceil_div(k, 64), 4))
  nslices = ceil_div(k, ks)
  n_head = ceil_div(batch, ROW_TILE)
  return dict(w1=w1, ks=ks, nslices=nslices, last_slice=k - (nslices - 1) * ks,
              nj=next(nj for nj in SLAB_WIDTHS if w1 <= nj), n_head=n_head,
              head_last=batch - (n_head - 1) * ROW_TILE)


def plan_of_regressor(shape):
  hidden, c, pre, post, batch, d, _ = shape
  return plan(c * (pre + 1 + post), hidden, d, batch)


def plan_of_classifier(shape):
  hidden, c, pre, post, c2, pre2, post2, batch, d, _ = shape
  return plan(c * (pre + 1 + post) + c2 * (pre2 + 1 + post2), hidden, d, batch)


def plan_of_trajectory(t):
  w = widths_of(t)
  return plan(w[0], t['hidden'], t['d'], t['batch'])
