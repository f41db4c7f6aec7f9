"""Float64 restatement of the BrainModelClassifier arithmetic contract for the tests.

Independent of the product: only oracle.lag (the reference's lag layout) and the helpers of tests/host_dnn.py
(the shuffle bijection, the seeded Glorot draw) are shared.
  * the input is concat(input_1, input_2) along the features, each the lagged view of its own stream (zero
    outside the file; a negative input_offset drops the leading rows of input_2 as of the output);
  * Dense layers z = a W + b, ReLU on the hidden layers (ReLU'(0) = 0), a sigmoid on the D output units;
  * loss = the mean over the B x D entries of max(z, 0) - z y + log1p(exp(-|z|)) on the output logit z, so
    dL/dz = (sigma(z) - y) / (B D);
  * accuracy = the fraction of entries with (z > 0) == (y > 0.5);
  * Adam (Keras, no amsgrad): m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2, w <- w - lr_t m / (sqrt(v) + eps),
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), m0 = v0 = 0, t from 1, every layer updated after the full backward pass;
  * rows, shuffle and initial weights as tests/host_dnn.py.
"""
import numpy as np

from oracle import lag as o_lag
from tests import host_dnn


def stream(files, batch, pre, post, pre2, post2, input_offset=0):
  """(X [n, K1 + K2], Y [n, D]) float64: the zipped, lagged, concatenated stream cut to whole minibatches."""
  xs, ys = [], []
  for feats, y in o_lag.minibatches(files, batch, pre=pre, post=post, pre2=pre2, post2=post2,
                                    input_offset=input_offset):
    xs.append(np.concatenate([feats['input_1'], feats['input_2']], axis=1))
    ys.append(y)
  return np.concatenate(xs).astype(np.float64), np.concatenate(ys).astype(np.float64)


def forward(weights, x):
  """(logits z, hidden pre-activations, activations [x, a1, ...], margin): margin = min over every hidden
  pre-activation AND every output logit of |z| / (|b| + sum_i |a_i W_ij|): how close a ReLU input came to its
  kink, or a logit to the decision threshold, relative to the float32 rounding scale of its sum."""
  ws = [np.asarray(w, np.float64) for w in weights]
  acts, zs, margin = [np.asarray(x, np.float64)], [], np.inf
  n_layers = len(ws) // 2
  z = None
  for l in range(n_layers):
    w, b = ws[2 * l], ws[2 * l + 1]
    z = acts[-1] @ w + b
    scale = np.abs(acts[-1]) @ np.abs(w) + np.abs(b)
    with np.errstate(invalid='ignore', divide='ignore'):
      rel = np.where(scale > 0, np.abs(z) / scale, np.inf)
    margin = min(margin, float(np.min(rel)) if rel.size else np.inf)
    if l < n_layers - 1:
      zs.append(z)
      acts.append(np.maximum(z, 0.0))
  return z, zs, acts, margin


def sigmoid(z):
  z = np.asarray(z, np.float64)
  e = np.exp(-np.abs(z))
  return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def entry_losses(z, y):
  return np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))


def correct(z, y):
  """The number of entries the threshold 0.5 gets right."""
  return int(np.sum((z > 0) == (y > 0.5)))


def loss_and_grads(weights, x, y):
  """(loss, [dW1, db1, ...], logits, margin, correct count) of one minibatch in float64."""
  ws = [np.asarray(w, np.float64) for w in weights]
  z, zs, acts, margin = forward(ws, x)
  y = np.asarray(y, np.float64)
  loss = float(np.mean(entry_losses(z, y)))
  dz = (sigmoid(z) - y) / z.size
  n_layers = len(ws) // 2
  grads = [None] * len(ws)
  for l in range(n_layers - 1, -1, -1):
    grads[2 * l] = acts[l].T @ dz
    grads[2 * l + 1] = dz.sum(axis=0)
    if l > 0:
      dz = (dz @ ws[2 * l].T) * (zs[l - 1] > 0)
  return loss, grads, z, margin, correct(z, y)


def adam(weights, m, v, grads, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
  """Update number t (from 1) of Keras Adam in float64; returns (weights, m, v)."""
  lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
  new_w, new_m, new_v = [], [], []
  for w, mi, vi, g in zip(weights, m, v, grads):
    mi = b1 * mi + (1.0 - b1) * g
    vi = b2 * vi + (1.0 - b2) * g * g
    new_w.append(w - lr_t * mi / (np.sqrt(vi) + eps))
    new_m.append(mi)
    new_v.append(vi)
  return new_w, new_m, new_v


def evaluate(weights, x, y, batch):
  """{'loss', 'accuracy'}: the means over the minibatches, and the smallest margin."""
  losses, accs, margin = [], [], np.inf
  for s in range(x.shape[0] // batch):
    rows = slice(s * batch, (s + 1) * batch)
    z, _, _, mg = forward(weights, x[rows])
    margin = min(margin, mg)
    losses.append(float(np.mean(entry_losses(z, y[rows]))))
    accs.append(correct(z, y[rows]) / float(z.size))
  return {'loss': float(np.mean(losses)), 'accuracy': float(np.mean(accs))}, margin


def train(weights, x, y, batch, epochs, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, shuffle_seed=None, state=None, t0=0):
  """Minibatch Adam over the stream (x, y): (weights, (m, v, t), history, margin); history = the mean over each
  epoch's steps of the forward-pass loss / accuracy before the step's update."""
  w = [np.asarray(a, np.float64) for a in weights]
  if state is None:
    m, v = [np.zeros_like(a) for a in w], [np.zeros_like(a) for a in w]
  else:
    m, v = [np.asarray(a, np.float64) for a in state[0]], [np.asarray(a, np.float64) for a in state[1]]
  t = t0
  n = x.shape[0]
  steps = n // batch
  hist = {'loss': [], 'accuracy': []}
  margin = np.inf
  for e in range(epochs):
    order = np.arange(n) if shuffle_seed is None else host_dnn.permutation(n, shuffle_seed, e)
    losses, accs = [], []
    for s in range(steps):
      rows = order[s * batch:(s + 1) * batch]
      loss, grads, z, mg, ok = loss_and_grads(w, x[rows], y[rows])
      margin = min(margin, mg)
      losses.append(loss)
      accs.append(ok / float(z.size))
      t += 1
      w, m, v = adam(w, m, v, grads, t, lr, b1, b2, eps)
    hist['loss'].append(float(np.mean(losses)))
    hist['accuracy'].append(float(np.mean(accs)))
  return w, (m, v, t), hist, margin
