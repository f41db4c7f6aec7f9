"""Float64 restatement of the BrainModelDNN arithmetic contract for the tests.

Independent of the product: only oracle.lag (the reference's lag layout) is shared.
  * Dense layers z = a W + b, ReLU on the hidden layers (ReLU'(0) = 0), a linear output layer;
  * loss = mean over the B x D entries of (p - y)^2, so dL/dp = 2 (p - y) / (B D);
  * RMSprop (Keras, momentum 0): v <- rho v + (1 - rho) g^2, w <- w - lr g / (sqrt(v) + eps), v0 = 0, every
    layer updated after the full backward pass;
  * minibatch s of an epoch is rows [s B, (s + 1) B) of the stream, or with a shuffle seed the rows
    permutation(n, seed, epoch)[s B:(s + 1) B] (the Feistel bijection of include/td_hotpath.h);
  * initial weights: glorot_uniform drawn with numpy.random.default_rng(seed), layer by layer.
"""
import numpy as np

from oracle import lag as o_lag

M32 = 0xffffffff


def mix32(z):
  """The 32-bit finaliser of the shuffle, on Python ints or uint64 arrays holding 32-bit values."""
  z = np.asarray(z, np.uint64) & np.uint64(M32)
  z ^= z >> np.uint64(16)
  z = (z * np.uint64(0x7feb352d)) & np.uint64(M32)
  z ^= z >> np.uint64(15)
  z = (z * np.uint64(0x846ca68b)) & np.uint64(M32)
  z ^= z >> np.uint64(16)
  return z


def permutation(n, seed, epoch):
  """perm[i] = the stream row slot i of epoch `epoch` visits: 4 Feistel rounds on 2 x half bits (the smallest
  even bit count with 2^bits >= n), cycle-walked into [0, n)."""
  bits = 2
  while (1 << bits) < n:
    bits += 2
  half = np.uint64(bits // 2)
  mask = np.uint64((1 << (bits // 2)) - 1)
  lo, hi = seed & M32, (seed >> 32) & M32
  keys = [np.uint64(int(mix32(lo ^ int(mix32(hi ^ int(mix32((epoch * 4 + r) & M32))))))) for r in range(4)]

  def rounds(v):
    for k in keys:
      left, right = v >> half, v & mask
      v = (right << half) | (left ^ (mix32(right ^ k) & mask))
    return v

  v = rounds(np.arange(n, dtype=np.uint64))
  out = v >= np.uint64(n)
  while out.any():
    v[out] = rounds(v[out])
    out = v >= np.uint64(n)
  return v.astype(np.int64)


def glorot(widths, seed):
  """[W1, b1, ...] as the product's documented initialisation (float32)."""
  rng = np.random.default_rng(seed)
  out = []
  for fi, fo in zip(widths[:-1], widths[1:]):
    lim = np.sqrt(6.0 / (fi + fo))
    out += [rng.uniform(-lim, lim, (fi, fo)).astype(np.float32), np.zeros((fo,), np.float32)]
  return out


def stream(files, batch, pre, post, input_offset=0):
  """(X [n, K], Y [n, D]) float64: the zipped, lagged stream of the files cut to whole minibatches."""
  xs, ys = [], []
  for feats, y in o_lag.minibatches(files, batch, pre=pre, post=post, input_offset=input_offset):
    xs.append(feats['input_1'])
    ys.append(y)
  return np.concatenate(xs).astype(np.float64), np.concatenate(ys).astype(np.float64)


def forward(weights, x):
  """(p, pre-activations of the hidden layers, activations [x, a1, ...], kink): kink = min over every hidden
  pre-activation of |z| / (|b| + sum_i |a_i W_ij|), how close a ReLU input came to its kink relative to the
  float32 rounding scale of its sum (inf without hidden layers)."""
  ws = [np.asarray(w, np.float64) for w in weights]
  acts, zs, kink = [np.asarray(x, np.float64)], [], np.inf
  n_layers = len(ws) // 2
  for l in range(n_layers):
    w, b = ws[2 * l], ws[2 * l + 1]
    z = acts[-1] @ w + b
    if l < n_layers - 1:
      scale = np.abs(acts[-1]) @ np.abs(w) + np.abs(b)
      with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(scale > 0, np.abs(z) / scale, np.inf)
      kink = min(kink, float(np.min(rel)) if rel.size else np.inf)
      zs.append(z)
      acts.append(np.maximum(z, 0.0))
    else:
      p = z
  return p, zs, acts, kink


def loss_and_grads(weights, x, y):
  """(loss, [dW1, db1, ...], p, kink) of one minibatch in float64."""
  ws = [np.asarray(w, np.float64) for w in weights]
  p, zs, acts, kink = forward(ws, x)
  y = np.asarray(y, np.float64)
  diff = p - y
  loss = float(np.mean(diff ** 2))
  dz = 2.0 * diff / diff.size
  n_layers = len(ws) // 2
  grads = [None] * len(ws)
  for l in range(n_layers - 1, -1, -1):
    grads[2 * l] = acts[l].T @ dz
    grads[2 * l + 1] = dz.sum(axis=0)
    if l > 0:
      dz = (dz @ ws[2 * l].T) * (zs[l - 1] > 0)
  return loss, grads, p, kink


def rmsprop(weights, state, grads, lr, rho=0.9, eps=1e-7):
  """One Keras RMSprop step (momentum 0) in float64; returns (weights, state)."""
  new_w, new_v = [], []
  for w, v, g in zip(weights, state, grads):
    v = rho * v + (1.0 - rho) * g * g
    new_w.append(w - lr * g / (np.sqrt(v) + eps))
    new_v.append(v)
  return new_w, new_v


def pearson_first(p, y):
  """Pearson r of output 0 with pearson_correlation's zero rule (a constant column gives 0)."""
  a, b = p[:, 0], y[:, 0]
  va, vb = np.sum((a - a.mean()) ** 2), np.sum((b - b.mean()) ** 2)
  if va <= 0 or vb <= 0:
    return 0.0
  return float(np.sum((a - a.mean()) * (b - b.mean())) / np.sqrt(va * vb))


def train(weights, x, y, batch, epochs, lr, rho=0.9, eps=1e-7, shuffle_seed=None, state=None):
  """Minibatch RMSprop over the stream (x, y): (weights, state, history, kink), history = the mean over each
  epoch's steps of the forward-pass loss / r / mse before the step's update."""
  w = [np.asarray(v, np.float64) for v in weights]
  v = [np.zeros_like(a) for a in w] if state is None else [np.asarray(a, np.float64) for a in state]
  n = x.shape[0]
  steps = n // batch
  hist = {'loss': [], 'pearson_correlation_first': [], 'mse': []}
  kink = np.inf
  for e in range(epochs):
    order = np.arange(n) if shuffle_seed is None else permutation(n, shuffle_seed, e)
    losses, rs = [], []
    for s in range(steps):
      rows = order[s * batch:(s + 1) * batch]
      loss, grads, p, k = loss_and_grads(w, x[rows], y[rows])
      kink = min(kink, k)
      losses.append(loss)
      rs.append(pearson_first(p, y[rows]))
      w, v = rmsprop(w, v, grads, lr, rho, eps)
    hist['loss'].append(float(np.mean(losses)))
    hist['mse'].append(float(np.mean(losses)))
    hist['pearson_correlation_first'].append(float(np.mean(rs)))
  return w, v, hist, kink
