"""Float64 restatement of BrainModelDNN trained on the Pearson correlation loss for the
tests.  Independent of the product: only the helpers of tests/host_dnn.py are shared.

For a step of B rows and D outputs, per output column o over the step's rows:
  pm = p - mean(p), ym = y - mean(y), Spp = sum pm^2, Syy = sum ym^2, Spy = sum pm ym, r_o = Spy / sqrt(Spp Syy);
  * loss (Keras' mean over frames of PearsonCorrelationLoss.call): L = -(1 / B) sum_o r_o;
  * dL/dp[i, o] = -(1 / B) (ym[i, o] / sqrt(Spp_o Syy_o) - r_o pm[i, o] / Spp_o);
  * the backward pass through the layers and RMSprop are those of tests/host_dnn.py;
  * the output layer's bias gradient is identically zero (the loss does not change with a shift of p) and is
    written as exact 0, not as the rounding residue of sum_i dZ;
  * zero rule: a column that is constant within the step, in the raw float64 sums
    sum p^2 - (sum p)^2 / B <= 32 eps64 sum p^2 (the same for y), has r_o = 0 and a zero dZ column.
"""
import numpy as np

from tests import host_dnn

TINY = 32 * np.finfo(np.float64).eps


def constant_columns(p, y):
  """[D] bool: the zero rule on the raw sums of p and of y."""
  n = float(p.shape[0])
  sp, sy, spp, syy = p.sum(axis=0), y.sum(axis=0), (p * p).sum(axis=0), (y * y).sum(axis=0)
  return (spp - sp ** 2 / n <= TINY * spp) | (syy - sy ** 2 / n <= TINY * syy)


def loss_and_dz(p, y):
  """(L, dL/dp [B, D], r [D]) of one step's predictions and targets."""
  p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
  n = float(p.shape[0])
  zero = constant_columns(p, y)
  pm, ym = p - p.mean(axis=0), y - y.mean(axis=0)
  spp, syy, spy = (pm * pm).sum(axis=0), (ym * ym).sum(axis=0), (pm * ym).sum(axis=0)
  spp, syy = np.where(zero, 1.0, spp), np.where(zero, 1.0, syy)
  power = np.sqrt(spp * syy)
  r = np.where(zero, 0.0, spy / power)
  dz = -(ym / power - r * pm / spp) / n
  dz[:, zero] = 0.0
  return float(-np.sum(r) / n), dz, r


def loss_and_grads(weights, x, y):
  """(loss, [dW1, db1, ...], p, kink) of one minibatch in float64."""
  ws = [np.asarray(w, np.float64) for w in weights]
  p, zs, acts, kink = host_dnn.forward(ws, x)
  loss, dz, _ = loss_and_dz(p, y)
  n_layers = len(ws) // 2
  grads = [None] * len(ws)
  for l in range(n_layers - 1, -1, -1):
    grads[2 * l] = acts[l].T @ dz
    grads[2 * l + 1] = dz.sum(axis=0)
    if l == n_layers - 1:
      grads[2 * l + 1] = np.zeros_like(grads[2 * l + 1])
    if l > 0:
      dz = (dz @ ws[2 * l].T) * (zs[l - 1] > 0)
  return loss, grads, p, kink


def train(weights, x, y, batch, epochs, lr, rho=0.9, eps=1e-7, shuffle_seed=None, state=None):
  """Minibatch RMSprop on the Pearson loss over the stream (x, y): (weights, state, history, kink), history =
  the mean over each epoch's steps of the forward-pass loss / r of output 0 / mse before the step's update."""
  w = [np.asarray(v, np.float64) for v in weights]
  v = [np.zeros_like(a) for a in w] if state is None else [np.asarray(a, np.float64) for a in state]
  n = x.shape[0]
  steps = n // batch
  hist = {'loss': [], 'pearson_correlation_first': [], 'mse': []}
  kink = np.inf
  for e in range(epochs):
    order = np.arange(n) if shuffle_seed is None else host_dnn.permutation(n, shuffle_seed, e)
    losses, rs, mses = [], [], []
    for s in range(steps):
      rows = order[s * batch:(s + 1) * batch]
      loss, grads, p, k = loss_and_grads(w, x[rows], y[rows])
      kink = min(kink, k)
      losses.append(loss)
      mses.append(float(np.mean((p - y[rows]) ** 2)))
      rs.append(host_dnn.pearson_first(p, y[rows]))
      w, v = host_dnn.rmsprop(w, v, grads, lr, rho, eps)
    hist['loss'].append(float(np.mean(losses)))
    hist['mse'].append(float(np.mean(mses)))
    hist['pearson_correlation_first'].append(float(np.mean(rs)))
  return w, v, hist, kink
