"""What the GPU suites of the td_mlp_* family (test_gpu_dnn, test_gpu_dnn_pearson, test_gpu_classifier,
test_gpu_dnn_strides) share: random recordings, the packed parameter layout, the per-tensor gradient distance, and
the data recipes of the reference's behaviour tests.  A plain module, not a conftest."""
import numpy as np

KINK = 1e-6          # a hidden pre-activation closer than this (relative to its sum of |terms|) to 0: redraw
# max|g - g64| / max|g64| per tensor.  Observed: <= 1e-6 on every tensor but one scalar, b1 of
# the one-layer K = 8192, D = 1 case (1.8e-5): the sum over 512 rows of p - y cancels to a few percent of its
# terms, and each float32 prediction carries the rounding of an 8192-term sum.
GRAD_BOUND = 5e-5


def make_files(rng, lengths, c, d, scale=1.0, c2=None):
  """One (x, x2, y, attention) tuple per length.  c2 None: a regressor's recordings (x2 zero, y = tanh of a
  normal draw); else a classifier's (x2 normal, y a 0 / 1 label).  The order of the draws is each suite's own."""
  out = []
  for n in lengths:
    x = (scale * rng.standard_normal((n, c))).astype(np.float32)
    z = np.zeros((n, 1), np.float32)
    if c2 is None:
      out.append((x, z, np.tanh(rng.standard_normal((n, d))).astype(np.float32), z))
    else:
      x2 = rng.standard_normal((n, c2)).astype(np.float32)
      out.append((x, x2, (rng.standard_normal((n, d)) > 0.3).astype(np.float32), z))
  return out


def flat(ws):
  return np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in ws])


def split(flat_params, widths):
  out, at = [], 0
  for fi, fo in zip(widths[:-1], widths[1:]):
    out.append(flat_params[at:at + fi * fo].reshape(fi, fo)); at += fi * fo
    out.append(flat_params[at:at + fo]); at += fo
  return out


def tensor_names(n):
  return ['W%d' % (i // 2 + 1) if i % 2 == 0 else 'b%d' % (i // 2 + 1) for i in range(n)]


def grad_distances(got, want):
  """{tensor name: max |g - g64| / max |g64|} over the leading tensors both lists have."""
  return {name: float(np.max(np.abs(gg - gw)) / max(np.max(np.abs(gw)), 1e-30))
          for name, gg, gw in zip(tensor_names(len(want)), got, want)}


def assert_within(dists, bound):
  for name, dist in dists.items():
    assert dist <= bound, (name, dist)


# ---- the data recipes of the reference's behaviour tests (test/brain_model_test.py), unchanged --------------
def simply_scaled(data_offset=0, channels=2, pre=0, post=0, batch=1000):
  from telluride_decoding_amd import brain_data
  rs = np.random.RandomState(0)
  n = 10000
  inp = rs.randn(n + 2 * abs(data_offset), channels).astype(np.float32)
  out = np.sin(inp[:, 0:1] * 2 * np.pi)
  if data_offset >= 0:
    inp, out = inp[0:n, :], out[data_offset:data_offset + n, :]
  else:
    inp, out = inp[-data_offset:-data_offset + n, :], out[0:n, :]
  bd = brain_data.TestBrainData('input', 'output', 100.0, pre_context=pre, post_context=post,
                                final_batch_size=batch)
  bd.preserve_test_data(inp, out, None)
  return bd.create_dataset('program_test')


def iir(pre):                                  # :494-503
  from telluride_decoding_amd import brain_data
  rs = np.random.RandomState(0)
  n = 10000
  inp = rs.randn(n + 1, 1).astype(np.float32)
  out = 0.4 * inp[0:-1, ] + 0.6 * inp[1:, :]
  bd = brain_data.TestBrainData('input', 'output', 100.0, pre_context=pre, post_context=0,
                                final_batch_size=128)
  bd.preserve_test_data(inp[1:n + 1, :], out, None)
  return bd.create_dataset('program_test')
