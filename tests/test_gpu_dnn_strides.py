"""Row strides through the td_mlp_* / td_mlpc_* wrappers: x, x2 and y as column ranges of wider device tensors
(ldx > c, ldx2 > c2, ldy > d) against the same calls on contiguous copies.  The arithmetic and its order are
the same and only addresses differ, so every result must be bitwise equal; a width passed where a leading
dimension belongs (or the reverse) reads the large values that fill the other columns."""
import numpy as np
import pytest

from tests import host_dnn
from tests.dnn_common import flat

pytestmark = pytest.mark.gpu

LENGTHS, OFFSET, BATCH, HIDDEN = [90, 75], 1, 70, [5]   # 163 stream rows: steps of 70, 70 (across the files), 23
C, PRE, POST = 3, 1, 2          # x: columns 1..3 of 5
C2, PRE2, POST2 = 2, 0, 1       # x2: columns 2..3 of 4
D = 2                           # y: columns 0..1 of 3
FILL = 1e30


def _inputs(h):
  """((x, x2, y, labels) as strided views, the same as contiguous copies, file offsets)."""
  rng = np.random.default_rng(21)
  rows = sum(LENGTHS)

  def wide(width, first, values):
    t = h.to_device(np.full((rows, width), FILL * np.sign(rng.standard_normal((rows, width))), np.float32))
    t[:, first:first + values.shape[1]] = h.to_device(values)
    return t[:, first:first + values.shape[1]]
  x = wide(5, 1, rng.standard_normal((rows, C)).astype(np.float32))
  x2 = wide(4, 2, rng.standard_normal((rows, C2)).astype(np.float32))
  target = np.tanh(rng.standard_normal((rows, D))).astype(np.float32)
  y = wide(3, 0, target)
  labels = wide(3, 0, (target > 0).astype(np.float32))
  strided = (x, x2, y, labels)
  assert [t.stride(0) for t in strided] == [5, 4, 3, 3] and not any(t.is_contiguous() for t in strided)
  packed = tuple(t.contiguous() for t in strided)
  assert [t.stride(0) for t in packed] == [C, C2, D, D]
  return strided, packed, np.concatenate(([0], np.cumsum(LENGTHS)))


def _calls(h, x, x2, y, labels, offs):
  """Every wrapper once; the arrays each one returns or updates, by name."""
  from telluride_decoding_amd import device
  k1, k2 = C * (PRE + 1 + POST), C2 * (PRE2 + 1 + POST2)
  w = flat(host_dnn.glorot([k1] + HIDDEN + [D], 3))
  wc = flat(host_dnn.glorot([k1 + k2] + HIDDEN + [D], 4))
  w[w == 0] = wc[wc == 0] = np.float32(0.01)             # (the zero biases)
  out = {}

  def keep(name, *tensors):
    for i, t in enumerate(tensors):
      out['%s[%d]' % (name, i)] = t.cpu().numpy()
  for loss in ('mse', 'pearson'):
    keep('mlp_grad ' + loss, *device.mlp_grad(x, y, offs, PRE, POST, HIDDEN, h.to_device(w), BATCH, 1,
                                              input_offset=OFFSET, handle=h, loss=loss))
  keep('mlp_forward', device.mlp_forward(x, offs, PRE, POST, HIDDEN, D, h.to_device(w), input_offset=OFFSET, handle=h))
  keep('mlpc_grad', *device.mlpc_grad(x, x2, labels, offs, PRE, POST, PRE2, POST2, HIDDEN, h.to_device(wc), BATCH, 1,
                                      input_offset=OFFSET, handle=h))
  keep('mlpc_forward', device.mlpc_forward(x, x2, offs, PRE, POST, PRE2, POST2, HIDDEN, D, h.to_device(wc),
                                           input_offset=OFFSET, handle=h))
  params, state = h.to_device(w), h.zeros((w.size,))
  sums = device.mlp_train(x, y, offs, PRE, POST, HIDDEN, params, state, BATCH, 1, 1e-3, 0.9, 1e-7,
                          input_offset=OFFSET, handle=h)
  keep('mlp_train', params, state, sums)
  params, state = h.to_device(wc), h.zeros((2 * wc.size,))
  sums = device.mlpc_train(x, x2, labels, offs, PRE, POST, PRE2, POST2, HIDDEN, params, state, BATCH, 1,
                           input_offset=OFFSET, handle=h)
  keep('mlpc_train', params, state, sums)
  return out


def test_strided_inputs_give_the_bits_of_contiguous_copies():
  from telluride_decoding_amd import device
  h = device.default_handle()
  strided, packed, offs = _inputs(h)
  got, want = _calls(h, *strided, offs), _calls(h, *packed, offs)
  assert sorted(got) == sorted(want) and len(got) == 14
  for name in want:
    assert np.all(np.isfinite(want[name])) and np.any(want[name] != 0), name      # (the filling was never read)
    np.testing.assert_array_equal(got[name], want[name], err_msg=name)
  assert want['mlp_train[2]'].shape == (1, 3, 6) and want['mlpc_train[2]'].shape == (1, 3, 6)
