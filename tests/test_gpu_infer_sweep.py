"""td_attention_sweep (csrc/sweep.hip) against the per-size route it replaces in
infer.run_reduction_test: every window mean bit for bit device.window_means combined as
infer._window_means_host combines columns, the decisions those of td_decide_wta / td_decide_step on
those means, end_first_section = infer.find_first_segment, correct = infer.fraction_correct x windows,
a second call the same bits, and TD_ERR_INVALID for every argument the header says it rejects.

The scores are drawn from [0.5, 1.5): without cancellation a float64 sum of n <= 3000 terms in any
order is within n 2^-53 relative of the exact one (here: <= 12 strided adds, an 8-level tree and one
division, against NumPy's pairwise sum), so "1e-12 relative + 1e-300 absolute of np.mean" is a property
of the arithmetic, not a tuned figure."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT_SIZES = [(10, 5), (100, 50), (200, 100), (400, 200), (700, 350), (1000, 500)]
CASES = [
    (9, [(10, 5)]),                  # no window
    (10, [(10, 5)]),                 # one window
    (2048, [(2, 1)]),
    (2048, [(64, 32)]),
    (2048, [(257, 128)]),            # the strided loop plus a partial wave
    (2048, [(1000, 500)]),
    (2048, DEFAULT_SIZES),           # sizes 700 and 1000 have few windows
]


def _scores(rng, frames, cols):
  """Two speakers' scores with exact ties: a stretch where speaker 2's frames ARE speaker 1's (whole
  windows inside it tie exactly) and single tied frames elsewhere."""
  s1 = rng.uniform(0.5, 1.5, (frames, cols))
  s2 = rng.uniform(0.5, 1.5, (frames, cols))
  lo, hi = frames // 4, frames // 4 + max(frames // 3, 1)
  s2[lo:hi] = s1[lo:hi]
  s2[::7] = s1[::7]
  return s1, s2


def _label_patterns(frames, width, hop):
  """Constant (0 and 1); switching exactly on a window edge; switching inside a window, from 0 and from 1."""
  zeros, ones = np.zeros(frames), np.ones(frames)
  n = (frames - width) // hop + 1 if frames >= width else 0
  edge = (n // 2) * hop if n > 1 else frames // 2
  inside = min(edge + max(width // 3, 1), frames - 1) if frames > 1 else 0
  if inside % hop == 0:
    inside += 1
  out = {'zeros': zeros, 'ones': ones}
  for name, at in (('edge', edge), ('inside', inside)):
    lab = zeros.copy()
    lab[at:] = 1.0
    out[name] = lab
    out[name + '_from_1'] = 1.0 - lab
  return out


def _reference_means(values, width, hop):
  """The per-size route's window means of a host array [frames, cols]: infer._window_means_host -- per column
  one td_window_means launch (device.window_means), the columns' means added in column order and divided by
  their number on the device."""
  from telluride_decoding_amd import infer
  return infer._window_means_host(values, width, hop)


def _same_bits(a, b):
  a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
  return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('cols', [1, 3])
@pytest.mark.parametrize('frames, sizes', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_sweep_matches_the_per_size_route(frames, sizes, cols):
  import torch
  from telluride_decoding_amd import device, infer
  h = device.default_handle()
  rng = np.random.default_rng(1000 * frames + 10 * len(sizes) + cols)
  s1, s2 = _scores(rng, frames, cols)
  s1_dev = h.to_device(s1, np.float64)
  if cols > 1:       # speaker 2 as a view into a wider tensor: a row stride that is not the column count
    wide = h.to_device(rng.uniform(0.5, 1.5, (frames, cols + 2)), np.float64)
    wide[:, 1:1 + cols] = h.to_device(s2, np.float64)
    s2_dev = wide[:, 1:1 + cols]
    assert s2_dev.stride(0) == cols + 2
  else:
    s2_dev = h.to_device(s2, np.float64)
  want_m1 = [_reference_means(s1, w, hop) for w, hop in sizes]
  want_m2 = [_reference_means(s2, w, hop) for w, hop in sizes]
  for name, lab in _label_patterns(frames, *sizes[0]).items():
    lab_dev = h.to_device(lab.reshape(-1, 1), np.float64).reshape(-1)
    want_lab = [_reference_means(lab, w, hop) for w, hop in sizes]
    for decoder in ('wta', 'stepped', 'none'):
      where = 'frames=%d sizes=%s cols=%d labels=%s decoder=%s' % (frames, sizes, cols, name, decoder)
      sweep = device.attention_sweep(s1_dev, s2_dev, lab_dev, sizes, decoder, handle=h)
      got = device.attention_sweep_host(sweep)
      again = device.attention_sweep(s1_dev, s2_dev, lab_dev, sizes, decoder, handle=h)
      assert torch.equal(sweep.packed, again.packed), where         # means, decisions and summary: one buffer
      assert got.means.shape == (3, int(got.window_offsets[-1])) and got.summary.shape == (len(sizes), 2)
      for k, (width, hop) in enumerate(sizes):
        first, last = int(got.window_offsets[k]), int(got.window_offsets[k + 1])
        n = last - first
        assert n == device.window_layout([0, frames], width, hop)[1], where
        m1, m2, ml = (got.means[i, first:last] for i in range(3))
        assert _same_bits(m1, want_m1[k]) and _same_bits(m2, want_m2[k]) and _same_bits(ml, want_lab[k]), where
        if n == 0:
          assert got.summary[k].tolist() == [0, 0], where
          continue
        # ... and close to NumPy's float64 mean of the window's entries
        for m, v in ((m1, s1), (m2, s2), (ml, lab.reshape(-1, 1))) if decoder == 'wta' else ():
          ref = np.array([np.mean(v[i * hop:i * hop + width]) for i in range(n)])
          assert np.all(np.abs(m - ref) <= 1e-12 * np.abs(ref) + 1e-300), where
        assert int(got.summary[k, 0]) == int(infer.find_first_segment(ml)), where
        dec = got.decisions[first:last]
        if decoder == 'none':
          assert not dec.any() and int(got.summary[k, 1]) == 0, where
          continue
        m1_dev = h.to_device(m1.reshape(-1, 1), np.float64).reshape(-1)
        m2_dev = h.to_device(m2.reshape(-1, 1), np.float64).reshape(-1)
        if decoder == 'wta':
          want_dec = device.decide_wta(m1_dev, m2_dev, handle=h).cpu().numpy()
          assert np.array_equal(want_dec, m1 > m2)
        else:
          want_dec = device.decide_step(m1_dev, m2_dev, [0, n], handle=h)[0].cpu().numpy()
        assert dec.dtype == np.uint8 and np.array_equal(dec, want_dec), where
        attention = np.stack([dec.astype(np.float64), np.zeros(n), np.zeros(n)], axis=1)
        frac = infer.fraction_correct(attention, ml)
        correct = int(got.summary[k, 1])
        assert correct / float(n) == frac and correct == int(round(frac * n)), where
  if frames == 2048 and sizes[0][0] <= 257:       # (the tied stretch holds whole windows of these sizes)
    assert int(np.sum(want_m1[0] == want_m2[0])) >= 1, 'the case has no tied window'


def test_stepped_walk_over_several_passes():
  """The stepped decoder's lane walks 16384 windows a pass (sweep.hip: kStepWords words of 64): 40 001 windows
  are three passes, the last one ending inside a word, next to a size that fits one word."""
  from telluride_decoding_amd import device, infer
  h = device.default_handle()
  frames, sizes = 40002, [(2, 1), (2000, 640)]
  rng = np.random.default_rng(5)
  s1, s2 = _scores(rng, frames, 1)
  runs = rng.integers(1, 40, frames)               # speaker 2 louder in runs of 1 .. 39 frames: the state moves about
  s2 += np.repeat(np.arange(frames) % 2, runs)[:frames].reshape(-1, 1) * 0.75
  lab = (np.arange(frames) >= 23456).astype(np.float64)
  s1_dev, s2_dev = h.to_device(s1, np.float64), h.to_device(s2, np.float64)
  lab_dev = h.to_device(lab.reshape(-1, 1), np.float64).reshape(-1)
  got = device.attention_sweep_host(device.attention_sweep(s1_dev, s2_dev, lab_dev, sizes, 'stepped', handle=h))
  assert got.window_offsets.tolist() == [0, 40001, 40001 + 60]
  for k, (width, hop) in enumerate(sizes):
    first, last = int(got.window_offsets[k]), int(got.window_offsets[k + 1])
    m1, m2, ml = (got.means[i, first:last] for i in range(3))
    assert _same_bits(m1, _reference_means(s1, width, hop)) and _same_bits(m2, _reference_means(s2, width, hop))
    assert _same_bits(ml, _reference_means(lab, width, hop))
    m1_dev = h.to_device(m1.reshape(-1, 1), np.float64).reshape(-1)
    m2_dev = h.to_device(m2.reshape(-1, 1), np.float64).reshape(-1)
    want = device.decide_step(m1_dev, m2_dev, [0, last - first], handle=h)[0].cpu().numpy()
    dec = got.decisions[first:last]
    assert np.array_equal(dec, want)
    if k == 0:                 # (the short windows follow the runs: both decisions occur)
      assert 0 < int(dec.sum()) < last - first
    attention = np.stack([dec.astype(np.float64), np.zeros(last - first), np.zeros(last - first)], axis=1)
    assert int(got.summary[k, 1]) / float(last - first) == infer.fraction_correct(attention, ml)
    assert int(got.summary[k, 0]) == int(infer.find_first_segment(ml)) > 0


def test_sweep_rejects_invalid_arguments():
  from telluride_decoding_amd import _lib, device
  h = device.default_handle()
  frames, cols = 64, 2
  s = h.zeros((frames, cols), 'float64')
  lab = h.zeros((frames,), 'float64')
  # room for 16 sizes of 11 windows each
  means, dec, summary = h.zeros((3, 256), 'float64'), h.zeros((256,), 'uint8'), h.zeros((16, 2), 'int64')
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())
  null = ctypes.c_void_p(0)

  def call(s1=ptr(s), ld1=cols, s2=ptr(s), ld2=cols, ncols=cols, labels=ptr(lab), rows=frames, sizes=((10, 5),),
           num_sizes=None, decoder=0, m=ptr(means), d=ptr(dec), sm=ptr(summary), handle=h.ptr):
    sizes_p = None
    if sizes is not None:
      arr = np.ascontiguousarray(np.asarray(sizes, np.intc).reshape(-1))
      sizes_p = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    return h.lib.td_attention_sweep(handle, s1, ld1, s2, ld2, ncols, labels, rows, sizes_p,
                                    len(sizes) if num_sizes is None else num_sizes, decoder, m, d, sm)

  assert call() == _lib.TD_OK
  bad = [dict(s1=null), dict(s2=null), dict(labels=null), dict(m=null), dict(d=null), dict(sm=null),
         dict(sizes=None, num_sizes=1), dict(handle=None),
         dict(num_sizes=0), dict(sizes=((10, 5),) * 17), dict(sizes=((0, 5),)), dict(sizes=((10, 0),)),
         dict(sizes=((10, 5), (-3, 1))), dict(ncols=0), dict(ld1=cols - 1), dict(ld2=cols - 1), dict(rows=-1),
         dict(decoder=3), dict(decoder=-1)]
  for kwargs in bad:
    assert call(**kwargs) == _lib.TD_ERR_INVALID, kwargs
  assert call(sizes=((10, 5),) * 16) == _lib.TD_OK
  h.synchronize()
  # ... and the wrapper raises
  with pytest.raises(ValueError, match='1 to 16 window sizes'):
    device.attention_sweep(s, s, lab, [(10, 5)] * 17, handle=h)
  with pytest.raises(ValueError, match='unknown decoder'):
    device.attention_sweep(s, s, lab, [(10, 5)], 'ssd', handle=h)
  with pytest.raises(ValueError, match='labels'):
    device.attention_sweep(s, s, lab[:10], [(10, 5)], handle=h)
  with pytest.raises(TypeError, match='must be a float64 tensor'):
    device.attention_sweep(s.float(), s, lab, [(10, 5)], handle=h)
