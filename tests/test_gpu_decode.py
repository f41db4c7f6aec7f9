"""GPU parity tests of the decode path (A3' forward, A5-A9) and of CCA (A4).

HIP kernels through the C-ABI vs the CPU oracle on the same seeded inputs and
vs the golden fixtures generated from the reference itself.
"""
import time

import numpy as np
import pytest

from oracle import attention as o_att
from oracle import cca as o_cca
from oracle import correlator as o_cor
from oracle import lag as o_lag
from oracle import pearson as o_p
from oracle import regression as o_reg
from tests import parity_log
from tests.conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _d64(h, v):
  return h.to_device(np.asarray(v, np.float64).reshape(-1, 1), np.float64).reshape(-1)


# (the route of each shape is the one tests/fir_edges.fir_route restates; the accuracy test of every route of the ladder is
# tests/test_gpu_fir_edges.py, of the streamed kernel the three tests below)
@pytest.mark.parametrize('c,pre,post,d,lens,off', [
    (64, 0, 31, 1, (1000, 300, 257), 0),  # one output: the streamed kernel (fir_stream_kernel), as every d = 1 below
    (16, 2, 3, 2, (700, 64), 0),        # matrix-core kernel, one group of two outputs
    (5, 0, 0, 1, (513,), 0),            # streamed kernel, 4-byte DMA
    (70, 3, 40, 3, (900,), 0),          # > 64 channels and > 32 lags: the VALU kernel's chunk loops, passes <2> + <1>
    (8, 1, 2, 1, (400, 300), 2),        # input_offset drops leading x rows per file (streamed kernel)
    (4, 6, 6, 1, (5, 3, 700), 0),       # files shorter than the context (streamed kernel)
    (63, 0, 31, 1, (1500, 200), 0),     # unaligned rows, 32 taps: the streamed kernel by 4-byte DMA
    (69, 2, 10, 3, (800, 333), 1),      # lane-per-channel kernel <32, 2>: two channel passes, outputs in pairs
    (64, 0, 31, 20, (3000, 500), 0),    # 20 outputs (a lambda sweep): matrix-core kernel, seven groups of <= 3
    (48, 5, 8, 11, (2048,), 0),         # matrix-core kernel, four groups
    (7, 0, 0, 9, (640,), 0),            # no lags, unaligned: lane-per-channel kernel <4, 8>, two output passes
    (130, 1, 1, 2, (300, 77), 0),       # three channel passes of the short-filter variant <4, 8>
])
def test_predict_fir_matches_dense_forward(dev, c, pre, post, d, lens, off):
  rng = np.random.default_rng(c * 100 + pre)
  h = dev.default_handle()
  k = c * (pre + 1 + post)
  w = (rng.standard_normal((k, d)) / np.sqrt(k)).astype(np.float32)
  b = rng.standard_normal(d).astype(np.float32)
  xs = [rng.standard_normal((n, c)).astype(np.float32) for n in lens]
  offs = np.concatenate(([0], np.cumsum(lens)))
  out = dev.predict_fir(h.to_device(np.concatenate(xs)), offs, h.to_device(w),
                        h.to_device(b.reshape(1, -1)).reshape(-1), pre, post, handle=h,
                        input_offset=off).cpu().numpy()
  for i, x in enumerate(xs):
    xl = o_lag.lag_matrix(x[off:].astype(np.float64), pre, post)
    want = xl @ w.astype(np.float64) + b
    got = out[offs[i]:offs[i] + want.shape[0]]
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('c', [64, 32, 48, 4, 60, 63, 61, 5, 1, 69, 80, 72, 100, 128])
@pytest.mark.parametrize('pre,post,lens,off,mode', [
    (0, 31, (6000, 6000, 6000), 0, 'f16x2'),     # the C4 shape: strips of several tile pairs
    (0, 36, (2500, 700, 20), 0, 'f16x2'),        # 37 lags (the codelab's): two lag slices
    (40, 20, (900, 64, 1300), 1, 'f16x2'),       # 61 lags, most of them past context
    (10, 30, (777,), 0, 'f32'),
    (5, 20, (700, 64, 1, 31, 33, 1300), 0, 'f16x2'),   # context before the frame, recordings of 1 / 31 / 33 rows
    (31, 0, (900, 257), 0, 'f16x2'),             # only past context
    (0, 0, (640, 100), 0, 'f16x2'),              # one lag
    (3, 7, (500, 300), 2, 'f16x2'),              # input_offset drops leading rows of every recording
    (0, 31, (1000, 300, 257), 0, 'f32'),         # the float32 matrix instruction (td_set_accumulate_mode F32)
    (2, 9, (77, 2049), 1, 'f32'),
])
def test_predict_fir_streamed_kernel_edges(dev, c, pre, post, lens, off, mode):
  """One output, up to 128 channels and 64 lags: fir_stream_kernel (decode.hip) in slices of <= 64
  channels x <= 32 lags (the first slice writes, the others add); rows of whole aligned 16-byte
  granules by 16-byte DMA (granules past a row's end read as zeros), 63 / 61 / 5 / 1 / 69 channels
  by 4-byte DMA, one row per instruction (channels past the row's end are lanes sent out of range --
  the decode of the reference's 63-channel Telluride4 and 69-channel codelab data).  Rows before / after a
  recording come from the buffer descriptor's range check as zeros, a wave's strip ends anywhere in a
  pair of tiles, the diagonal sums are DPP lane shifts across two tiles: every one of those against
  the float64 lag matrix of the oracle (brain_model.py:335-341), in both arithmetic modes, with rows
  of very different magnitudes (the float16 pieces are scaled per row)."""
  rng = np.random.default_rng(pre * 37 + post + c)
  h = dev.default_handle()
  nl = pre + 1 + post
  w = (rng.standard_normal((c * nl, 1)) / np.sqrt(c * nl)).astype(np.float32)
  b = rng.standard_normal(1).astype(np.float32)
  xs = [rng.standard_normal((n, c)).astype(np.float32) for n in lens]
  # rows 2^-20 ... 2^20 apart in scale, one all-zero row, one row with a single huge sample
  for x in xs:
    n = x.shape[0]
    x *= np.exp2(rng.integers(-20, 21, size=(n, 1))).astype(np.float32)
    if n > 40:
      x[7] = 0.0
      x[20, min(3, c - 1)] = 3.0e30
  offs = np.concatenate(([0], np.cumsum(lens)))
  saved = h.accumulate_mode
  try:
    h.set_accumulate_mode(mode)
    out = dev.predict_fir(h.to_device(np.concatenate(xs)), offs, h.to_device(w),
                          h.to_device(b.reshape(1, -1)).reshape(-1), pre, post, handle=h,
                          input_offset=off).cpu().numpy()
  finally:
    h.set_accumulate_mode(saved)
  worst = 0.0
  for i, x in enumerate(xs):
    if x.shape[0] <= off:
      continue
    xl = o_lag.lag_matrix(x[off:].astype(np.float64), pre, post)
    want = xl @ w.astype(np.float64) + b
    got = out[offs[i]:offs[i] + want.shape[0]].astype(np.float64)
    # error relative to the size of the terms of each output's sum (a float32 rounding of every term)
    size = np.abs(xl) @ np.abs(w.astype(np.float64)) + np.abs(b)
    err = np.max(np.abs(got - want) / size)
    worst = max(worst, err)
    # (a product of two float16 pieces is exact to 2^-22 = 2.4e-7; with fewer than four channels an
    # output is a sum of so few terms that their errors do not average below that)
    assert err < (4e-7 if c >= 4 else 6e-7), (i, err)
  parity_log.record('fir_stream c%d pre%d post%d %s' % (c, pre, post, mode), gpu_vs_ref64=worst)


def test_predict_fir_streamed_kernel_random_shapes(dev):
  """Forty random shapes of the streamed kernel's domain (channels in granules of four up to 64, up to
  32 lags split any way between past and future, recordings of 1 .. 5000 rows, leading rows dropped,
  rows wider than the channels used, with and without a bias) against the float64 lag matrix."""
  import torch
  rng = np.random.default_rng(2024)
  h = dev.default_handle()
  for case in range(80):
    if case < 40:
      c = 4 * int(rng.integers(1, 17))
      nl = int(rng.integers(1, 33))
      pad = 4 * int(rng.integers(0, 4))
    else:      # any channel count up to 128, up to 64 lags, any row pitch: 4-byte DMA, slices
      c = int(rng.integers(1, 129))
      nl = int(rng.integers(1, 65))
      pad = int(rng.integers(0, 7))
    pre = int(rng.integers(0, nl))
    post = nl - 1 - pre
    lens = [int(v) for v in rng.integers(1, 5001, size=int(rng.integers(1, 6)))]
    off = int(rng.integers(0, 4)) if min(lens) > 8 else 0
    n = int(np.sum(lens))
    wide = rng.standard_normal((n, c + pad)).astype(np.float32)
    x = wide[:, :c]
    w = (rng.standard_normal((c * nl, 1)) / np.sqrt(c * nl)).astype(np.float32)
    b = rng.standard_normal(1).astype(np.float32) if case % 2 else None
    offs = np.concatenate(([0], np.cumsum(lens)))
    xd = h.to_device(wide)[:, :c]
    bd = h.to_device(b.reshape(1, -1)).reshape(-1) if b is not None else None
    out = dev.predict_fir(xd, offs, h.to_device(w), bd, pre, post, handle=h, input_offset=off).cpu().numpy()
    for i in range(len(lens)):
      xi = x[offs[i] + off:offs[i + 1]]
      if xi.shape[0] == 0:
        continue
      xl = o_lag.lag_matrix(xi.astype(np.float64), pre, post)
      want = xl @ w.astype(np.float64) + (b if b is not None else 0.0)
      got = out[offs[i]:offs[i] + want.shape[0]].astype(np.float64)
      size = np.abs(xl) @ np.abs(w.astype(np.float64)) + (np.abs(b) if b is not None else 0.0) + 1e-30
      err = np.max(np.abs(got - want) / size)
      assert err < (4e-7 if c >= 4 else 6e-7), (case, c, pre, post, lens, off, pad, i, err)


def test_predict_fir_streamed_kernel_strided_rows_and_nonfinite(dev):
  """Rows wider than the 64 channels used (a column slice of a wider array), and what a NaN / Inf
  sample does: exactly the outputs whose lag window holds it become non-finite (numpy's answer)."""
  import torch
  rng = np.random.default_rng(11)
  h = dev.default_handle()
  n, pre, post = 1500, 0, 31
  wide = rng.standard_normal((n, 80)).astype(np.float32)
  w = (rng.standard_normal((64 * 32, 1)) / 45.0).astype(np.float32)
  xd = h.to_device(wide)[:, 8:72]                      # ldx = 80, base 32-byte aligned
  out = dev.predict_fir(xd, [0, n], h.to_device(w), None, pre, post, handle=h).cpu().numpy()
  want = o_lag.lag_matrix(wide[:, 8:72].astype(np.float64), pre, post) @ w.astype(np.float64)
  np.testing.assert_allclose(out, want, rtol=2e-5, atol=2e-5)
  for cc in (64, 63, 69):                      # (16-byte DMA; 4-byte DMA; two channel slices)
    x = np.ascontiguousarray(wide[:, :cc])
    x[700, 5] = np.nan
    x[900, cc - 4] = np.inf
    x[901, 0] = np.nan                         # (the sample that follows row 900's last channel in memory)
    for pre2, post2 in ((0, 31), (2, 9), (3, 40)):   # (a filter shorter than the 32-lag tile, two lag slices)
      w2 = (rng.standard_normal((cc * (pre2 + 1 + post2), 1)) / 45.0).astype(np.float32)
      out = dev.predict_fir(h.to_device(x), [0, n], h.to_device(w2), None, pre2, post2, handle=h).cpu().numpy()
      bad = ~np.isfinite(out[:, 0])
      expect = np.zeros(n, bool)
      expect[700 - post2:700 + pre2 + 1] = True
      expect[900 - post2:901 + pre2 + 1] = True
      assert np.array_equal(bad, expect), (cc, pre2, post2, np.flatnonzero(bad != expect))


def test_window_pearson_zero_rule_is_per_model(dev):
  """td_window_pearson: the columns are several models of `group` outputs each (the lambdas of a
  jackknife fold); a constant column zeroes the Pearson result of ITS model only -- the
  reference calls pearson_correlation once per model (regression.py:197-214,
  brain_model.py:72-79)."""
  rng = np.random.default_rng(5)
  h = dev.default_handle()
  n, width, group, models = 1200, 400, 2, 3
  cols = group * models
  a = rng.standard_normal((n, cols)).astype(np.float32)
  b = (0.5 * a + rng.standard_normal((n, cols))).astype(np.float32)
  b[:400, 3] = 1.25                      # window 0: second output of model 1 is constant
  a[400:800, 4] = -3.0                   # window 1: first truth column of model 2 is constant
  sums = dev.window_sums(h.to_device(a), h.to_device(b), [0, n], width, width, handle=h)
  got = dev.window_scores(sums, width, 1, handle=h, group=group).cpu().numpy()
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  for wi in range(3):
    r = slice(wi * width, (wi + 1) * width)
    for m in range(models):
      c = slice(m * group, (m + 1) * group)
      want = o_p.pearson_correlation(a64[r, c], b64[r, c])
      want = want if np.ndim(want) == 1 else np.zeros(group)
      np.testing.assert_allclose(got[wi, c], want, rtol=1e-9, atol=1e-12)
  assert np.all(got[0, 2:4] == 0) and np.all(got[0, :2] != 0) and np.all(got[0, 4:] != 0)
  assert np.all(got[1, 4:] == 0) and np.all(got[1, :4] != 0)
  # one group over all the columns = the single-model rule of td_window_scores(mode 1)
  whole = dev.window_scores(sums, width, 1, handle=h).cpu().numpy()
  assert np.all(whole[0] == 0) and np.all(whole[1] == 0) and np.all(whole[2] != 0)
  with pytest.raises(ValueError, match='whole groups'):
    dev.window_scores(sums, width, 1, handle=h, group=4)


def test_window_sums_and_scores(dev):
  rng = np.random.default_rng(3)
  h = dev.default_handle()
  lens = (2400, 999, 3100)
  cols = 3
  a = (rng.standard_normal((sum(lens), cols)) + 0.5).astype(np.float32)
  b = (0.6 * a + rng.standard_normal(a.shape)).astype(np.float32)
  b[2400:3399, 1] = 2.0                     # a constant column inside trial 1
  offs = np.concatenate(([0], np.cumsum(lens)))
  width, hop = 1000, 100
  sums = dev.window_sums(h.to_device(a), h.to_device(b), offs, width, hop, handle=h)
  wo, total = dev.window_layout(offs, width, hop)
  assert total == sum(max(0, (n - width) // hop + 1) for n in lens) == sums.shape[0]
  np.testing.assert_array_equal(wo, [0, 15, 15, 37])     # trial 1 is shorter than a window
  s = sums.cpu().numpy()
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  starts = np.concatenate([offs[t] + o_cor.window_starts(lens[t], width, hop) for t in range(3)])
  for wi in (0, 7, 14, 15, 36):
    r = slice(starts[wi], starts[wi] + width)
    want = np.stack([a64[r].sum(0), b64[r].sum(0), (a64[r] ** 2).sum(0), (b64[r] ** 2).sum(0),
                     (a64[r] * b64[r]).sum(0)], axis=1)
    np.testing.assert_allclose(s[wi], want, rtol=1e-12, atol=1e-9)
  # flavour A6/A7: trained global statistics, mean over the window
  cor = o_cor.Correlator()
  cor.add(a64, b64)
  for red in ('first', 'second', 'mean'):
    got = dev.window_scores(sums, width, 0, red, cor.mean_x, cor.mean_y, cor.power,
                            handle=h).cpu().numpy()
    frames = o_cor.reduce_correlations(cor.correlate(a64, b64), red)
    want = np.array([np.mean(frames[st:st + width]) for st in starts])
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
  # flavour A5: per-window Pearson, incl. the constant-column -> zeros rule
  got = dev.window_scores(sums, width, 1, handle=h).cpu().numpy()
  for wi in (0, 14, 20, 36):
    r = slice(starts[wi], starts[wi] + width)
    want = o_p.pearson_correlation(a64[r], b64[r])
    want = want if want.ndim == 1 else np.zeros(cols)
    np.testing.assert_allclose(got[wi], want, rtol=1e-9, atol=1e-12)


def test_window_sums_at_c4_size_properties(dev):
  """BASELINE C4 size (200 trials x 6000 frames, W = 1000, hop = 100): size-independent
  checks -- windows tile the trial, sums of non-overlapping windows add up."""
  import torch
  h = dev.default_handle()
  trials, frames = 200, 6000
  torch.manual_seed(4)
  a = torch.randn(trials * frames, 1, device='cuda')
  b = torch.randn(trials * frames, 1, device='cuda')
  offs = np.arange(trials + 1) * frames
  s = dev.window_sums(a, b, offs, 1000, 100, handle=h)
  assert s.shape[0] == trials * 51
  s = s.reshape(trials, 51, 5).cpu().numpy()
  whole = dev.window_sums(a, b, offs, 6000, 6000, handle=h).reshape(trials, 5).cpu().numpy()
  np.testing.assert_allclose(s[:, 0::10, :].sum(axis=1), whole, rtol=1e-12, atol=1e-9)
  ad = a.double().reshape(trials, frames)
  np.testing.assert_allclose(whole[:, 0], ad.sum(1).cpu().numpy(), rtol=1e-12, atol=1e-9)


def test_frame_scores_reductions_match_golden(dev):
  g = golden('g5_correlator')
  h = dev.default_handle()
  x, y = g['x'], g['y']
  xd, yd = h.to_device(x), h.to_device(y)
  args = (g['mean_x'], g['mean_y'], g['power'])
  got = dev.frame_scores(xd, yd, 'all', *args, handle=h).cpu().numpy()
  np.testing.assert_allclose(got, g['corr'], rtol=2e-5, atol=2e-6)   # reference is float32
  for red in ('first', 'second', 'mean', 'mean-squared'):
    got = dev.frame_scores(xd, yd, red, *args, handle=h).cpu().numpy()
    np.testing.assert_allclose(got, g['red_' + red.replace('-', '_')], rtol=5e-5, atol=5e-6)
  with pytest.raises(ValueError, match='Unknown reduction technique'):
    dev.frame_scores(xd, yd, 'bogus', *args, handle=h)


def test_wta_and_step_match_reference_sequences(dev):
  g = golden('g7_decoders')
  h = dev.default_handle()
  for a, b, want in ((g['cor1'], g['cor2'], g['wta_lit']), (g['rand1'], g['rand2'], g['wta_rand'])):
    got = dev.decide_wta(_d64(h, a), _d64(h, b), handle=h).cpu().numpy()
    np.testing.assert_array_equal(got, want)            # bit exact, ties -> speaker 2
  for a, b, want in ((g['cor1'], g['cor2'], g['step_lit']), (g['short1'], g['cor2'], g['step_short']),
                     (g['rand1'], g['rand2'], g['step_rand'])):
    got, _ = dev.decide_step(_d64(h, a), _d64(h, b), [0, len(a)], handle=h)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
  # several trials in one launch, states independent; chunked calls carry the state
  a = np.concatenate((g['cor1'], g['short1'], g['rand1']))
  b = np.concatenate((g['cor2'], g['cor2'], g['rand2']))
  got, st = dev.decide_step(_d64(h, a), _d64(h, b), [0, 13, 26, 526], handle=h)
  np.testing.assert_array_equal(got.cpu().numpy(),
                                np.concatenate((g['step_lit'], g['step_short'], g['step_rand'])))
  first, st1 = dev.decide_step(_d64(h, g['rand1'][:200]), _d64(h, g['rand2'][:200]), [0, 200], handle=h)
  second, _ = dev.decide_step(_d64(h, g['rand1'][200:]), _d64(h, g['rand2'][200:]), [0, 300],
                              state=st1, handle=h)
  np.testing.assert_array_equal(np.concatenate((first.cpu().numpy(), second.cpu().numpy())),
                                g['step_rand'])


@pytest.mark.parametrize('name,tune,offset', [('ssd_tuned', True, 0.0), ('ssd_default', False, 0.0),
                                              ('ssd_offset', True, 1.0)])
def test_state_space_decoder_matches_reference_trajectory(dev, name, tune, offset):
  g = golden('g7_decoders')
  h = dev.default_handle()
  c = g[name + '_corr']
  prior = o_att.tune_log_normal_priors(c[:30, 0], c[:30, 1], offset) if tune else None
  out = dev.decode_ssd(_d64(h, c[:, 0]), _d64(h, c[:, 1]), [0, c.shape[0]], offset=offset,
                       prior=prior, handle=h).cpu().numpy()
  want = g[name + '_traj']
  np.testing.assert_allclose(out, want, rtol=1e-7, atol=1e-9)
  np.testing.assert_array_equal(out[:, 0] >= 0.5, want[:, 0] >= 0.5)
  # batched: the same trial three times plus a short one stays independent
  s1 = np.concatenate((c[:, 0], c[:40, 0], c[:, 0]))
  s2 = np.concatenate((c[:, 1], c[:40, 1], c[:, 1]))
  n = c.shape[0]
  out3 = dev.decode_ssd(_d64(h, s1), _d64(h, s2), [0, n, n + 40, 2 * n + 40], offset=offset,
                        prior=prior, handle=h).cpu().numpy()
  np.testing.assert_array_equal(out3[:n], out)
  np.testing.assert_array_equal(out3[n + 40:], out)
  np.testing.assert_array_equal(out3[n:n + 40], out[:40])
  # fed as the windows arrive (td_decode_ssd_stream): any split of the trial over calls gives the
  # outputs of the single call, bit for bit -- one window at a time, then uneven chunks; two trials
  # with their own states in one call
  st = dev.ssd_state(1, handle=h)
  pieces = [dev.decode_ssd(_d64(h, c[i:i + 1, 0]), _d64(h, c[i:i + 1, 1]), [0, 1], offset=offset,
                           prior=prior, handle=h, state=st).cpu().numpy() for i in range(n)]
  np.testing.assert_array_equal(np.concatenate(pieces), out)
  st2 = dev.ssd_state(2, handle=h)
  got = [[], []]
  for a, b in ((0, 5), (5, 6), (6, 33), (33, n)):
    s1 = np.concatenate((c[a:b, 0], c[a:b, 0]))
    s2 = np.concatenate((c[a:b, 1], c[a:b, 1]))
    o = dev.decode_ssd(_d64(h, s1), _d64(h, s2), [0, b - a, 2 * (b - a)], offset=offset, prior=prior,
                       handle=h, state=st2).cpu().numpy()
    got[0].append(o[:b - a]); got[1].append(o[b - a:])
  np.testing.assert_array_equal(np.concatenate(got[0]), out)
  np.testing.assert_array_equal(np.concatenate(got[1]), out)


def test_attention_decoder_classes(dev):
  from telluride_decoding_amd import attention_decoder as ad
  g = golden('g7_decoders')
  wta = ad.create_attention_decoder('wta')
  assert wta.attention(0.6, 0.4)[0] and not wta.attention(0.4, 0.6)[0]
  assert wta.attention(0.6 * np.ones(5), 0.4 * np.ones(5)) == (True, 0, 0)
  stp = ad.create_attention_decoder('stepped')
  got = [stp.attention(a, b)[0] for a, b in zip(g['cor1'], g['cor2'])]
  np.testing.assert_array_equal(got, g['step_lit'])
  np.testing.assert_array_equal(ad.StepAttentionDecoder().attention_batch(g['cor1'], g['cor2'])[0],
                                g['step_lit'])
  c = g['ssd_tuned_corr']
  ssd = ad.create_attention_decoder('ssd')
  ssd.tune(c[:30, 0], c[:30, 1])
  np.testing.assert_allclose(ssd.mu_d, g['ssd_tuned_mu_d_tuned'], rtol=1e-12)
  stream = np.array([ssd.attention(a, b) for a, b in c[:40]])
  np.testing.assert_allclose(stream, g['ssd_tuned_traj'][:40], rtol=1e-7, atol=1e-9)
  # (the streaming object keeps its state on the device: the 300th call costs what the 20th did)
  t0 = time.perf_counter()
  for a, b in c[40:60]:
    ssd.attention(a, b)
  early = time.perf_counter() - t0
  for a, b in np.tile(c[60:100], (6, 1)):
    ssd.attention(a, b)
  t0 = time.perf_counter()
  for a, b in c[100:120]:
    ssd.attention(a, b)
  assert time.perf_counter() - t0 < 5 * early + 0.05
  batch = ad.create_attention_decoder('ssd')
  batch.tune(c[:30, 0], c[:30, 1])
  p, lo, hi = batch.attention_batch(c[:, 0], c[:, 1])
  np.testing.assert_allclose(np.stack((p, lo, hi), 1), g['ssd_tuned_traj'], rtol=1e-7, atol=1e-9)
  with pytest.raises(ValueError, match=r'Unknown type \(bogus\) requested from create_attention_decoder'):
    ad.create_attention_decoder('bogus')


def test_end_to_end_two_speaker_decode_matches_reference(dev):
  """G9: fit -> predict -> correlate -> window -> decide, every decision equal to
  the reference's (attended-speaker argmax bit-exact), scores within 1e-5."""
  from telluride_decoding_amd import brain_data, brain_model, infer_decoder, attention_decoder
  g = golden('g9_end_to_end')
  c, pre, post, batch = (int(v) for v in g['cfg'])
  lamb = float(g['lamb'])
  h = dev.default_handle()
  bd = brain_data.TestBrainData('eeg', 'envelope', 100, pre_context=pre, post_context=post,
                                final_batch_size=batch)
  for i in range(4):
    eeg, env = g['train_eeg%d' % i], g['train_env%d' % i]
    bd.add_file(eeg, env[:, 0:1], env[:, 1:2])
  train = bd.create_dataset('train')
  model = brain_model.BrainModelLinearRegression(train, regularization_lambda=lamb)
  assert model.fit(train) == {}
  # TRF weights: the same rule as test_gpu_fit.test_ridge_matches_reference_golden -- strict
  # 1e-5 against the reference's float32 output unless the reference itself is further than
  # 3e-6 from its own algorithm in float64
  files64 = [(g['train_eeg%d' % i].astype(np.float64), g['train_env%d' % i][:, 1:2].astype(np.float64),
              g['train_env%d' % i][:, 0:1].astype(np.float64),
              np.zeros((g['train_eeg%d' % i].shape[0], 1))) for i in range(4)]
  w64, _, _, _, _ = o_reg.linear_regressor_from_batches(
      o_lag.minibatches(files64, batch, pre=pre, post=post), lamb=lamb)
  scale = np.max(np.abs(w64))
  d_gpu_64 = np.max(np.abs(model.w_estimate - w64)) / scale
  d_32_64 = np.max(np.abs(g['w'] - w64)) / scale
  d_gpu_32 = np.max(np.abs(model.w_estimate - g['w'])) / scale
  parity_log.record('ridge_g9_end_to_end', gpu_ref64=d_gpu_64, ref32_ref64=d_32_64,
                    gpu_ref32=d_gpu_32, strict=bool(d_gpu_32 < 1e-5))
  assert d_gpu_64 < 1e-5
  assert d_gpu_32 < (1e-5 if d_32_64 < 3e-6 else 1e-5 + 1.01 * d_32_64)
  # trained correlation statistics: truth = attended envelope, prediction = model
  dec = infer_decoder.LinearRegressionDecoder(model, reduction='first')
  pred = model.predict_device(train)
  _, _, y, offs = train.device_arrays(h)
  used = train.rows_used()
  import torch
  rows = torch.cat([torch.arange(offs[i], offs[i] + u) for i, u in enumerate(used)]).cuda()
  dec.add_data_correlator(y[rows], pred[rows])
  np.testing.assert_allclose(dec.correlation_params.power, g['power'], rtol=1e-4)
  width = int(g['width'])
  flips = total = 0
  margins = []
  for step_name, step in (('half', None), ('hop50', 50)):
    for i in range(3):
      eeg, env, att = g['test_eeg%d' % i], g['test_env%d' % i], g['test_att%d' % i]
      n_used = (eeg.shape[0] // 200) * 200        # the reference's 200-frame minibatches
      x = h.to_device(eeg)
      p = dev.predict_fir(x, [0, eeg.shape[0]], *model._device_weights(h), pre, post, handle=h)
      scores = []
      for spk in (0, 1):
        s, _ = dec.decode_windows(h.to_device(env[:n_used, spk:spk + 1]), p[:n_used].contiguous(),
                                  [0, n_used], width, step)
        scores.append(s)
      k = '%s_t%d_' % (step_name, i)
      got1, got2 = scores[0].cpu().numpy(), scores[1].cpu().numpy()
      np.testing.assert_allclose(got1, g[k + 's1'], rtol=1e-5, atol=2e-6)
      np.testing.assert_allclose(got2, g[k + 's2'], rtol=1e-5, atol=2e-6)
      wta = attention_decoder.AttentionDecoder().attention_batch(scores[0], scores[1])[0]
      stp = attention_decoder.StepAttentionDecoder().attention_batch(scores[0], scores[1])[0]
      flips += int(np.sum(wta != g[k + 'wta'])) + int(np.sum(stp != g[k + 'step']))
      total += 2 * len(wta)
      margins.append(np.min(np.abs(g[k + 's1'] - g[k + 's2'])))
  print('end-to-end: %d decisions, %d flips, min |s1 - s2| margin %.3e' % (total, flips, min(margins)))
  parity_log.record('decisions_g9_end_to_end', decisions=total, flips=flips, min_margin=min(margins))
  assert flips == 0


def test_decode_fused_equals_unfused_at_scale(dev):
  """td_decode_fused vs the separate kernels on a C4-shaped problem (smaller trial
  count), plus accuracy of the winner-take-all decision on planted attention."""
  from telluride_decoding_amd import synth
  h = dev.default_handle()
  trials = synth.make_trials(7, 12, 6000, 64, switch_half=True)
  eeg = np.concatenate([t[0] for t in trials])
  env = np.concatenate([t[1] for t in trials])
  att = np.concatenate([t[2] for t in trials])
  offs = np.arange(13) * 6000
  attended = np.where(att > 0.5, env[:, 1:2], env[:, 0:1]).astype(np.float32)
  st = dev.LagStats(64, 0, 31, d=1)
  xd, envd = h.to_device(eeg), h.to_device(env)
  st.accumulate(xd, None, h.to_device(attended), offs)
  w, b = st.ridge_solve([0.1])
  w, b = w[0].contiguous(), b[0].contiguous()
  pred = dev.predict_fir(xd, offs, w, b, 0, 31, handle=h)
  corr = []
  for spk in (0, 1):
    s = dev.window_sums(envd[:, spk:spk + 1], pred, [0, eeg.shape[0]], eeg.shape[0],
                        eeg.shape[0], handle=h).cpu().numpy()[0, 0]
    n = eeg.shape[0]
    mean_t, mean_p = s[0] / n, s[1] / n
    power = np.sqrt((s[2] - s[0] ** 2 / n) * (s[3] - s[1] ** 2 / n)) / n
    corr += [mean_t, mean_p, power]
  scores, decisions = dev.decode_fused(xd, envd, offs, w, b, 0, 31, 1000, 100, corr, handle=h)
  scores, decisions = scores.cpu().numpy(), decisions.cpu().numpy()
  assert scores.shape == (12 * 51, 2)
  for spk in (0, 1):
    sums = dev.window_sums(envd[:, spk:spk + 1], pred, offs, 1000, 100, handle=h)
    want = dev.window_scores(sums, 1000, 0, 'first', corr[3 * spk], corr[3 * spk + 1],
                             corr[3 * spk + 2], handle=h).cpu().numpy()
    np.testing.assert_array_equal(scores[:, spk], want)
  np.testing.assert_array_equal(decisions, scores[:, 0] > scores[:, 1])
  labels = dev.window_means(h.to_device(att.astype(np.float64), np.float64).reshape(-1), offs, 1000,
                            100, handle=h).cpu().numpy()
  clear = (labels < 0.05) | (labels > 0.95)          # windows with one attended speaker
  acc = np.mean((decisions[clear] == 1) == (labels[clear] < 0.5))
  assert acc > 0.95, acc                              # reference floor: infer_test.py:171-176


@pytest.mark.parametrize('width,hop,pre,post', [(1000, 100, 0, 31), (1000, 500, 0, 31), (400, 200, 3, 20),
                                                (256, 64, 0, 7), (96, 32, 0, 40),
                                                # short windows: blocks of gcd(W, hop) < 32 frames in the
                                                # per-trial tail kernel (the harness' W = 10), and a pair
                                                # without a common divisor worth blocks (the unfused chain)
                                                (10, 5, 0, 31), (30, 12, 2, 9), (37, 11, 0, 5)])
def test_decode_fused_matches_oracle(dev, width, hop, pre, post):
  """td_decode_fused (FIR prediction -> block sums of both speakers -> window scores +
  winner-take-all) against the ORACLE chain: dense forward on the
  materialised lag matrix, per-frame global-statistics correlation
  (infer_decoder.py:326-328), np.mean per window (infer.py:263-265), strict > (attention_
  decoder.py:128-134).  24 distinct trials, half of them with an attention switch, of different
  lengths (incl. one window exactly and none at all)."""
  from telluride_decoding_amd import synth
  h = dev.default_handle()
  c = 64
  lens = [6000, 5000, 3100, width, width - 1, 4321, 2048, 6000] * 3
  rng = np.random.default_rng(width + hop)
  h_att, h_unatt = synth.impulse_responses(rng, c)
  trials = []
  for i, n in enumerate(lens):
    att = np.zeros((n,), np.float32)
    if i % 2 == 1:
      att[n // 2:] = 1.0
    trials.append(synth.trial(rng, n, c, h_att, h_unatt, att))
  eeg = np.concatenate([t[0] for t in trials])
  env = np.concatenate([t[1] for t in trials])
  att = np.concatenate([t[2] for t in trials])
  offs = np.concatenate(([0], np.cumsum(lens)))
  attended = np.where(att > 0.5, env[:, 1:2], env[:, 0:1]).astype(np.float32)
  st = dev.LagStats(c, pre, post, d=1)
  xd, envd = h.to_device(eeg), h.to_device(env)
  st.accumulate(xd, None, h.to_device(attended), offs)
  w, b = st.ridge_solve([0.1])
  w, b = w[0].contiguous(), b[0].contiguous()
  wn, bn = w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
  # oracle: predictions per trial (context never crosses a trial), trained statistics over all
  pred_o = [o_reg.dense_forward(o_lag.lag_matrix(t[0].astype(np.float64), pre, post), wn, bn)
            for t in trials]
  cors, corr = [], []
  for spk in (0, 1):
    cor = o_cor.Correlator()
    cor.add(env[:, spk:spk + 1].astype(np.float64), np.concatenate(pred_o))
    cors.append(cor)
    corr += [float(cor.mean_x[0]), float(cor.mean_y[0]), float(cor.power[0])]
  scores, decisions = dev.decode_fused(xd, envd, offs, w, b, pre, post, width, hop, corr, handle=h)
  scores, decisions = scores.cpu().numpy(), decisions.cpu().numpy()
  want = [[], []]
  for t, p in zip(trials, pred_o):
    for spk in (0, 1):
      want[spk].append(o_cor.windowed_means(
          cors[spk].correlate(t[1][:, spk:spk + 1].astype(np.float64), p), t[2], width, hop)[0])
  want = [np.concatenate(v) for v in want]
  assert scores.shape == (len(want[0]), 2) and len(want[0]) > 0
  # float32 predictions on the device vs float64 in the oracle: 1e-5 relative (north_star)
  tol = 1e-5 * max(np.max(np.abs(want[0])), np.max(np.abs(want[1])))
  np.testing.assert_allclose(scores[:, 0], want[0], rtol=1e-5, atol=tol)
  np.testing.assert_allclose(scores[:, 1], want[1], rtol=1e-5, atol=tol)
  truth = o_att.wta_sequence(want[0], want[1])
  margin = np.abs(want[0] - want[1])
  flips = int(np.sum(decisions != truth))
  print('fused decode W=%d hop=%d: %d windows, %d decision flips vs oracle, min margin %.2e' %
        (width, hop, len(truth), flips, margin.min()))
  parity_log.record('decode_fused_W%d_hop%d' % (width, hop), windows=len(truth), flips=flips,
                    min_margin=float(margin.min()),
                    max_score_err=float(max(np.max(np.abs(scores[:, 0] - want[0])),
                                            np.max(np.abs(scores[:, 1] - want[1])))))
  assert flips == 0                   # attended-speaker argmax bit-exact


@pytest.mark.parametrize('width,hop', [(10, 5), (7, 3), (200, 77), (300, 7)])
def test_window_sums_without_shared_blocks(dev, width, hop):
  """Windows whose width and hop share no block of >= 32 frames (the reference harness' W = 10,
  hop = 5, infer.py:376-378): thread-per-window kernel for short windows, workgroup-per-window
  beyond 256 frames; every window against float64 NumPy, and td_decode_fused on that shape
  against the window sums."""
  rng = np.random.default_rng(width)
  h = dev.default_handle()
  lens = (640, 9, 1201)
  cols = 2
  a = rng.standard_normal((sum(lens), cols)).astype(np.float32)
  b = (0.5 * a + rng.standard_normal(a.shape)).astype(np.float32)
  offs = np.concatenate(([0], np.cumsum(lens)))
  sums = dev.window_sums(h.to_device(a), h.to_device(b), offs, width, hop, handle=h).cpu().numpy()
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  starts = np.concatenate([offs[t] + o_cor.window_starts(lens[t], width, hop) for t in range(3)])
  assert sums.shape == (len(starts), cols, 5)
  want = np.stack([np.stack([a64[s:s + width].sum(0), b64[s:s + width].sum(0),
                             (a64[s:s + width] ** 2).sum(0), (b64[s:s + width] ** 2).sum(0),
                             (a64[s:s + width] * b64[s:s + width]).sum(0)], axis=1) for s in starts])
  np.testing.assert_allclose(sums, want, rtol=1e-12, atol=1e-10)


def test_pearson_functions(dev):
  from telluride_decoding_amd import brain_model, cca
  g = golden('g3_pearson')
  kat = g['kat']
  r = brain_model.pearson_correlation(kat[:, 1:2], kat[:, 2:3])
  assert abs(float(r[0]) - 0.5298) < 1e-4                      # brain_model_test.py:1065
  np.testing.assert_allclose(brain_model.pearson_correlation(g['x'], g['y']), g['r'], atol=2e-6)
  z = brain_model.pearson_correlation(g['x_const'], g['y'])
  assert z.shape == g['r_zero'].shape and not z.any()
  assert abs(brain_model.pearson_correlation_first(g['x'], g['y']) - g['r_first']) < 2e-6
  assert abs(brain_model.pearson_correlation_second(g['x'], g['y']) - g['r_second']) < 2e-6
  yy = np.concatenate((g['x'], g['y']), axis=1)
  np.testing.assert_allclose(cca.cca_pearson_correlation(None, yy), g['r_cca'], atol=2e-6)
  with pytest.raises(ValueError, match='CCA y matrix does not have even # dims'):
    cca.cca_pearson_correlation(None, yy[:, :7])


def test_pearson_correlation_loss(dev):
  """brain_model.PearsonCorrelationLoss (reference brain_model.py:94-126): the per-frame
  negative correlations of the reference's own code (golden G13, generate_golden.py) -- the six-point
  known answer of test/brain_model_test.py:1083-1090 (sum -0.5298) and a seeded [300, 3] block -- from the
  window-sums and frame-scores kernels; a shape mismatch is the reference's ValueError."""
  from telluride_decoding_amd import brain_model
  g = golden('g13_loss_time_axis')
  pcl = brain_model.PearsonCorrelationLoss()
  got = pcl.call(g['kat'][:, 1:2], g['kat'][:, 2:3])
  np.testing.assert_allclose(got, g['loss_kat'], rtol=2e-5, atol=2e-7)
  assert abs(float(np.sum(got)) + 0.5298) < 1e-4
  got = pcl(g['x'], g['y'])
  assert got.shape == g['loss'].shape and got.dtype == np.float32
  np.testing.assert_allclose(got, g['loss'], rtol=2e-5, atol=2e-6)
  with pytest.raises(ValueError, match='must have the same size'):
    pcl.call(g['x'], g['y'][:, :2])


def _aligned(a, ref):
  """Fix the per-component sign ambiguity of CCA rotations."""
  sign = np.sign(np.sum(a * ref, axis=0))
  sign[sign == 0] = 1
  return a * sign


@pytest.mark.parametrize('name', ['t42', 'r10'])
def test_cca_matches_reference_golden(dev, name):
  from telluride_decoding_amd import brain_data, cca
  g = golden('g4_cca')
  dim, batch = (int(v) for v in g[name + '_cfg'])
  bd = brain_data.TestBrainData('input_1', 'input_2', 100.0, final_batch_size=batch)
  bd.preserve_test_data(g['x1'], np.ones((g['x1'].shape[0], 1), np.float32), g['x2'])
  ds = bd.create_dataset('program_test', temporal_context=False)
  a, b, mx, my, e = cca.calculate_cca_parameters_from_dataset(
      ds, dim, regularization=float(g[name + '_reg']), mini_batch_count=1000)
  np.testing.assert_allclose(e, g[name + '_e'], rtol=2e-5, atol=2e-6)
  np.testing.assert_allclose(mx, g[name + '_mean_x'], atol=1e-6)
  np.testing.assert_allclose(my, g[name + '_mean_y'], atol=1e-6)
  # singular vectors of well separated singular values, up to a joint sign
  nsep = 2
  np.testing.assert_allclose(_aligned(a[:, :nsep], g[name + '_rot_x'][:, :nsep]),
                             g[name + '_rot_x'][:, :nsep], atol=3e-4)
  np.testing.assert_allclose(_aligned(b[:, :nsep], g[name + '_rot_y'][:, :nsep]),
                             g[name + '_rot_y'][:, :nsep], atol=3e-4)
  if name == 't42':                                             # cca_test.py:111-123
    assert e[0] > 0.90 and e[1] > 0.60 and e[2] < 0.02
  with pytest.raises(ValueError, match='regularization lambda must be >= 0'):
    cca.calculate_cca_parameters_from_dataset(ds, dim, regularization=-1)


def test_cca_lagged_fit_transform_and_model(dev):
  from telluride_decoding_amd import brain_data, cca
  g = golden('g4_cca')
  pre, post, pre2, post2, batch, dim = (int(v) for v in g['lag_cfg'])
  bd = brain_data.TestBrainData('eeg', 'env', 100.0, pre_context=pre, post_context=post,
                                in2_fields='env', in2_pre_context=pre2, in2_post_context=post2,
                                final_batch_size=batch)
  for i in range(2):
    bd.add_file(g['lag_eeg%d' % i], g['lag_env%d' % i][:, 0:1], g['lag_env%d' % i])
  ds = bd.create_dataset('train')
  a, b, mx, my, e = cca.calculate_cca_parameters_from_dataset(ds, dim, regularization=0.1,
                                                              mini_batch_count=0)
  np.testing.assert_allclose(e, g['lag_e'], rtol=1e-4, atol=1e-5)
  model = cca.BrainModelCCA(ds, cca_dims=dim, regularization_lambda=0.1)
  assert model.fit(ds) == {}
  # transform vs the oracle using the SAME rotations (isolates the kernel)
  out = model.predict(ds)
  files = [(g['lag_eeg%d' % i], g['lag_env%d' % i], g['lag_env%d' % i][:, 0:1],
            np.zeros((3000, 1), np.float32)) for i in range(2)]
  want = np.concatenate([o_cca.cca_transform(f['input_1'].astype(np.float64),
                                             f['input_2'].astype(np.float64), model.mean_x,
                                             model.mean_y, model.rot_x, model.rot_y)
                         for f, _ in o_lag.minibatches(files, batch, pre=pre, post=post,
                                                       pre2=pre2, post2=post2)])
  np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4)
  ev = model.evaluate(ds)
  r_batches = [o_p.cca_pearson_correlation(None, want[s:s + batch])[0]
               for s in range(0, want.shape[0], batch)]
  assert abs(ev['cca_pearson_correlation_first'] - np.mean(r_batches)) < 1e-5
  assert ev['cca_pearson_correlation_first'] > 0.5
  with pytest.raises(ValueError, match=r'Input 2 feature width \(1\) should not be <= 1'):
    bd1 = brain_data.TestBrainData('eeg', 'env', 100.0, final_batch_size=100)
    bd1.preserve_test_data(g['lag_eeg0'], g['lag_env0'][:, 0:1])
    cca.BrainModelCCA(bd1.create_dataset('train'))


@pytest.mark.parametrize('c1,c2,dims,lens,off', [
    (64, 8, 5, (100000,), 0),            # the C3 shape (a tenth of its rows): strips of many tiles
    (64, 8, 8, (700, 31, 1, 33, 1300), 0),   # 16 outputs; recordings of 1 / 31 / 33 rows
    (32, 4, 2, (900, 257), 0),           # narrower views: granules past a row's end read as zeros
    (4, 8, 1, (640, 100), 0),
    (60, 8, 3, (500, 300), 2),           # input_offset > 0: x starts later, its last rows do not exist
    (64, 4, 4, (500, 300), -3),          # input_offset < 0: the same for the second view
])
def test_cca_transform_streamed_kernel_edges(dev, c1, c2, dims, lens, off):
  """The transform without context (cca.py:157-161) on cca_project_stream_kernel: both views by DMA,
  float16 x 2 under a per-row, per-view scale -- the views decades apart in magnitude (EEG in volts,
  envelopes in thousands), rows 2^30 apart in scale inside a view -- against float64."""
  rng = np.random.default_rng(c1 + 7 * c2 + dims)
  h = dev.default_handle()
  n = int(np.sum(lens))
  x = (rng.standard_normal((n, c1)) * 2e-5).astype(np.float32)
  x2 = (rng.standard_normal((n, c2)) * 3e3 + 1e3).astype(np.float32)
  x *= np.exp2(rng.integers(-15, 16, size=(n, 1))).astype(np.float32)
  mean1 = x.mean(0).astype(np.float32)
  mean2 = x2.mean(0).astype(np.float32)
  rot1 = (rng.standard_normal((c1, dims)) * 1e4).astype(np.float32)
  rot2 = (rng.standard_normal((c2, dims)) * 1e-3).astype(np.float32)
  offs = np.concatenate(([0], np.cumsum(lens)))
  out = dev.cca_transform(h.to_device(x), h.to_device(x2), offs, h.to_device(mean1), h.to_device(rot1),
                          h.to_device(mean2), h.to_device(rot2), 0, 0, 0, 0, handle=h,
                          input_offset=off).cpu().numpy().astype(np.float64)
  dx, dy = max(off, 0), max(-off, 0)
  worst = 0.0
  for f in range(len(lens)):
    a, b = int(offs[f]), int(offs[f + 1])
    nx, ny = max(b - a - dx, 0), max(b - a - dy, 0)
    x64, y64 = x[a + dx:b].astype(np.float64), x2[a + dy:b].astype(np.float64)
    for (v, m, r, cnt, col0) in ((x64, mean1, rot1, nx, 0), (y64, mean2, rot2, ny, dims)):
      if cnt == 0:
        continue
      want = (v - m.astype(np.float64)) @ r.astype(np.float64)
      size = np.abs(v) @ np.abs(r.astype(np.float64)) + np.abs(m.astype(np.float64)) @ np.abs(r.astype(np.float64))
      err = np.max(np.abs(out[a:a + cnt, col0:col0 + dims] - want) / size)
      worst = max(worst, err)
      assert err < 6e-7, (f, col0, err)
  parity_log.record('cca_transform_stream c%d+%d dims%d' % (c1, c2, dims), gpu_vs_ref64=worst)


def test_linear_regression_model_api(dev):
  """BrainModelLinearRegression: the W/b known answer, predict, evaluate."""
  from telluride_decoding_amd import brain_data, brain_model
  g = golden('g2_ridge')
  x, y = g['kat_x'], g['kat_y']
  bd = brain_data.TestBrainData('input_1', 'output', 100.0, final_batch_size=100)
  bd.preserve_test_data(x, y)
  ds = bd.create_dataset('train')
  w, b, cov_x, cov_xy, shrink = brain_model.calculate_linear_regressor_parameters_from_dataset(
      ds, lamb=0.0)
  np.testing.assert_allclose(w, [[1, 3], [2, 4]], atol=1e-4)     # brain_model_test.py:192-193
  np.testing.assert_allclose(b, [[5, 6]], atol=1e-4)
  np.testing.assert_allclose(cov_x, g['kat_cov_x'], rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(cov_xy, g['kat_cov_xy'], rtol=1e-5, atol=1e-6)
  assert shrink == 0.0
  # the same through a plain iterable of already-lagged minibatches
  batches = [({'input_1': x[i:i + 100]}, y[i:i + 100]) for i in range(0, 10000, 100)]
  w2, b2, _, _, _ = brain_model.calculate_linear_regressor_parameters_from_dataset(batches, lamb=0.0)
  np.testing.assert_allclose(w2, w, atol=2e-5)
  model = brain_model.BrainModelLinearRegression(ds, regularization_lambda=0.0)
  model.fit(ds)
  pred = model.predict(ds)
  np.testing.assert_allclose(pred, y, rtol=1e-5, atol=1e-4)       # brain_model_test.py:243-249
  np.testing.assert_allclose(model({'input_1': x[:50]}), y[:50], rtol=1e-5, atol=1e-4)
  ev = model.evaluate(ds)
  assert ev['loss'] < 1e-6 and ev['pearson_correlation_first'] > 0.9999
  # shrinkage branch against the reference's golden output
  files = [g['c1_eeg%d' % i] for i in range(3)]
  bd = brain_data.TestBrainData('eeg', 'env', 100.0, final_batch_size=100)
  for i in range(3):
    bd.add_file(g['c1_eeg%d' % i], g['c1_env%d' % i][:, 0:1])
  ws, bs, cs, _, sh = brain_model.calculate_linear_regressor_parameters_from_dataset(
      bd.create_dataset('train'), lamb=0.3, use_ridge=False)
  np.testing.assert_allclose(ws, g['shrink_0p3_w'], rtol=1e-3, atol=2e-5)
  np.testing.assert_allclose(cs, g['shrink_0p3_cov_x'], rtol=1e-4, atol=1e-4)
  with pytest.raises(ValueError, match='Regularization lambda must be between 0 and 1'):
    brain_model.calculate_linear_regressor_parameters_from_dataset(ds, lamb=2.0, use_ridge=False)


@pytest.mark.parametrize('c,pre,post,d,lens', [
    (64, 0, 31, 20, (3000, 129, 31250, 64)),     # the sweep's shape: 20 lambdas as output columns
    (16, 2, 5, 3, (500, 500, 7)),                # narrow, a recording shorter than the context
    (70, 0, 3, 2, (900, 300)),                   # not the matrix-core kernel's shape: one call per recording
])
def test_predict_fir_per_file_equals_one_call_per_file(dev, c, pre, post, d, lens):
  """td_predict_fir_per_file (every recording under its own weights, one launch) against
  td_predict_fir recording by recording: the same kernel and arithmetic, bit for bit."""
  rng = np.random.default_rng(c + d)
  h = dev.default_handle()
  offs = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
  x = h.to_device(rng.standard_normal((int(offs[-1]), c)).astype(np.float32))
  k = c * (pre + 1 + post)
  w = h.to_device(rng.standard_normal((len(lens), k, d)).astype(np.float32))
  b = h.to_device(rng.standard_normal((len(lens), d)).astype(np.float32))
  got = dev.predict_fir_per_file(x, offs, w, b, pre, post).cpu().numpy()
  for f in range(len(lens)):
    one = dev.predict_fir(x[int(offs[f]):int(offs[f + 1])], [0, lens[f]], w[f].contiguous(),
                          b[f].contiguous(), pre, post).cpu().numpy()
    np.testing.assert_array_equal(got[int(offs[f]):int(offs[f + 1])], one)


def test_forward_model_with_many_outputs(dev):
  """A forward model (one envelope with context -> 20 EEG channels): more outputs than the
  batched solver's right-hand sides, through fit / predict / evaluate of the model class."""
  from telluride_decoding_amd import brain_data, brain_model
  rng = np.random.default_rng(21)
  n, c, d, post = 6000, 2, 20, 7
  x = rng.standard_normal((n, c)).astype(np.float32)
  xp = np.vstack([x.astype(np.float64), np.zeros((post, c))])      # brain_data.py:448-454
  lagged = np.hstack([xp[l:l + n] for l in range(post + 1)])
  y = (lagged @ rng.standard_normal((lagged.shape[1], d)) * 0.3 + 0.1 * rng.standard_normal((n, d)) +
       rng.standard_normal((1, d))).astype(np.float32)
  bd = brain_data.TestBrainData('input_1', 'output', 100.0, final_batch_size=100, post_context=post)
  bd.preserve_test_data(x, y)
  ds = bd.create_dataset('train')
  model = brain_model.BrainModelLinearRegression(ds, regularization_lambda=0.01)
  model.fit(ds)
  w, b = model.weight_matrices
  cov = np.hstack([lagged, np.ones((n, 1))])
  sol = np.linalg.solve(cov.T @ cov / n + 0.01 * np.eye(cov.shape[1]), cov.T @ y.astype(np.float64) / n)
  np.testing.assert_allclose(w, sol[:-1], rtol=2e-4, atol=2e-5)
  np.testing.assert_allclose(np.ravel(b), sol[-1], rtol=2e-4, atol=2e-5)
  pred = model.predict(ds)
  np.testing.assert_allclose(pred, cov @ sol, rtol=1e-4, atol=2e-4)
  ev = model.evaluate(ds)
  assert ev['pearson_correlation_first'] > 0.9
  # the shrinkage branch (use_ridge=False) solves through td_spd_solve, 8 columns at a time
  from oracle import regression as o_reg
  batches = [({'input_1': lagged[i:i + 500].astype(np.float32)}, y[i:i + 500]) for i in range(0, n, 500)]
  ws, bs, _, _, sh = brain_model.calculate_linear_regressor_parameters_from_dataset(
      batches, lamb=0.3, use_ridge=False)
  wr, br, _, _, shr = o_reg.linear_regressor_from_batches(batches, lamb=0.3, use_ridge=False)
  assert sh == shr
  np.testing.assert_allclose(ws, wr, rtol=1e-3, atol=2e-5)
  np.testing.assert_allclose(np.ravel(bs), np.ravel(br), rtol=1e-3, atol=2e-5)


def test_decoder_streaming_api_and_persistence(dev, tmp_path):
  from telluride_decoding_amd import infer_decoder
  g = golden('g5_correlator')
  x, y = g['x'], g['y']
  dec = infer_decoder.Decoder(lambda v: v, reduction='all')
  for s in range(0, x.shape[0], 400):
    dec.add_data_correlator(x[s:s + 400], y[s:s + 400])
  p = dec.correlation_params
  assert p.count == int(g['count'])
  for k in ('sum_x', 'sum_y', 'sum_x2', 'sum_y2', 'mean_x', 'mean_y', 'power'):
    np.testing.assert_allclose(getattr(p, k), g[k], rtol=2e-5)
  np.testing.assert_allclose(dec.compute_correlation(x, y), g['corr'], rtol=2e-5, atol=2e-6)
  np.testing.assert_allclose(np.mean(dec.compute_correlation(g['x64'], g['y64'])) * 0 + 1, 1)
  d64 = infer_decoder.Decoder(lambda v: v)
  for s in range(0, 3000, 300):
    d64.add_data_correlator(g['x64'][s:s + 300].astype(np.float32), g['y64'][s:s + 300].astype(np.float32))
  r = np.mean(d64.compute_correlation(g['x64'].astype(np.float32), g['y64'].astype(np.float32)))
  np.testing.assert_allclose(r, 1, rtol=1e-5)                     # infer_decoder_test.py:191-203
  # windows (average_data) and d'
  gw = golden('g6_windows')
  np.testing.assert_array_equal(infer_decoder.average_data(np.reshape(np.arange(12), (6, 2)), 3),
                                [[2, 3], [8, 9]])                 # infer_decoder_test.py:350-354
  np.testing.assert_allclose(infer_decoder.average_data(gw['avg_in'], 10), gw['avg_out'], rtol=1e-12)
  gl = golden('g8_lda')
  assert abs(infer_decoder.calculate_dprime(gl['dp_d1'], gl['dp_d2']) - float(gl['dp'])) < 1e-12
  # LDA + JSON round trip (infer_decoder_test.py:487-508)
  d1 = infer_decoder.average_data(gl['c0'], 1)
  dprime = dec.compute_lda_model(gl['c0'], gl['c1'])
  np.testing.assert_allclose(dprime, gl['dprime'], rtol=1e-6)
  path = str(tmp_path / 'decoder_model.json')
  dec.save_parameters(path)
  loaded = infer_decoder.Decoder(lambda v: v, reduction='lda')
  loaded.restore_parameters(path)
  np.testing.assert_array_equal(loaded.reduce_with_lda(d1)[:, 0], dec.reduce_with_lda(d1)[:, 0])
  np.testing.assert_allclose(loaded.correlation_params.power, dec.correlation_params.power)
  # errors the reference's tests match on
  with pytest.raises(ValueError, match='Unknown reduction technique'):
    infer_decoder.Decoder(lambda v: v, reduction='bogus')
  with pytest.raises(TypeError, match='Must supply a callable model'):
    infer_decoder.Decoder(3)
  with pytest.raises(ValueError, match='Couldn\'t determine model type'):
    infer_decoder.create_decoder('mystery')
  assert isinstance(infer_decoder.create_decoder('my_linear_model'), infer_decoder.LinearRegressionDecoder)
  assert isinstance(infer_decoder.create_decoder('CCA'), infer_decoder.CCADecoder)


@pytest.mark.gpu
@pytest.mark.parametrize('rows,width,hop', [(120000, 120000, 120000), (65000, 32000, 16000)])
def test_long_window_sums_match_float64(dev, rows, width, hop):
  """Whole-recording windows (the global statistics of infer_decoder.py:288-310): thousands of
  blocks per window go through the wave-per-output reduction."""
  rng = np.random.default_rng(rows)
  a = (rng.standard_normal((rows, 3)) + 0.3).astype(np.float32)
  b = (0.5 * a + rng.standard_normal((rows, 3))).astype(np.float32)
  h = dev.default_handle()
  got = dev.window_sums(h.to_device(a), h.to_device(b), [0, rows], width, hop, handle=h).cpu().numpy()
  n_win = (rows - width) // hop + 1
  assert got.shape == (n_win, 3, 5)
  a64, b64 = a.astype(np.float64), b.astype(np.float64)
  for w in range(n_win):
    s = slice(w * hop, w * hop + width)
    want = np.stack([a64[s].sum(0), b64[s].sum(0), (a64[s] ** 2).sum(0), (b64[s] ** 2).sum(0),
                     (a64[s] * b64[s]).sum(0)], axis=1)
    np.testing.assert_allclose(got[w], want, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('c', [64, 63, 69])
def test_decode_fused_at_full_c4_size(dev, c):
  """BASELINE config C4 at its full size -- 200 DISTINCT trials x 6000 frames x 64 channels, W = 1000,
  hop = 100 -- through td_decode_fused: every one of the 10 200 decisions identical to (and every score
  within 4e-15 of) the unfused kernel chain (FIR prediction -> window sums -> scores -> winner-take-all), and
  ALL 200 trials (10 200 decisions) against the float64 oracle chain with 0 decision flips (VERDICT r4:
  the test checked 16 trials, only bench.py all of them).  The same shape at the reference's own
  channel counts -- 63 (Telluride4, notebook :613) and 69 (doc/DecodingCodelab.md:709): the streamed
  FIR by 4-byte DMA / with the narrow fifth k-step, the accumulate on virtual images -- with a seeded
  subset of 16 trials against the oracle."""
  from telluride_decoding_amd import synth
  h = dev.default_handle()
  n_trials, frames, pre, post, width, hop = 200, 6000, 0, 31, 1000, 100
  trials = synth.make_trials(44, n_trials, frames, c, switch_half=True)
  eeg = np.concatenate([t[0] for t in trials])
  env = np.concatenate([t[1] for t in trials])
  att = np.concatenate([t[2] for t in trials])
  offs = np.arange(n_trials + 1, dtype=np.int64) * frames
  attended = np.where(att > 0.5, env[:, 1:2], env[:, 0:1]).astype(np.float32)
  xd, envd = h.to_device(eeg), h.to_device(env)
  st = dev.LagStats(c, pre, post, d=1)
  st.accumulate(xd, None, h.to_device(attended), offs)
  w, b = st.ridge_solve([0.1])
  w, b = w[0].contiguous(), b[0].contiguous()
  pred = dev.predict_fir(xd, offs, w, b, pre, post, handle=h)
  n = eeg.shape[0]
  corr = []
  for spk in (0, 1):
    s = dev.window_sums(envd[:, spk:spk + 1], pred, [0, n], n, n, handle=h).cpu().numpy()[0, 0]
    corr += [s[0] / n, s[1] / n, np.sqrt((s[2] - s[0] ** 2 / n) * (s[3] - s[1] ** 2 / n)) / n]
  scores, decisions = dev.decode_fused(xd, envd, offs, w, b, pre, post, width, hop, corr, handle=h)
  scores, decisions = scores.cpu().numpy(), decisions.cpu().numpy()
  per_trial = (frames - width) // hop + 1
  assert scores.shape == (n_trials * per_trial, 2) == (10200, 2)
  # (1) all trials: fused == unfused -- the same float64 block sums; the score formula is contracted
  # into fused multiply-adds differently in the two kernels, so a score may differ in its last bits
  # (1 of 10 200 did, by 2.7e-16 relative); the decisions must be identical
  unfused = []
  for spk in (0, 1):
    sums = dev.window_sums(envd[:, spk:spk + 1], pred, offs, width, hop, handle=h)
    want = dev.window_scores(sums, width, 0, 'first', corr[3 * spk], corr[3 * spk + 1],
                             corr[3 * spk + 2], handle=h).cpu().numpy()
    unfused.append(want)
    np.testing.assert_allclose(scores[:, spk], want, rtol=4e-15, atol=1e-19)
  np.testing.assert_array_equal(decisions, scores[:, 0] > scores[:, 1])
  np.testing.assert_array_equal(decisions, unfused[0] > unfused[1])
  # (2) a seeded subset against the oracle chain in float64
  wn, bn = w.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
  subset = (list(range(n_trials)) if c == 64 else
            sorted(np.random.default_rng(4).choice(n_trials, 16, replace=False).tolist()))
  flips = checked = 0
  worst = 0.0
  for ti in subset:
    t = trials[ti]
    p = o_reg.dense_forward(o_lag.lag_matrix(t[0].astype(np.float64), pre, post), wn, bn)
    sc = []
    for spk in (0, 1):
      cor = o_cor.Correlator()
      cor.mean_x, cor.mean_y, cor.power = corr[3 * spk], corr[3 * spk + 1], corr[3 * spk + 2]
      sc.append(o_cor.windowed_means(cor.correlate(t[1][:, spk:spk + 1].astype(np.float64), p),
                                     t[2], width, hop)[0])
    truth = o_att.wta_sequence(sc[0], sc[1])
    got = decisions[ti * per_trial:(ti + 1) * per_trial]
    flips += int(np.sum(got != truth))
    checked += len(truth)
    for spk in (0, 1):
      worst = max(worst, float(np.max(np.abs(scores[ti * per_trial:(ti + 1) * per_trial, spk] - sc[spk]))))
  parity_log.record('decode_fused_full_c4_%dch' % c, windows=10200, checked_vs_oracle=checked, flips=flips,
                    max_score_err=worst)
  assert checked == len(subset) * per_trial and flips == 0
  assert worst <= 1e-5 * np.max(np.abs(scores))


@pytest.mark.parametrize('cols,b_cols,width,hop', [(20, 1, 1000, 1000), (12, 2, 200, 100), (6, 3, 96, 32), (40, 1, 500, 250)])
def test_window_sums_against_a_cycled_truth(dev, cols, b_cols, width, hop):
  """td_window_sums_cycled (round 6): column j of `a` paired with column j % b_cols of `b` -- several models'
  predictions against ONE truth (regression.py:197-214, the lambdas of a sweep as output columns) -- equals
  td_window_sums against the tiled copy of b, bit for bit (the same kernels, the same order of additions)."""
  import torch
  h = dev.default_handle()
  torch.manual_seed(cols)
  lens = [3100, 1250, 2077]
  offs = np.concatenate(([0], np.cumsum(lens)))
  a = torch.randn(sum(lens), cols, device='cuda')
  b = torch.randn(sum(lens), b_cols, device='cuda')
  tiled = b.repeat(1, cols // b_cols).contiguous()
  want = dev.window_sums(a, tiled, offs, width, hop, handle=h)
  got = dev.window_sums(a, b, offs, width, hop, handle=h)
  assert got.shape == want.shape and got.shape[0] > 0
  assert torch.equal(got, want)
  # float64 reference of one window
  k = int(got.shape[0]) // 2
  wo, _ = dev.window_layout(offs, width, hop)
  t = max(i for i in range(len(lens)) if wo[i] <= k)
  r0 = int(offs[t]) + (k - int(wo[t])) * hop
  aa = a[r0:r0 + width].double().cpu().numpy(); bb = tiled[r0:r0 + width].double().cpu().numpy()
  ref = np.stack([aa.sum(0), bb.sum(0), (aa * aa).sum(0), (bb * bb).sum(0), (aa * bb).sum(0)], axis=1)
  np.testing.assert_allclose(got[k].cpu().numpy(), ref, rtol=1e-12, atol=1e-9)


def test_window_sums_cycled_needs_a_common_block(dev):
  """Windows without a common block of >= 32 frames: the cycled form is refused (ValueError), the caller tiles."""
  import torch
  h = dev.default_handle()
  a = torch.randn(500, 4, device='cuda'); b = torch.randn(500, 1, device='cuda')
  with pytest.raises(ValueError):
    dev.window_sums(a, b, [0, 500], 10, 5, handle=h)
