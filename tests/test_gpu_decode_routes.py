"""Every branch of the decode side's launch ladders (decode.hip: td_launch_fir, td_cca_transform; windows.hip:
td_window_sums_cycled, td_decide_step, td_decode_ssd_stream, td_decode_fused), bit for bit against the parent.

The host plans of those ladders (file tables, strip plans, block and window tables, the window-offset upload) have
one definition each and the kernels index the tables by position: a plan that moved without changing gives the
parent's output bit for bit, a wrong `first` or an off-by-one strip does not.  One seeded case per branch, at the
smallest shape that reaches it: recordings of 300, 33 and 1 rows unless a case says otherwise.  Every case runs
twice (assert_array_equal) and the SHA-256 of its output bytes must equal PARENT_SHA256: what the library of the
parent commit 7fffd56 ("Add saved models, the infer driver and a one-call window-size sweep") gave for these seeds
on the MI355X, run once through TD_HOTPATH_LIB.  Accuracy against float64 is test_gpu_decode.py's business.

The branch each case reaches, read from the route conditions (nl = pre + 1 + post; the rows of every input are
contiguous and 16-byte aligned):

td_predict_fir (c, pre, post, d)
  project4        (8, 0, 0, 3)     nl = 1, c % 4 == 0, d <= 32: project_mfma_kernel<4>  (c <= 8)
  project8        (12, 0, 0, 3)    project_mfma_kernel<8>   (c <= 16)
  project16       (20, 0, 0, 3)    project_mfma_kernel<16>  (c <= 32)
  project32       (64, 0, 0, 9)    project_mfma_kernel<32>
  stream          (64, 0, 31, 1)   d = 1, nl <= 64, c <= 128: fir_stream_kernel, 16-byte DMA, one slice
  stream_dw       (63, 0, 31, 1)   rows of 63 floats: the 4-byte DMA form
  stream_k5       (72, 0, 31, 1)   65 .. 80 channels: the channels past 64 as a fifth k-step, one launch
  stream_2ch      (100, 0, 31, 1)  two channel slices (64 + 36), the second adds
  stream_2lag     (64, 0, 36, 1)   37 lags: two lag slices (32 + 5), the second adds
  stream_f32      (64, 0, 31, 1)   accumulate mode 'f32': the float32 matrix instruction
  mfma            (64, 0, 31, 2)   d = 2 keeps it off the streamed kernel: predict_fir_mfma_kernel, one group
  mfma_groups     (64, 0, 31, 20)  80 KB of LDS hold 3 outputs' weights: 7 output groups (grid.y = 7)
  wave32x2        (63, 0, 31, 2)   unaligned rows, d = 2, nl <= 32: predict_fir_wave_kernel<32, 2>
  wave32x1        (130, 3, 4, 1)   c > 128 (not streamed), 8 lags, d = 1: <32, 1>, three channel passes
  wave4x8         (130, 1, 1, 2)   nl <= 4: <4, 8>
  valu            (5, 0, 32, 7)    33 lags, unaligned: predict_fir_kernel<4>, <2> and <1> for 7 outputs

td_predict_fir_per_file (c, pre, post, d)
  per_file        (64, 0, 31, 3)   predict_fir_mfma_kernel in one launch, whole workgroups of strips a recording
  per_file_each   (70, 0, 3, 2)    c > 64: one td_launch_fir per recording (predict_fir_wave_kernel<4, 8>)

td_cca_transform (c1, c2, dims), no context
  cca_stream      (64, 8, 5)       c2 <= 8: cca_project_stream_kernel
  cca_stream_p2   the same with input_offset 2; cca_stream_m3 with -3 (only the rows the call defines are hashed)
  cca_project     (64, 16, 3)      c2 > 8: cca_project_kernel<108>
  cca_fallback    (63, 8, 2)       unaligned first view: neg_mean_rot_kernel twice and two td_launch_fir
  cca_fallback_pre  the same with pre1 = 2 (context on the first view)

td_window_sums / td_window_sums_cycled (cols, width, hop), trials of 1000, 450 and 90 frames
  sums_narrow     (2, 96, 32)      g = 32: block_sums_kernel, window_from_blocks_kernel
  sums_cols       (12, 96, 32)     8 <= cols <= 64: block_sums_cols_kernel
  sums_wide       (2, 2080, 32)    g = 32, width / g = 65 > 64: window_from_blocks_wide_kernel.  No trial of 1000
                                   frames holds a window of 65 blocks of >= 32 frames: this case's first
                                   trial has 2500 frames (14 windows)
  sums_short      (2, 10, 5)       gcd 5, width <= 256: window_sums_short_kernel
  sums_each       (2, 300, 7)      gcd 1, width > 256: window_sums_kernel, a workgroup a window
  sums_cycled     (6, 96, 32), b of 3 columns: block_sums_kernel with a cycled b
  window_means, decide_step with a state vector, decode_ssd with state (the states are hashed too)

td_decode_fused, 64 channels, 32 lags, trials of 600 frames
  fused_chain       4 trials, W = 10 / hop 5:   g = 0 and fewer than 16 trials: the unfused chain
  fused_trial_gcd   16 trials, W = 10 / hop 5:  decode_trial_kernel on blocks of gcd = 5 frames
  fused_trial       16 trials, W = 128 / hop 64: decode_trial_kernel, g = 64
  fused_pair        4 trials, W = 128 / hop 64: block_sums_pair_kernel + decode_finalize_kernel
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS = (300, 33, 1)
TRIALS = (1000, 450, 90)

FIR = {
    'project4': (8, 0, 0, 3), 'project8': (12, 0, 0, 3), 'project16': (20, 0, 0, 3), 'project32': (64, 0, 0, 9),
    'stream': (64, 0, 31, 1), 'stream_dw': (63, 0, 31, 1), 'stream_k5': (72, 0, 31, 1),
    'stream_2ch': (100, 0, 31, 1), 'stream_2lag': (64, 0, 36, 1), 'stream_f32': (64, 0, 31, 1),
    'mfma': (64, 0, 31, 2), 'mfma_groups': (64, 0, 31, 20),
    'wave32x2': (63, 0, 31, 2), 'wave32x1': (130, 3, 4, 1), 'wave4x8': (130, 1, 1, 2), 'valu': (5, 0, 32, 7),
}
FIR_PER_FILE = {'per_file': (64, 0, 31, 3), 'per_file_each': (70, 0, 3, 2)}
# (c1, c2, dims, pre1, input_offset)
CCA = {
    'cca_stream': (64, 8, 5, 0, 0), 'cca_stream_p2': (64, 8, 5, 0, 2), 'cca_stream_m3': (64, 8, 5, 0, -3),
    'cca_project': (64, 16, 3, 0, 0), 'cca_fallback': (63, 8, 2, 0, 0), 'cca_fallback_pre': (63, 8, 2, 2, 0),
}
# (cols, b_cols, width, hop, trials)
SUMS = {
    'sums_narrow': (2, 2, 96, 32, TRIALS), 'sums_cols': (12, 12, 96, 32, TRIALS),
    'sums_wide': (2, 2, 2080, 32, (2500, 450, 90)), 'sums_short': (2, 2, 10, 5, TRIALS),
    'sums_each': (2, 2, 300, 7, TRIALS), 'sums_cycled': (6, 3, 96, 32, TRIALS),
}
# (trials, width, hop)
FUSED = {
    'fused_chain': (4, 10, 5), 'fused_trial_gcd': (16, 10, 5), 'fused_trial': (16, 128, 64),
    'fused_pair': (4, 128, 64),
}

# the parent commit's output: SHA-256 of the bytes of every array a case returns, in order
PARENT_SHA256 = {
    'project4': '95406a2e18a06353aa5c5eb403115b9ea85af3a120be7267ee9b65255a8aea2d',
    'project8': 'aea8b8c2b5240b4c252b820c51a83e0e8437acfac0043bff8542cd7b92aaf0fb',
    'project16': '9d961773361ac13e441827b1a70ed729eb43beeac5025c3557a9fc82f7f3c8ff',
    'project32': '1db7a4e32a55dba68dd397295f69cae35fe9dbb7449b89fe6a948097c7f67735',
    'stream': 'e99f3b9ad39011300be868400ab19eab8aa2a4d8179e5601f302f721b6856c34',
    'stream_dw': '784495df15c1e78d3302346807b7a7438ec467ac75c59511dd1b916112a2dd5e',
    'stream_k5': '9de6515b01601e7b7d1e0ff3fc7283be0d245f26616b181d297a9d4cde77e599',
    'stream_2ch': 'ada30dda47d8696bd495034991f2f3d40494d5f9c180541c4afe0f29e2c13786',
    'stream_2lag': '78f649b345d8e3f923f7b3ea7b85867a0b521bdf2fbad954ee5a666c38ee7423',
    'stream_f32': '1a5b0acdebadcdbf909388e814cf003c8eaa36c59a897d012db00c96bc4b5744',
    'mfma': 'd3d2554a23c45c030ec4a30a21ac3d085fbd713afb81f5c137c35e2ad37d44e9',
    'mfma_groups': '6d2e5417060c520b4391c2f6bdd01bb01001d1c2b62af9d56998e8d14643dea8',
    'wave32x2': '4ccc2488f72bd6510d2fa8a9509741aa6fa406e3b2d1e69ce9d94e924727a993',
    'wave32x1': '773aafd6e33b9e402e42324427198bf8ea7a76192e4953b0769f1c5b061e4a77',
    'wave4x8': '9815df86565764870e1fab43c22403dc0a7c167b3e91c3492b0dca3f7ef6b6cb',
    'valu': '8d948821c27bf3570642fc07bcd20ad14c15565040632c33905b08dc0faa7ef7',
    'per_file': '468b163fe7e6448bda1427173a1ad266eab49497c844c8d0ba69ba0fe99a17a5',
    'per_file_each': 'ac9b2cfd551bb3d8b7a7403869393bc50b861b573dd8748b8a2877eb7c9b537f',
    'cca_stream': 'f9203132fc8b906b9c9fe338b60b7132a65d435adfe3f2524a32a08aebfb0986',
    'cca_stream_p2': '2456ac409d6b8d7a4f2125501036c3c43d2eae84d6b9ae201e862d11c38d5602',
    'cca_stream_m3': '2b6ace7aa0a1f3317dac0cfe6ad4b44d8596066b8a222c6fb730255186961a73',
    'cca_project': 'f6519af9122aaa67d695b11d8530a8f3d1e3abb68602afea6fee53241204bd1e',
    'cca_fallback': 'ee3080d630dda82f210cad9ccf830bb1b0ecb7ad21703f0450c934650c986c4f',
    'cca_fallback_pre': '8899f8db5413e0f54793e5afa92ae97fcb400dd696b09c71ea0836cabdbdf8db',
    'sums_narrow': 'd9e46756ad1449b62c6dab7458df0c1394acfd4c766a4285ab98f4f572baebfa',
    'sums_cols': '83e002273bcc1c50185546eaa9ad2cca55d203cbea54be0a2d0046559f7ec4b5',
    'sums_wide': '119e2a148c0ad7baf733a145d02c9567a3a79dc0c7d1c0e4915230c3d8a0a3e0',
    'sums_short': 'fe35d8bd3ed7676bb11f6f8f146819e0bc896b2cb4eb71321365d0571b4deb10',
    'sums_each': '18d4fdc0366712ea2621489d38a3d6fc5c2d102f9fa1a8d037f0552590e9aa05',
    'sums_cycled': '92e6abfea920900f3ef45486e4f6b2bf6444374ec2dbcb4b6d5fe84484168adf',
    'fused_chain': '5c78882081c22f6f84c2123b39e5b8dfa805c591a034f99d772dae82af32e943',
    'fused_trial_gcd': '4a533abe958f0fe5d2bc94116231389ac7508b744fe99299d0dc504d97a9ae5b',
    'fused_trial': '3f8931c207a14457e1613660abef59c997c81f07f0482dee46e3932c76d06187',
    'fused_pair': 'c99344cc422242ff951e5c1dba5f5a2de7d462e8fedc58f0e702014ef4515178',
    'window_means': 'c12373ec77e1a9e8c31b2d19e96556161e2dd97b35cb608794831b362f157d66',
    'decide_step': '99d85f1fe42bcc598fb470fc627d7ffa95a1a020ac706fd4d0b07dcf13f76923',
    'decode_ssd': '9778a96eba9080a3edd702488dc4312de677be702042816791b827cef27552ea',
}


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _rng(name):
  return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], 'little'))


def _offs(lens):
  return np.concatenate(([0], np.cumsum(lens)))


def _fir(dev, h, name):
  per_file = name in FIR_PER_FILE
  c, pre, post, d = (FIR_PER_FILE if per_file else FIR)[name]
  rng = _rng(name)
  k = c * (pre + 1 + post)
  x = rng.standard_normal((sum(LENS), c)).astype(np.float32)
  shape = (len(LENS), k, d) if per_file else (k, d)
  w = (rng.standard_normal(shape) / np.sqrt(k)).astype(np.float32)
  b = rng.standard_normal(shape[:-2] + (d,)).astype(np.float32)
  xd, wd, bd = h.to_device(x), h.to_device(w), h.to_device(b)
  call = dev.predict_fir_per_file if per_file else dev.predict_fir
  saved = h.accumulate_mode
  outs = []
  try:
    if name == 'stream_f32':
      h.set_accumulate_mode('f32')
    for _ in range(2):
      out = h.zeros((sum(LENS), d), 'float32')
      call(xd, _offs(LENS), wd, bd, pre, post, out=out, handle=h)
      outs.append([out.cpu().numpy()])
  finally:
    h.set_accumulate_mode(saved)
  return outs


def _cca(dev, h, name):
  c1, c2, dims, pre1, off = CCA[name]
  rng = _rng(name)
  n = sum(LENS)
  x = rng.standard_normal((n, c1)).astype(np.float32)
  x2 = rng.standard_normal((n, c2)).astype(np.float32)
  k1 = c1 * (pre1 + 1)
  args = [h.to_device(v) for v in (
      x, x2, (0.1 * rng.standard_normal(k1)).astype(np.float32),
      (rng.standard_normal((k1, dims)) / np.sqrt(k1)).astype(np.float32),
      (0.1 * rng.standard_normal(c2)).astype(np.float32),
      (rng.standard_normal((c2, dims)) / np.sqrt(c2)).astype(np.float32))]
  offs = _offs(LENS)
  dx, dy = max(off, 0), max(-off, 0)
  outs = []
  for _ in range(2):
    out = dev.cca_transform(args[0], args[1], offs, args[2], args[3], args[4], args[5], pre1, 0, 0, 0,
                            handle=h, input_offset=off).cpu().numpy()
    # the rows the call defines: the first n - dx of a recording for the first view, n - dy for the second
    parts = []
    for f, nf in enumerate(LENS):
      a = int(offs[f])
      parts.append(out[a:a + max(nf - dx, 0), :dims].copy())
      parts.append(out[a:a + max(nf - dy, 0), dims:].copy())
    outs.append(parts)
  return outs


def _sums(dev, h, name):
  cols, b_cols, width, hop, trials = SUMS[name]
  rng = _rng(name)
  a = rng.standard_normal((sum(trials), cols)).astype(np.float32)
  b = rng.standard_normal((sum(trials), b_cols)).astype(np.float32)
  ad, bd = h.to_device(a), h.to_device(b)
  outs = [[dev.window_sums(ad, bd, _offs(trials), width, hop, handle=h).cpu().numpy()] for _ in range(2)]
  assert outs[0][0].shape[0] > 0
  return outs


def _scores(dev, h, name, width, hop):
  """Two float64 score streams over TRIALS' windows and their window offsets."""
  rng = _rng(name)
  wo, total = dev.window_layout(_offs(TRIALS), width, hop)
  s = [h.to_device(rng.standard_normal(total), np.float64) for _ in range(2)]
  return s[0], s[1], wo


def _window_means(dev, h, name):
  v = h.to_device(_rng(name).standard_normal(sum(TRIALS)), np.float64)
  return [[dev.window_means(v, _offs(TRIALS), 96, 32, handle=h).cpu().numpy()] for _ in range(2)]


def _decide_step(dev, h, name):
  s1, s2, wo = _scores(dev, h, name, 10, 5)
  outs = []
  for _ in range(2):
    out, st = dev.decide_step(s1, s2, wo, state=np.array([0.25, 0.5, 0.75]), handle=h)
    outs.append([out.cpu().numpy(), st])
  return outs


def _decode_ssd(dev, h, name):
  s1, s2, wo = _scores(dev, h, name, 96, 32)
  outs = []
  for _ in range(2):
    state = dev.ssd_state(len(TRIALS), handle=h)
    out = dev.decode_ssd(s1, s2, wo, outer_iter=3, handle=h, state=state)
    outs.append([out.cpu().numpy(), state.cpu().numpy()])
  return outs


def _fused(dev, h, name):
  n_trials, width, hop = FUSED[name]
  c, post, n = 64, 31, 600
  rng = _rng(name)
  eeg = h.to_device(rng.standard_normal((n_trials * n, c)).astype(np.float32))
  env = h.to_device(rng.standard_normal((n_trials * n, 2)).astype(np.float32))
  w = h.to_device((rng.standard_normal((c * (post + 1), 1)) / np.sqrt(c * (post + 1))).astype(np.float32))
  b = h.to_device(rng.standard_normal(1).astype(np.float32))
  corr = [0.1, 0.05, 1.2, -0.1, 0.02, 0.9]
  outs = []
  for _ in range(2):
    scores, dec = dev.decode_fused(eeg, env, _offs((n,) * n_trials), w, b, 0, post, width, hop, corr, handle=h)
    outs.append([scores.cpu().numpy(), dec.cpu().numpy()])
  assert outs[0][1].shape[0] > 0
  return outs


RUNNERS = {}
for _table, _fn in ((FIR, _fir), (FIR_PER_FILE, _fir), (CCA, _cca), (SUMS, _sums), (FUSED, _fused)):
  for _name in _table:
    RUNNERS[_name] = _fn
RUNNERS.update(window_means=_window_means, decide_step=_decide_step, decode_ssd=_decode_ssd)


@pytest.mark.parametrize('name', list(RUNNERS))
def test_route_gives_the_parents_bytes(dev, name):
  first, second = RUNNERS[name](dev, dev.default_handle(), name)
  assert len(first) == len(second)
  sha = hashlib.sha256()
  for u, v in zip(first, second):
    np.testing.assert_array_equal(u, v)
    sha.update(np.ascontiguousarray(u).tobytes())
  print('ROUTE %s %s' % (name, sha.hexdigest()))
  assert sha.hexdigest() == PARENT_SHA256[name]
