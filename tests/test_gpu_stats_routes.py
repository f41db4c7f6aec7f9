"""Every branch of the statistics' host code (stats.hip, stats_accumulate.hip, stats_moments.hip, stats_exchange.hip:
the route ladder of td_stats_accumulate_ranges, accumulate_fused, td_stats_accumulate_each, the expansion and the
exchange), bit for bit against the parent.

The accumulate has no floating-point atomics: the matrix kernels leave partial slabs, the finalize launch sums them in
float64 in a fixed order.  Host code that moved without changing (segments, window jobs, the finalize description,
scratch offsets, the channel-table phase) gives the parent's bytes; a wrong `first_slot`, a block range off by one or a
table cleared at the wrong call does not.  One seeded case per branch, at the smallest shape that reaches it:
recordings of 300, 33 and 1 rows ("A"; a second set "B" of 120 and 7 rows for the calls that accumulate onto
statistics that already hold files) unless a case says otherwise.  Every case runs twice on objects of its own
(assert_array_equal) and the SHA-256 of its output must equal PARENT_SHA256: what the library of the parent commit
2e8bf1d ("State the online push wrappers' and banks' shared host code once") gave for these seeds on the MI355X, run
once through TD_HOTPATH_LIB.  The output of a case is what td_stats_pack writes (the sums and both window arrays) and
(frames, files), for every statistics object of the case.  Accuracy against float64 is
test_gpu_fit.py::test_moments_match_dense_lag_matrix's business.  (The strips of the targets kernel follow the
handle's CU count: the table belongs to the whole chip.)

The branch each case reaches, read from the route conditions and the planners.  Shapes are (c1, pre, post, d);
l1 = pre + 1 + post; parts: 1 MAIN, 2 TARGETS, 4 TARGETS_FIRST, 8 DEFER.

Fused route (stats_fusable: c2 = 0, 1 <= d <= 4, c1 <= 64, l1 <= 32; new_frames > 0)
  n16_both        (16, 0, 3, 1)    td_narrow16_plan: c <= 16, l1 <= 16, d <= 4: one streaming kernel, parts 3
  n16_apart       the same, MAIN then TARGETS (two narrow16 launches, two finalize launches)
  n16_onto        the same, A then B: the second call adds to the sums and appends its windows
  virt            (21, 0, 31, 1)   td_lagcov_virt_plan `narrow` (9 .. 32 channels, l >= 5): the targets pass measures
                                   the channel maxima (pre = 0)
  virt_pre        (21, 2, 9, 1)    a pre-context: nobody measured, td_chan_max_works into a scratch table (own_tab)
  virt_mid_d4     (40, 0, 9, 4)    td_lagcov_virt_plan `mid` (33 .. 64 channels that are not whole aligned 64-channel
                                   rows), four target columns: five reductions in the finalize launch
  plain           (64, 0, 31, 1)   aligned 64-channel rows: td_lagcov_plan, float16 kernel, maxima from the targets pass
  plain_pre       (64, 16, 15, 1)  a pre-context: the lag kernel measures for itself
  plain_d4        (64, 0, 9, 4)    four target columns on the plain plan
  plain_f32, plain_bf16x3          (64, 0, 31, 1) under accumulate modes 'f32' and 'bf16x3' (no channel table)
  tfirst          TARGETS | TARGETS_FIRST, then MAIN: the maxima travel in the statistics' own table (`ahead`)
  defer_ahead     TARGETS | TARGETS_FIRST, then MAIN | DEFER, then td_stats_complete: the deferred finalize reads the
                  statistics' table and zeroes nothing: can_wait
  defer_own       MAIN | TARGETS | DEFER, then td_stats_complete: the call measures into the HANDLE's table; the lag
                  kernel copies the scales into the statistics' dscale block and zeroes the next table itself
                  (mp.scale_out / mp.zero_tab), so that no reduction of the pending launch points into the handle's
                  table -- the condition under which can_wait would be false
  rows_used       (64, 0, 31, 1) with rows_used (288, 32, 0): N' below the file length, one file without rows
  offset_p2, offset_m3             input_offset 2 and -3 (the 1-row recording has no rows left)
  ranges          time ranges (0, 150), (10, 33), (0, 1) with edge flags 1, 2, 3: the tail of the first recording and
                  the head of the second belong to another rank
  all_empty       rows_used (0, 0, 0): new_frames = 0 sends fusable statistics down the general ladder

td_stats_accumulate_each (64, 0, 31, 1), three recordings
  each            handled = 1; every recording's statistics are hashed
  refusals (test_accumulate_each_refusals, the code only): -1 an object that holds files, -2 the same object twice,
  -3 a narrow16 shape (16, 0, 3, 1), -4 a virtual-image shape (21, 0, 31, 1)

One-pass Gram (stats_one_pass: c2 > 0, d = 0, l1 = l2 = 1, c1 <= 64, c2 <= 31), c1 = 64, c2 = 8
  gram            fresh statistics: the reduction overwrites (gram_fresh)
  gram_onto       A then B: the second call adds
  gram_apart      MAIN, then TARGETS (which has nothing left to add)

General main (c1, pre1, post1, d | c2, pre2, post2)
  tiles69         (69, 0, 36, 1)   65 .. 128 channels, <= 64 lags, mode 'f16x2': lagcov_auto hands the call to
                                   td_lagcov_virt (`wide`); 37 lags: the targets in a window of 32 lags from lag 0
                                   and td_lagcov_column for the 5 lags after it
  tiles100        (100, 0, 3, 1)   the same, four blocks of 32 channels
  pairs69_bf16x3  (69, 0, 36, 1)   under 'bf16x3' td_lagcov_virt_plan refuses: the tile pairs of lagcov_auto itself
                                   (gather_tile_pair_kernel, td_lagcov, scatter_tile_pair_kernel), 3 passes
  pairs100_f32    (100, 0, 3, 1)   under 'f32': 6 passes
  wide130         (130, 0, 3, 1)   above 128 channels: td_lagcov
  cca_column      (64, 0, 7, 0 | 1, 5, 0)   one-column second view: td_lagcov_column twice, operands swapped
  cca_swapped     (64, 0, 7, 0 | 4, 5, 0)   c2 <= 8 < c1: swapped segments, added back reversed and transposed
  cca_direct      (64, 0, 7, 0 | 12, 5, 0)  c2 > 8: the direct cross-covariance
  cca_range       cca_swapped's shape under ranges with u_begin != 0: direct
  (all four: the second view's ones rows from the targets kernel, pre2 = 5 <= 31)
  cca_pre33       (64, 0, 3, 0 | 4, 33, 0)  pre2 > 31: the second view's ones rows on the skinny kernel

General targets
  d12_c6          (6, 0, 3, 12)    d > 4, c1 <= 8: swapped operands; the ones rows from the d = 0 targets call
  d12_c20         (20, 0, 3, 12)   d <= 16, l1 <= 32: slices of four columns
  d20_c6          (6, 0, 3, 20)    swapped operands, the targets kernel handles the ones row
  d20_c6_pre33    (6, 33, 0, 20)   pre > 31: the ones row on the skinny kernel, td_colsum
  d20_c20         (20, 0, 3, 20)   neither special form: the skinny kernel on [y | 1], td_colsum
  tiles69 (above) 33+ lags, after > 0
  before69        (69, 33, 3, 1)   33+ lags with pre > 31: before > 0

Edge cases: all_empty (above); no_files: num_files = 0 leaves fresh statistics as they are.

Moved, not rewritten: moments_2 / moments_5 (td_stats_moments of 2 and 5 recordings, either side of
kExpandFusedFiles; xtx and xty are hashed), combine (three sources), pack_unpack (pack -> unpack into an object of
the same layout -> pack).
"""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS_A = (300, 33, 1)
LENS_B = (120, 7)

# name: ((c1, pre1, post1, d), (c2, pre2, post2), accumulate mode, steps); a step is 'complete' or
# (data set, parts, keyword arguments of LagStats.accumulate)
_N16, _V21, _P64 = (16, 0, 3, 1), (21, 0, 31, 1), (64, 0, 31, 1)
_RANGES = dict(ranges=[(0, 150), (10, 33), (0, 1)], edges=[1, 2, 3])
_GRAM = ((64, 0, 0, 0), (8, 0, 0))
ACC = {
    'n16_both': (_N16, None, None, [('A', 3, {})]),
    'n16_apart': (_N16, None, None, [('A', 1, {}), ('A', 2, {})]),
    'n16_onto': (_N16, None, None, [('A', 3, {}), ('B', 3, {})]),
    'virt': (_V21, None, None, [('A', 3, {})]),
    'virt_pre': ((21, 2, 9, 1), None, None, [('A', 3, {})]),
    'virt_mid_d4': ((40, 0, 9, 4), None, None, [('A', 3, {})]),
    'plain': (_P64, None, None, [('A', 3, {})]),
    'plain_pre': ((64, 16, 15, 1), None, None, [('A', 3, {})]),
    'plain_d4': ((64, 0, 9, 4), None, None, [('A', 3, {})]),
    'plain_f32': (_P64, None, 'f32', [('A', 3, {})]),
    'plain_bf16x3': (_P64, None, 'bf16x3', [('A', 3, {})]),
    'tfirst': (_P64, None, None, [('A', 2 | 4, {}), ('A', 1, {})]),
    'defer_ahead': (_P64, None, None, [('A', 2 | 4, {}), ('A', 1 | 8, {}), 'complete']),
    'defer_own': (_P64, None, None, [('A', 3 | 8, {}), 'complete']),
    'rows_used': (_P64, None, None, [('A', 3, dict(rows_used=[288, 32, 0]))]),
    'offset_p2': (_P64, None, None, [('A', 3, dict(input_offset=2))]),
    'offset_m3': (_P64, None, None, [('A', 3, dict(input_offset=-3))]),
    'ranges': (_P64, None, None, [('A', 3, _RANGES)]),
    'all_empty': (_P64, None, None, [('A', 3, dict(rows_used=[0, 0, 0]))]),
    'no_files': (_P64, None, None, [('A', 3, dict(no_files=True))]),
    'gram': _GRAM + (None, [('A', 3, {})]),
    'gram_onto': _GRAM + (None, [('A', 3, {}), ('B', 3, {})]),
    'gram_apart': _GRAM + (None, [('A', 1, {}), ('A', 2, {})]),
    'tiles69': ((69, 0, 36, 1), None, None, [('A', 3, {})]),
    'tiles100': ((100, 0, 3, 1), None, None, [('A', 3, {})]),
    'pairs69_bf16x3': ((69, 0, 36, 1), None, 'bf16x3', [('A', 3, {})]),
    'pairs100_f32': ((100, 0, 3, 1), None, 'f32', [('A', 3, {})]),
    'wide130': ((130, 0, 3, 1), None, None, [('A', 3, {})]),
    'cca_column': ((64, 0, 7, 0), (1, 5, 0), None, [('A', 3, {})]),
    'cca_swapped': ((64, 0, 7, 0), (4, 5, 0), None, [('A', 3, {})]),
    'cca_direct': ((64, 0, 7, 0), (12, 5, 0), None, [('A', 3, {})]),
    'cca_range': ((64, 0, 7, 0), (4, 5, 0), None, [('A', 3, _RANGES)]),
    'cca_pre33': ((64, 0, 3, 0), (4, 33, 0), None, [('A', 3, {})]),
    'd12_c6': ((6, 0, 3, 12), None, None, [('A', 3, {})]),
    'd12_c20': ((20, 0, 3, 12), None, None, [('A', 3, {})]),
    'd20_c6': ((6, 0, 3, 20), None, None, [('A', 3, {})]),
    'd20_c6_pre33': ((6, 33, 0, 20), None, None, [('A', 3, {})]),
    'd20_c20': ((20, 0, 3, 20), None, None, [('A', 3, {})]),
    'before69': ((69, 33, 3, 1), None, None, [('A', 3, {})]),
}

# the parent commit's output: SHA-256 of the bytes of every array a case returns, in order
PARENT_SHA256 = {
    'n16_both': '095fa5e43789fbc3d81cd08ad9e082d27362c8e09e0caca6c3f4cfa9891c14c5',
    'n16_apart': '0e3a9d39146f45682dfc79bb9900d20d04d347c39857e5a63275786824a2b42a',
    'n16_onto': '97c982d4431985f1edd08c96cd37bd4742b522e74bf8ca01475c28492d02c103',
    'virt': '253b9f8400514b383c5fd47160861ebf4b4d43b91dfb0a9ee0a3337c299ec72a',
    'virt_pre': 'd29ab3d6c47a479838c6bd1711c6a05bc0afe81b2ec425b7358404101a26a625',
    'virt_mid_d4': '9809ae8767f18b9b90144e75629e76aa119669f7efe2436e96cc41a398e0a90a',
    'plain': '0862732d629062794f1d9f82a7f9764b6b27c42e85a6c89503a24f51c2e19737',
    'plain_pre': '3151dfd0852c0bff62b09d03ebe4b4a34d26cb8e36034d31d60fdff43cf911b1',
    'plain_d4': 'fc303c54070d4e719a8f0bf05053e717037d1e523f91a751ee24b2ee81a03ac5',
    'plain_f32': '9f5a227399cdf79d0fb8f2936a2137ce2bdecec01b5f6c502dc272c1cdbd6722',
    'plain_bf16x3': '4b8c645cf37197688bd271cb58391197ae406e433e83a47816c300dd016377e6',
    'tfirst': '7df7f3d16ee777783faac779ad40609e61aa800318e5d75b3e4a785a8e82e3f3',
    'defer_ahead': '08cd93d3fb4e0dd39ad82e26915776ed83cbf909d369a6a80c0008ab4d65ea51',
    'defer_own': '586e70a8c091ff1661bb2d2447acff748ce58dc6c35691c76baeadd669a406ac',
    'rows_used': '797dc2d846a676cbbd6b64d4797a848286a8b1e92a4deebb0fde43a42d6bc3d1',
    'offset_p2': '24dc27b564150b1727407c6f7b2592f01c62876211551dd57512475998094f4d',
    'offset_m3': '222cc4317479219ceee343ad31abd4376e6442e86a505cf2bc1e26ec03a7c673',
    'ranges': 'ef49e0bceb278cff61d2481aa218c5791438862259c19c1443cb53843be250da',
    'all_empty': '5ae2d7f7d58fe4a6066637cb33e43a8a7c52ab85ef61ca27d12968211692b819',
    'no_files': 'a86458cd4a9731d188b32d99ad7748fc5a22a6f03415643aad9668b87c571c08',
    'gram': '1a0768ef9eb5682fc61dbb0cb48f4bfc8ac989fb6947a9f6503d1e5c6a14f072',
    'gram_onto': '50641974466ea722740996dc6eb897c27d295a31d5e0b71adb4f7397646c7d8d',
    'gram_apart': '203306bcde6bc199adac8747a9ad834e922c1d534e075a4877cb1399606790ea',
    'tiles69': '578f16230b1f742fb4e8db28dbcf915bd7ba15edce9de38615ff09bfab9731b6',
    'tiles100': '05515f249829dd59aacc1cc3bc5a85d43a95bb50e3a39fa72b6b54a6bcab6634',
    'pairs69_bf16x3': 'da1beb194177841d2563fa3621edb8044506f1de7bcdf1c323bf254fa493ae31',
    'pairs100_f32': '1f5041100ca156049f83f39bc3d3ab5f3b00d523fbe36c04d99d5dfeecc437d1',
    'wide130': '48a30bd1a6210b50fe40a237902db7f566217e83b3b5f9d740ab6935c26a5516',
    'cca_column': '322c75c5bb95413bdb233e866261e8b2ae739165edf9942755dfc04f5f8cf5c9',
    'cca_swapped': 'ccafd456b4a072dbaae78c851d0a14957c514682f8fa7547f59d3ada618b8d42',
    'cca_direct': '9b86a4088b21120fd28758abbe8671960397224b9964c287eedde591faecba83',
    'cca_range': '0650a58f3ac0831482376e037fa2403df9f627376d1bfeab3a15b49e9341ea6a',
    'cca_pre33': '1545b77f20b0dd554372071c023c0864b3c041971f5f24c307186fdb63673f79',
    'd12_c6': '54209303fa68ec3f781ef78adcb3930deab254b3c606dbabf07fc35fd0248406',
    'd12_c20': '0524e5a87db253e5b5ff4201a2695ac5d59fef2c9ab9ff9cf8ff723365071c2d',
    'd20_c6': '6a0a3fdea0c88d32ebfb2ba62fc79507c732e189977111080ff41d416cc683ed',
    'd20_c6_pre33': '1059673c38605a07f925c4deea2f30763ddcca307b4676056a5cee28c431aeb8',
    'd20_c20': 'c5e199fdc1f04143bab97e18207a6c732397427de1359c31a28e29c11099ce00',
    'before69': '475b27b3eb18651f90f7146af531b0f263018ff3eb0a1dad914aed5c3d37fccb',
    'each': '79f98841c6beffec6251c6e96e826c6af2e8fa71a01f3a59f03e05ecfb461267',
    'moments_2': 'a137282f496e20b5af67df938172a3538f32b89e07a3363c398030607be10604',
    'moments_5': 'ce06ad4649ee0b8aa0b4510d613efc2aa056af08bc2aeba606df747fe7d3b4e4',
    'combine': '58e5d596bc1ea6eaab10fc9dc73e788922cdac4c5490274be3e42871ea155eac',
    'pack_unpack': 'b633659458aca51785ef9a90c71996a8178c7757c4d6d3b0085880e22d0037f2',
}

# the refusals of td_stats_accumulate_ranges in the order the parent reports them: (what is wrong, the message)
MESSAGES = [
    ('null_stats', 'td_stats_accumulate: NULL argument'),
    ('one_range_array', 'td_stats_accumulate_ranges: give both range arrays or neither'),
    ('ranges_with_offset', 'td_stats_accumulate_ranges: time ranges need input_offset = 0'),
    ('parts_5', 'td_stats_accumulate_parts: parts must be 1, 2, 3 or TD_ACC_TARGETS | TD_ACC_TARGETS_FIRST'),
    ('defer_targets', 'td_stats_accumulate_parts: TD_ACC_DEFER goes with TD_ACC_MAIN (| TD_ACC_TARGETS)'),
    ('tfirst_cca',
     'td_stats_accumulate_parts: TARGETS_FIRST is for regression statistics (targets, no second input)'),
    ('null_x', 'td_stats_accumulate: NULL input'),
    ('small_ldx', 'ldx (63) < channels (64)'),
    ('null_x2', 'input_2 missing or ldx2 too small'),
    ('null_y', 'y missing or ldy too small'),
    ('decreasing_offsets', 'file_offsets must be non-decreasing'),
    ('rows_used_301', 'rows_used[0] = 301 outside [0, 300]'),
    ('range_past_end', 'range [10, 34) of file 1 outside [0, 33]'),
    ('targets_before_main', 'td_stats_accumulate_parts: TARGETS before MAIN (say TD_ACC_TARGETS_FIRST)'),
    ('tfirst_empty', 'td_stats_accumulate_parts: TARGETS_FIRST needs the fused accumulate path'),
    # two bad arguments: the one checked first is reported
    ('one_range_array+parts_5', 'td_stats_accumulate_ranges: give both range arrays or neither'),
    ('small_ldx+rows_used_301', 'ldx (63) < channels (64)'),
]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


def _rng(name):
  return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], 'little'))


def _offs(lens):
  return np.concatenate(([0], np.cumsum(lens)))


def _data(h, rng, lens, c1, c2, d):
  """x (channels of uneven scale), x2, y of the recordings `lens` on the device."""
  n = sum(lens)
  x = (rng.standard_normal((n, c1)) * np.logspace(-1, 1, c1)).astype(np.float32)
  x2 = rng.standard_normal((n, c2)).astype(np.float32) if c2 else None
  y = (x[:, :1] * 0.3 + rng.standard_normal((n, d))).astype(np.float32) if d else None
  return tuple(None if v is None else h.to_device(v) for v in (x, x2, y)) + (_offs(lens),)


def _packed(st):
  """What td_stats_pack writes and (frames, files)."""
  frames, files = st.counts()
  return [st.pack(files, 0).cpu().numpy(), np.array([frames, files], np.int64)]


def _accumulate(dev, h, name):
  (c1, pre1, post1, d), second, mode, steps = ACC[name]
  c2, pre2, post2 = second or (0, 0, 0)
  rng = _rng(name)
  sets = {'A': _data(h, rng, LENS_A, c1, c2, d), 'B': _data(h, rng, LENS_B, c1, c2, d)}
  saved = h.accumulate_mode
  outs = []
  try:
    if mode:
      h.set_accumulate_mode(mode)
    for _ in range(2):
      st = dev.LagStats(c1, pre1, post1, c2, pre2, post2, d, handle=h)
      st.reset()
      for step in steps:
        if step == 'complete':
          st.complete()
          continue
        which, parts, kw = step
        x, x2, y, offs = sets[which]
        kw = dict(kw)
        if kw.pop('no_files', False):
          offs = offs[-1:]
        st.accumulate(x, x2, y, offs, parts=parts, **kw)
      outs.append(_packed(st))
  finally:
    h.set_accumulate_mode(saved)
  return outs


def _each(dev, h, name):
  c, pre, post, d = _P64
  x, _, y, offs = _data(h, _rng(name), LENS_A, c, 0, d)
  outs = []
  for _ in range(2):
    each = [dev.LagStats(c, pre, post, d=d, handle=h) for _ in LENS_A]
    for st in each:
      st.reset()
    assert dev.LagStats.accumulate_each(each, x, y, offs)
    assert dev.LagStats.last_each_status == 1
    outs.append([a for st in each for a in _packed(st)])
  return outs


def _moments(dev, h, name):
  lens = {'moments_2': (300, 33), 'moments_5': (300, 33, 1, 120, 7)}[name]
  c, pre, post, d = 64, 2, 5, 1
  x, _, y, offs = _data(h, _rng(name), lens, c, 0, d)
  st = dev.LagStats(c, pre, post, d=d, handle=h)
  st.accumulate(x, None, y, offs)
  outs = []
  for _ in range(2):
    m = st.moments()
    outs.append([m['xtx'].cpu().numpy(), m['xty'].cpu().numpy()])
  return outs


def _exchange(dev, h, name):
  c, pre, post, d = 64, 2, 5, 1
  rng = _rng(name)
  srcs = []
  for lens in (LENS_A, LENS_B, (50,)):
    x, _, y, offs = _data(h, rng, lens, c, 0, d)
    st = dev.LagStats(c, pre, post, d=d, handle=h)
    st.accumulate(x, None, y, offs)
    srcs.append(st)
  outs = []
  for _ in range(2):
    dst = srcs[0].like()
    if name == 'combine':
      dst.combine(srcs)
    else:
      frames, files = srcs[0].counts()
      dst.unpack(srcs[0].pack(files + 2, 1), files + 2, total_frames=frames)
    outs.append(_packed(dst))
  return outs


RUNNERS = {name: _accumulate for name in ACC}
RUNNERS.update(each=_each, moments_2=_moments, moments_5=_moments, combine=_exchange, pack_unpack=_exchange)


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


def test_accumulate_each_refusals(dev):
  """handled = -1 .. -4 of td_stats_accumulate_each: nothing is queued, the caller goes file by file."""
  h = dev.default_handle()

  def status(shape, prepare=None, twice=False):
    c, pre, post, d = shape
    x, _, y, offs = _data(h, _rng('each_refusals'), LENS_A, c, 0, d)
    each = [dev.LagStats(c, pre, post, d=d, handle=h) for _ in LENS_A]
    for st in each:
      st.reset()
    if prepare:
      each[1].accumulate(x, None, y, offs)
    if twice:
      each[2] = each[0]
    assert not dev.LagStats.accumulate_each(each, x, y, offs)
    return dev.LagStats.last_each_status

  assert status(_P64, prepare=True) == -1
  assert status(_P64, twice=True) == -2
  assert status(_N16) == -3
  assert status(_V21) == -4


def test_accumulate_refusals_word_for_word(dev):
  """The messages of td_stats_accumulate_ranges and which of two bad arguments is reported (MESSAGES)."""
  from telluride_decoding_amd import _lib
  h = dev.default_handle()
  x, x2, y, offs = _data(h, _rng('messages'), LENS_A, 64, 4, 1)
  reg = dev.LagStats(64, 0, 31, d=1, handle=h)
  cca = dev.LagStats(64, 0, 3, 4, 2, 0, handle=h)
  i64 = lambda v: _lib.i64_array(v)
  ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

  def call(wrong):
    a = dict(st=reg, x=x, ldx=64, x2=None, ldx2=0, y=y, ldy=1, offs=list(offs), off=0, used=None, rb=None, re=None,
             parts=3)
    for w in wrong.split('+'):
      if w == 'null_stats': a['st'] = None
      elif w == 'one_range_array': a['rb'] = [0, 0, 0]
      elif w == 'ranges_with_offset': a.update(rb=[0, 0, 0], re=[1, 1, 1], off=1)
      elif w == 'parts_5': a['parts'] = 5
      elif w == 'defer_targets': a['parts'] = 2 | 8
      elif w == 'tfirst_cca': a.update(st=cca, x2=x2, ldx2=4, y=None, ldy=0, parts=2 | 4)
      elif w == 'null_x': a['x'] = None
      elif w == 'small_ldx': a['ldx'] = 63
      elif w == 'null_x2': a.update(st=cca, y=None, ldy=0)
      elif w == 'null_y': a['y'] = None
      elif w == 'decreasing_offsets': a['offs'] = [0, 300, 299, 334]
      elif w == 'rows_used_301': a['used'] = [301, 33, 1]
      elif w == 'range_past_end': a.update(rb=[0, 10, 0], re=[150, 34, 1])
      elif w == 'targets_before_main': a['parts'] = 2
      elif w == 'tfirst_empty': a.update(parts=2 | 4, used=[0, 0, 0])
      else: raise KeyError(w)
    keep = [i64(a['offs'])] + [i64(a[k]) if a[k] is not None else (None, None) for k in ('used', 'rb', 're')]
    a['st'] is None or a['st'].reset()
    return h.lib.td_stats_accumulate_ranges(
        h.ptr, a['st'].ptr if a['st'] is not None else ctypes.c_void_p(0), ptr(a['x']), a['ldx'], ptr(a['x2']),
        a['ldx2'], ptr(a['y']), a['ldy'], keep[0][1], len(a['offs']) - 1, a['off'], keep[1][1], keep[2][1],
        keep[3][1], None, a['parts'])

  for wrong, message in MESSAGES:
    with pytest.raises(ValueError) as err:
      h.check(call(wrong))
    assert str(err.value) == message, wrong
  for st in (reg, cca):
    assert st.counts() == (0, 0)
