"""The online audio front end without a GPU: the ctypes prototypes of td_audio_online_* against the header,
td_audio_online_plan against a restatement by counting, online.host_audio_plan and tests/host_audio.windows_loop on
the whole recording over rates, windows, lengths and cuts, the bound K on the carried rows by brute force, the state
size, every refusal by name, online.OnlineAudioFeatures' NumPy session -- cut into pushes every way, against
HostAudioFeatures(exact=True).compute_intensity(whole), as a bank, flushed and reset -- and online.FrameJoin."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online_audio as hoa
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_audio_online_plan', 'td_audio_online_push', 'td_audio_online_state_bytes']
LARGE = [20011, 48000 + 777]


def test_argtypes_match_the_header_prototypes():
  """td_audio_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py); the family stays out of the closed td_online_*,
  td_cca_online_* and td_fc_online_* sets; the header's limits are the module's."""
  from telluride_decoding_amd import _lib, device
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_audio_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert not re.fullmatch(r'td_(online|cca_online|fc_online)_\w+', name)
    assert name in _lib.header_symbols()
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
  for macro, value in (('TD_AUDIO_ONLINE_MAX_CHANNELS', device.AUDIO_ONLINE_MAX_CHANNELS),
                       ('TD_AUDIO_ONLINE_MAX_TAIL', device.AUDIO_ONLINE_MAX_TAIL),
                       ('TD_AUDIO_X_I16', device.AUDIO_X_TYPES['int16']),
                       ('TD_AUDIO_X_F32', device.AUDIO_X_TYPES['float32']),
                       ('TD_AUDIO_X_F64', device.AUDIO_X_TYPES['float64'])):
    found = re.search(r'#define\s+%s\s+(\d+)' % macro, raw)
    assert found and int(found.group(1)) == value, macro
  assert (device.AUDIO_ONLINE_MAX_CHANNELS, device.AUDIO_ONLINE_MAX_TAIL) == (8, 8192)


def _random_cut(total, rng, most):
  sizes = []
  while sum(sizes) < total:
    sizes.append(int(min(rng.integers(0, most), total - sum(sizes))))
  return sizes


def _walk(sizes, fs_in, fs_out, window, k, checks):
  """One cut through td_audio_online_plan, a flush of its own behind it: the clamped windows of the emitted frames
  in order, with every plan checked against the restatements on the way."""
  from telluride_decoding_amd import device, online
  windows, at, frames = [], 0, 0
  for j, n in enumerate(list(sizes) + [0]):
    flush = j == len(sizes)
    plan = device.audio_online_plan(at, n, fs_in, fs_out, window, flush)
    assert tuple(plan) == online.host_audio_plan(at, n, fs_in, fs_out, window, flush), (at, n, flush)
    assert plan.tail_rows == k
    assert plan.frames_before == frames, (at, n)                       # (monotone: what was emitted stays emitted)
    assert plan.frames_before <= plan.frames_after <= hoa.frames_of(at + n, fs_in, fs_out), (at, n, plan)
    assert plan.held == hoa.frames_of(at + n, fs_in, fs_out) - plan.frames_after
    if checks:
      assert plan.frames_after == hoa.brute_emitted(at + n, fs_in, fs_out, window, flush), (at, n, flush)
    for i in range(plan.frames_before, plan.frames_after):
      a, u = hoa.raw_window(i, fs_in, fs_out, window)
      assert flush or u <= at + n                                      # (a pushed frame's clamp never acts)
      assert max(0, a) >= at - k, (i, a, at, k)                         # (and it reaches no further back than the tail)
      windows.append((max(0, a), min(at + n, u)))
    at, frames = at + n, plan.frames_after
    if not flush:                                                      # the rows the next push may need: at most K
      a, _ = hoa.raw_window(frames, fs_in, fs_out, window)
      assert at - max(0, a) <= k, (at, frames, a, k)
  return np.array(windows, np.int64).reshape(-1, 2)


@pytest.mark.parametrize('fs_in,fs_out,window', hoa.PLAN_CASES, ids=hoa.PLAN_IDS)
def test_plan_emits_the_whole_recordings_windows_over_any_cut(fs_in, fs_out, window):
  """N in 0..400 and a few large values; one-row pushes (every N on the way is a prefix: monotone, never above
  F(N), the brute-force count, online.host_audio_plan's tuple) and seeded random cuts with empty pushes; a flush at
  every N in 0..400.  The windows of the emitted frames, in order, are tests/host_audio.windows_loop of the whole
  recording; the rows a push may need never exceed K, walked row by row to 4 K + 50."""
  from telluride_decoding_amd import device, online
  from tests import host_audio as ha
  k = hoa.tail_rows(fs_in, fs_out, window)
  assert k == online.audio_tail_rows(fs_in, fs_out, window)
  rng = np.random.default_rng(int(fs_in + 7 * fs_out + 100 * window))
  whole = lambda n: ha.windows_loop(n, 0, hoa.frames_of(n, fs_in, fs_out), fs_in, fs_out, window)
  got = _walk([1] * 400, fs_in, fs_out, window, k, True)
  np.testing.assert_array_equal(got, whole(400))
  for n in range(0, 401):                          # a flush at every N: exactly the whole recording's windows
    pushed = device.audio_online_plan(0, n, fs_in, fs_out, window, False).frames_after
    plan = device.audio_online_plan(n, 0, fs_in, fs_out, window, True)
    assert (plan.frames_before, plan.frames_after, plan.held) == (pushed, hoa.frames_of(n, fs_in, fs_out), 0)
    want = whole(n)
    for i in range(plan.frames_after):
      a, u = hoa.raw_window(i, fs_in, fs_out, window)
      assert (max(0, a), min(n, u)) == tuple(want[i]) and (i >= pushed or u <= n), (n, i)
  for total in (400, 57):
    for _ in range(3):
      np.testing.assert_array_equal(_walk(_random_cut(total, rng, 12), fs_in, fs_out, window, k, True), whole(total))
  for total in LARGE + [int(rng.integers(5000, 30000))]:
    sizes = _random_cut(total, rng, max(2 * k + 2, 50))
    sizes[1:1] = [k - 1, 0, k, k + 1]
    sizes = [s for s in sizes if s >= 0]
    total = sum(sizes)
    np.testing.assert_array_equal(_walk(sizes, fs_in, fs_out, window, k, False), whole(total))
    assert device.audio_online_plan(0, total, fs_in, fs_out, window).frames_after == hoa.brute_emitted(
        total, fs_in, fs_out, window)
  worst = 0
  for n in range(0, 4 * k + 50):                   # the bound on the carried rows, row by row
    e = device.audio_online_plan(0, n, fs_in, fs_out, window).frames_after
    worst = max(worst, n - max(0, hoa.raw_window(e, fs_in, fs_out, window)[0]))
  assert 0 < worst <= k, (worst, k)


def test_the_second_condition_binds_and_frames_are_held():
  """16000 -> 64 Hz, window 0.5: u_i <= N often holds for a frame F(N) does not count yet -- 762 times in N < 3000."""
  from telluride_decoding_amd import device
  binds = 0
  for n in range(3000):
    plan = device.audio_online_plan(0, n, 16000, 64, 0.5)
    total = hoa.frames_of(n, 16000, 64)
    binds += hoa.raw_window(total, 16000, 64, 0.5)[1] <= n
    assert plan.frames_after <= total
  assert binds == 762
  # window 3: frames wait for their 1.5 frames of future audio, and a flush emits them clamped
  plan = device.audio_online_plan(0, 3000, 16000, 64, 3)
  assert (plan.frames_after, plan.held, plan.tail_rows) == (11, 1, 752)
  assert tuple(device.audio_online_plan(3000, 0, 16000, 64, 3, True))[:3] == (11, 12, 0)


def test_state_bytes_are_the_formula_and_every_refusal_is_named():
  from telluride_decoding_amd import device
  for c in (1, 2, 3, 8):
    for k in (1, 3, 252, 6002, 8192):
      assert device.audio_online_state_bytes(c, k) == 2 * 4 * k * c
  for bad, what in (((0, 5), 'channels'), ((9, 5), 'channels'), ((2, 0), 'carried rows'), ((2, 8193), 'carried rows')):
    with pytest.raises(ValueError, match='td_audio_online_state_bytes.*' + what):
      device.audio_online_state_bytes(*bad)
  # the cap admits 48 kHz -> 64 Hz at window 8
  assert device.audio_online_plan(0, 10, 48000, 64, 8).tail_rows == 6002 <= device.AUDIO_ONLINE_MAX_TAIL
  for args, what in (((0, 5, 0.0, 64, 1), 'rates'), ((0, 5, 16000, -1.0, 1), 'rates'),
                     ((0, 5, float('inf'), 64, 1), 'rates'), ((0, 5, 16000, float('nan'), 1), 'rates'),
                     ((0, 5, 16000, 64, 0.0), 'window'), ((0, 5, 16000, 64, float('inf')), 'window'),
                     ((0, 5, 16000, 64, float('nan')), 'window'), ((0, 5, 100, 100, 1), 'pass-through'),
                     ((0, 5, 64, 100, 1), 'pass-through'), ((0, 5, 64, 100, 0.5), 'pass-through'),
                     ((0, 5, 48000, 64, 11), 'carries 8252 rows'), ((-1, 5, 16000, 64, 1), 'rows behind'),
                     ((0, -5, 16000, 64, 1), 'rows behind')):
    with pytest.raises(ValueError, match='td_audio_online_plan.*' + what):
      device.audio_online_plan(*args)


@pytest.fixture
def host_only(monkeypatch):
  """OnlineAudioFeatures' NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def test_refusals_name_the_parameter(host_only):
  from telluride_decoding_amd import online
  for args in ((100, 100, 1), (64, 100, 1), (64, 100, 0.5)):
    with pytest.raises(ValueError, match='pass-through.*nothing to compute'):
      online.OnlineAudioFeatures(hoa.features(*args))
  with pytest.raises(ValueError, match='preprocess.AudioFeatures, not a dict'):
    online.OnlineAudioFeatures(dict(fs_in=1))
  with pytest.raises(ValueError, match='carries 8252 rows'):
    online.OnlineAudioFeatures(hoa.features(48000, 64, 11))
  assert online.OnlineAudioFeatures(hoa.features(48000, 64, 8)).tail_rows == 6002
  for key, value in (('_fs_in', float('inf')), ('_window', float('nan')), ('_exponent', float('nan'))):
    f = hoa.features(16000, 64, 1)
    setattr(f, key, value)                       # (the constructor's checks let these through)
    with pytest.raises(ValueError, match='finite.* %s' % key[1:]):
      online.OnlineAudioFeatures(f)
  with pytest.raises(ValueError, match='1 to 8 channels, not 9.*nothing is transposed'):
    online.OnlineAudioFeatures(hoa.features(16000, 64, 1)).push(np.zeros((20, 9), np.int16))
  with pytest.raises(ValueError, match='1 to 8 channels, not 3000'):       # (compute_intensity would transpose this)
    online.OnlineAudioFeatures(hoa.features(16000, 64, 1)).push(np.zeros((2, 3000), np.int16))
  for i, key in enumerate(('fs_in', 'fs_out', 'window', 'exponent')):
    args = [16000, 64, 1, 1]
    args[i] = args[i] * 2
    with pytest.raises(ValueError, match='share fs_in, fs_out, window and exponent: %s is' % key):
      online.OnlineAudioFeatures([hoa.features(16000, 64, 1, 1), hoa.features(*args)])
  with pytest.raises(ValueError, match='2 AudioFeatures for num_sessions=3'):
    online.OnlineAudioFeatures([hoa.features(16000, 64, 1)] * 2, num_sessions=3)
  bank = online.OnlineAudioFeatures(hoa.features(16000, 64, 1), num_sessions=2)
  with pytest.raises(ValueError, match=r'audio \[2, n, c\]'):
    bank.push(np.zeros((20, 2), np.int16))
  # the object is read, never written: no buffer appears in the AudioFeatures
  f = hoa.features(16000, 64, 1)
  one = online.OnlineAudioFeatures(f)
  assert one.push(np.zeros((300, 2), np.int16)).shape == (1, 1, 2) and f._buff is None
  with pytest.raises(ValueError, match=r'audio \[1, n, 2\]'):
    one.push(np.zeros((20, 3), np.int16))


# (fs_in, fs_out, window, exponent, channels, dtype)
CASES = [(16000, 64, 1, 1, 2, 'int16'), (6300, 100, 1, 1, 1, 'float32'), (6400, 100, 1, hoa.LOG10_2, 3, 'float64'),
         (6500, 100, 1.5, 0.5, 8, 'int16'), (100, 64, 0.1, 1, 2, 'float32'), (64, 100, 1.5, 2, 1, 'int16'),
         (16000, 64, 3, 1, 2, 'int16'), (1000, 100, 0.5, -1, 4, 'float64'), (3, 2, 1, 0, 2, 'int16'),
         (100, 100, 3, 1, 2, 'int16')]


@pytest.mark.parametrize('case', CASES, ids=['%d_to_%d_w%g_e%.3g_c%d_%s' % c for c in CASES])
def test_numpy_session_is_cut_invariant_and_the_whole_recordings_envelope(host_only, case):
  """Every cut of hoa.cuts (one push, one-row pushes, 1 / 63 / 64 / 65 / K - 1 / K / K + 1 and the rest, seeded
  random sizes with empty pushes) gives the arrays of one push, the state included, and -- the input being integers,
  every sum exact -- exactly HostAudioFeatures(exact=True).compute_intensity(whole): values, NaN positions, count."""
  from telluride_decoding_amd import online
  fs_in, fs_out, window, exponent, c, dtype = case
  x = hoa.recording(c, dtype)
  want, _ = hoa.oracle(x, fs_in, fs_out, window, exponent)
  k = hoa.tail_rows(fs_in, fs_out, window)
  got = {}
  for name, (sizes, _) in sorted(hoa.cuts(hoa.ROWS, k, seed=c).items()):
    obj = online.OnlineAudioFeatures(hoa.features(fs_in, fs_out, window, exponent))
    got[name] = hoa.run_audio(obj, x, sizes) + (obj.state,)
    assert (obj.rows_pushed, obj.frames_emitted, obj.tail_rows) == (hoa.ROWS, want.shape[0], k)
  out32, out64, state = got['whole']
  assert out64.shape == (1,) + want.shape and out64.dtype == np.float64 and out32.dtype == np.float32
  np.testing.assert_array_equal(out64[0], want)                 # (NaN positions included)
  with np.errstate(over='ignore'):
    np.testing.assert_array_equal(out32, out64.astype(np.float32))
  if (fs_in, fs_out) == (100, 64):
    assert np.isnan(want).any() and not np.isnan(want).all()
  sq = np.asarray(x).astype(np.float32)
  np.testing.assert_array_equal(state[0], np.concatenate([np.zeros((k, c), np.float32), sq * sq])[-k:])
  assert state.dtype == np.float32 and state.shape == (1, k, c)
  for name in got:
    for a, b in zip(got[name], got['whole']):
      np.testing.assert_array_equal(a, b, err_msg=name)


def test_numpy_session_on_noise_sits_within_1e_12_of_the_exact_restatement(host_only):
  """Non-integer float32 input: cut invariance by array equality, and the distance to the exactly summed
  restatement within the project's 1e-12 x max."""
  from telluride_decoding_amd import online
  x = hoa.noise(2)
  for fs_in, fs_out, window, exponent in ((16000, 64, 1, 1), (6500, 100, 1.5, hoa.LOG10_2), (100, 64, 0.1, 1)):
    want, _ = hoa.oracle(x, fs_in, fs_out, window, exponent)
    k = hoa.tail_rows(fs_in, fs_out, window)
    cuts = hoa.cuts(hoa.ROWS, k, seed=3)
    runs = [hoa.run_audio(online.OnlineAudioFeatures(hoa.features(fs_in, fs_out, window, exponent)), x, cuts[name][0])
            for name in ('whole', 'edges', 'random')]
    for other in runs[1:]:
      np.testing.assert_array_equal(other[1], runs[0][1])
    got = runs[0][1][0]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    assert np.max(np.abs(got[ok] - want[ok])) <= 1e-12 * np.max(np.abs(want[ok]))


def test_non_finite_input_keeps_its_positions(host_only):
  from telluride_decoding_amd import online
  x = np.array(hoa.noise(2))
  x[700, 0], x[1500, 1], x[2200, 0] = np.inf, np.nan, -np.inf
  want, _ = hoa.oracle(x, 6400, 100, 1.5, 1)
  got = hoa.run_audio(online.OnlineAudioFeatures(hoa.features(6400, 100, 1.5, 1)), x, [699, 2, 1, 1000, 1298])[1][0]
  assert np.isinf(want).sum() >= 2 and np.isnan(want).sum() >= 1
  assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))


def test_a_bank_is_its_sessions(host_only):
  from telluride_decoding_amd import online
  x = hoa.recording(2, 'int16', sessions=3)
  sizes = [37, 0, 250, 1, 2712]
  f = hoa.features(16000, 64, 1.5, 0.5)
  bank = online.OnlineAudioFeatures([f, hoa.features(16000, 64, 1.5, 0.5), f])
  got32, got64 = hoa.run_audio(bank, x, sizes)
  for i in range(3):
    one = online.OnlineAudioFeatures(f)
    want32, want64 = hoa.run_audio(one, x[i], sizes)
    np.testing.assert_array_equal(got64[i], want64[0])
    np.testing.assert_array_equal(got32[i], want32[0])
    np.testing.assert_array_equal(bank.state[i], one.state[0])
  assert not np.array_equal(got64[0], got64[1])
  shared = online.OnlineAudioFeatures(f, num_sessions=3)
  np.testing.assert_array_equal(hoa.run_audio(shared, x, sizes)[1], got64)


def test_flush_reset_and_pushes_around_k(host_only):
  from telluride_decoding_amd import online
  x = hoa.recording(2, 'int16')
  f = hoa.features(16000, 64, 1)
  k = 252
  obj = online.OnlineAudioFeatures(f)
  assert obj.state is None and (obj.rows_pushed, obj.frames_emitted, obj.tail_rows) == (0, 0, k)
  assert obj.push(x[:0]).shape == (1, 0, 2) and not obj.state.any()
  assert obj.push(x[:125]).shape == (1, 0, 2)            # u_0 = 125 is there, but F(125) = round(0.5) = 0
  first = obj.push(x[125:126])
  assert first.shape == (1, 1, 2) and first.dtype == np.float32
  assert obj.flush().shape == (1, 0, 2)
  for call in (lambda: obj.push(x[:5]), obj.flush):
    with pytest.raises(ValueError, match='flushed.*reset'):
      call()
  obj.reset()
  assert (obj.rows_pushed, obj.frames_emitted) == (0, 0) and not obj.state.any()
  fresh = hoa.run_audio(online.OnlineAudioFeatures(f), x, [hoa.ROWS])
  np.testing.assert_array_equal(hoa.run_audio(obj, x, [1500, 1500])[1], fresh[1])
  obj.reset()                                            # a reset in the middle of a recording
  obj.push(x[:777])
  obj.reset()
  np.testing.assert_array_equal(hoa.run_audio(obj, x, [hoa.ROWS])[1], fresh[1])
  for n in (k - 1, k, k + 1):                            # a push of n rows, shorter pushes on both sides of it
    obj.reset()
    np.testing.assert_array_equal(hoa.run_audio(obj, x, [100, n, 3, n, hoa.ROWS - 103 - 2 * n])[1], fresh[1])
  # a 1-D push is one channel; lists and other integer types go through float32 as compute_intensity's astype does
  mono = online.OnlineAudioFeatures(f)
  a = hoa.run_audio(mono, np.asarray(x[:, 0]), [hoa.ROWS])[1]
  np.testing.assert_array_equal(a[0, :, 0], fresh[1][0, :, 0])
  wide = online.OnlineAudioFeatures(f)
  np.testing.assert_array_equal(hoa.run_audio(wide, np.asarray(x, np.int64), [hoa.ROWS])[1], fresh[1])
  # a flush before any row; tensors in, tensors out, and a flush answers as the last push did
  assert online.OnlineAudioFeatures(f).flush().shape == (1, 0, 0)
  import torch
  t = online.OnlineAudioFeatures(f)
  out = t.push(torch.from_numpy(np.array(x[:1000])))
  assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (1, 4, 2)
  last = t.flush(want64=True)
  assert isinstance(last[1], torch.Tensor) and last[1].dtype == torch.float64
  np.testing.assert_array_equal(out.numpy(), fresh[0][:, :4])


def test_frame_join_lines_the_streams_up():
  from telluride_decoding_amd import online
  eeg = np.arange(2 * 20 * 3, dtype=np.float32).reshape(2, 20, 3)
  env = np.arange(2 * 20 * 2, dtype=np.float32).reshape(2, 20, 2) + 1000
  join = online.FrameJoin(3)
  steps = [((0, 4), (0, 0)), ((4, 4), (0, 3)), ((4, 9), (3, 3)), ((9, 15), (3, 11)), ((15, 20), (11, 17))]
  got, at = [[], [], []], 0
  for (e0, e1), (a0, a1) in steps:
    out = join.push(eeg[:, e0:e1], env[:, a0:a1, 0], env[:, a0:a1, 1])
    m = min(e1, a1) - at
    assert [o.shape for o in out] == [(2, m, 3), (2, m), (2, m)], (e1, a1)
    at += m
    for i in range(3):
      got[i].append(out[i])
    assert join.frames_returned == at and join.frames_delivered == [e1, a1, a1]
  np.testing.assert_array_equal(np.concatenate(got[0], axis=1), eeg[:, :17])
  np.testing.assert_array_equal(np.concatenate(got[1], axis=1), env[:, :17, 0])
  np.testing.assert_array_equal(np.concatenate(got[2], axis=1), env[:, :17, 1])
  rest = join.flush(eeg[:, 20:20], env[:, 17:19, 0], env[:, 17:19, 1])
  assert [b.shape for b in rest.blocks] == [(2, 2, 3), (2, 2), (2, 2)] and rest.beyond == [1, 0, 0]
  np.testing.assert_array_equal(rest.blocks[0], eeg[:, 17:19])
  np.testing.assert_array_equal(rest.blocks[2], env[:, 17:19, 1])
  again = join.flush()
  assert [b.shape[1] for b in again.blocks] == [0, 0, 0] and again.beyond == [0, 0, 0]
  # one session's [m, ...] blocks lie along axis 0; torch tensors stay torch tensors
  import torch
  one = online.FrameJoin(2, axis=0)
  a, b = torch.arange(12.0).reshape(6, 2), torch.arange(6.0)
  out = one.push(a[:5], b[:2])
  assert all(isinstance(o, torch.Tensor) for o in out) and [tuple(o.shape) for o in out] == [(2, 2), (2,)]
  out = one.push(a[5:], b[2:])
  assert torch.equal(out[0], a[2:]) and torch.equal(out[1], b[2:])
  end = one.flush()
  assert end.beyond == [0, 0] and all(isinstance(o, torch.Tensor) for o in end.blocks)
  one.reset()
  assert one.frames_returned == 0 and tuple(one.push(a[:1], b[:3])[1].shape) == (1,)
  with pytest.raises(ValueError, match='takes 2 blocks, one per stream, not 3'):
    one.push(a, b, b)
  with pytest.raises(ValueError, match='at least one stream'):
    online.FrameJoin(0)
  with pytest.raises(ValueError, match='flush before any push'):
    online.FrameJoin(2).flush()
  with pytest.raises(ValueError, match='no axis 1'):
    online.FrameJoin(1).push(np.zeros((3,)))
