"""The online front end without a GPU: the ctypes prototypes of td_frontend_* against the header, td_frontend_plan
against preprocess.resample_indices over rates, lengths and cuts, the state and LDS sizes against their formulas,
every refusal by name, and online.OnlinePreprocessor's NumPy session -- cut into pushes every way, against
tests/host_preprocess.HostPreprocessor on the whole recording, as a bank, flushed and reset."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online_pre as ho
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_frontend_lds_bytes', 'td_frontend_plan', 'td_frontend_push', 'td_frontend_state_bytes']
RATES = [(1000, 100), (1000, 64), (512, 64), (100, 100), (64, 100), (100, 1000), (44100, 100), (3, 2), (2, 3),
         (1000, 999)]
LENGTHS = list(range(1, 60)) + [997, 1000, 1003]


def test_argtypes_match_the_header_prototypes():
  """td_frontend_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py); the family stays out of the closed td_online_*,
  td_cca_online_* and td_fc_online_* sets; the header's limits are the module's."""
  from telluride_decoding_amd import _lib, device
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_frontend_\w+)\s*\(([^)]*)\)\s*;', text))
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
  for macro, value in (('TD_FRONTEND_LDS_BYTES', device.FRONTEND_LDS_BYTES),
                       ('TD_FRONTEND_MAX_GROUPS', device.FRONTEND_MAX_GROUPS)):
    found = re.search(r'#define\s+%s\s+(\d+)' % macro, raw)
    assert found and int(found.group(1)) == value, macro
  assert (device.FRONTEND_LDS_BYTES, device.FRONTEND_MAX_CHANNELS, device.FRONTEND_MAX_SECTIONS) == (49152, 128, 16)


def _random_cut(total, rng):
  sizes = []
  while sum(sizes) < total:
    sizes.append(int(min(rng.integers(0, 12), total - sum(sizes))))
  return sizes


@pytest.mark.parametrize('fs_in,fs_out', RATES)
def test_plan_emits_the_rows_of_resample_indices_over_any_cut(fs_in, fs_out):
  """N in 1..59 and 997, 1000, 1003; pushes of one row and a seeded random cut with empty pushes, then a flush: the
  rows of the emitted frames, concatenated, are resample_indices(N); every plan is the brute-force count and
  online.host_frontend_plan's; held <= 1, and 0 when not downsampling."""
  from telluride_decoding_amd import device, online, preprocess
  rng = np.random.default_rng(fs_in + fs_out)
  held_seen = 0
  for total in LENGTHS:
    want, _ = preprocess.resample_indices(total, fs_in, fs_out)
    for sizes in ([1] * total, _random_cut(total, rng)):
      rows, at, frames = [], 0, 0
      for k, n in enumerate(sizes + [0]):
        flush = k == len(sizes)
        plan = device.frontend_plan(at, n, fs_in, fs_out, flush)
        assert plan.frames_before == frames == ho.brute_frames(at, fs_in, fs_out, False), (total, at)
        assert plan.frames_after == ho.brute_frames(at + n, fs_in, fs_out, flush), (total, at, n, flush)
        assert tuple(plan) == online.host_frontend_plan(at, n, fs_in, fs_out, flush)[:3]
        assert 0 <= plan.held <= 1 and (plan.held == 0 or fs_out < fs_in), (total, at, n, plan)
        held_seen = max(held_seen, plan.held)
        r = online.frame_rows(plan.frames_before, plan.frames_after - plan.frames_before, fs_in, fs_out)
        if not flush:
          assert r.size == 0 or r.max() <= at + n - 1
        rows += list(np.minimum(at + n - 1, r))
        at, frames = at + n, plan.frames_after
      assert rows == list(want), (total, sizes)
  if (fs_in, fs_out) in ((1000, 100), (1000, 64), (44100, 100)):
    assert held_seen == 1
  with pytest.raises(ValueError, match='td_frontend_plan.*rates'):
    device.frontend_plan(0, 5, 0.0, fs_out)
  with pytest.raises(ValueError, match='td_frontend_plan'):
    device.frontend_plan(-1, 5, fs_in, fs_out)


def test_the_hold_back_and_the_clamp():
  from telluride_decoding_amd import device
  # 14 rows at 1000 -> 100: frame 1 reads row 10, which is there, but resample_indices(14) has 1 frame: held back
  assert tuple(device.frontend_plan(0, 14, 1000, 100)) == (0, 1, 1)
  assert tuple(device.frontend_plan(14, 0, 1000, 100, True)) == (1, 1, 1)        # (and a flush drops it)
  assert tuple(device.frontend_plan(14, 2, 1000, 100)) == (1, 2, 0)              # (16 rows: emitted)
  # 1 row at 64 -> 100: resample_indices(1) has 2 frames, both from row 0; frame 1 reads row rint(0.64) = 1
  assert tuple(device.frontend_plan(0, 1, 64, 100)) == (0, 1, 0)
  assert tuple(device.frontend_plan(1, 0, 64, 100, True)) == (1, 2, 0)
  assert tuple(device.frontend_plan(0, 1, 64, 100, True)) == (0, 2, 0)
  assert tuple(device.frontend_plan(7, 5, 250, 250)) == (7, 12, 0)


def test_state_and_lds_bytes_are_their_formulas_and_the_limits_are_named():
  from telluride_decoding_amd import device
  for c in (1, 5, 64, 128):
    for sections in (0, 1, 7, 16):
      assert device.frontend_state_bytes(c, sections) == 8 * (2 * sections + 2) * c
  for c, groups in ((1, 0), (5, 2), (64, 1), (65, 0), (128, 0), (128, 32)):
    for emitted in (0, 1, 10, 64, 65, 3000):
      pass_, lds = device.frontend_lds_bytes(c, groups, emitted)
      want = min(64, max(emitted, 1))
      while want > 1 and 8 * want * (c + groups) > device.FRONTEND_LDS_BYTES:
        want = (want + 1) // 2
      assert (pass_, lds) == (want, 8 * want * (c + groups)), (c, groups, emitted)
      assert lds <= device.FRONTEND_LDS_BYTES
  assert device.frontend_lds_bytes(64, 1, 100) == (64, 33280)       # the timed configuration: whole passes of 64
  assert device.frontend_lds_bytes(128, 32, 100)[0] == 32
  for bad, what in (((0, 1), 'channels'), ((129, 1), 'channels'), ((4, -1), 'sections'), ((4, 17), 'sections')):
    with pytest.raises(ValueError, match='td_frontend_state_bytes.*' + what):
      device.frontend_state_bytes(*bad)
  for bad, what in (((0, 0, 1), 'channels'), ((129, 0, 1), 'channels'), ((4, -1, 1), 'groups'), ((4, 33, 1), 'groups'),
                    ((4, 0, -1), 'frames')):
    with pytest.raises(ValueError, match='td_frontend_lds_bytes.*' + what):
      device.frontend_lds_bytes(*bad)


@pytest.fixture
def host_only(monkeypatch):
  """OnlinePreprocessor's NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def test_refusals_name_the_parameter(host_only):
  from telluride_decoding_amd import online
  good = dict(fs_in=1000, fs_out=100, data_mean=0.0, data_std=1.0)
  x = np.zeros((20, 4), np.float32)
  for key in ('pre_context', 'post_context'):
    with pytest.raises(ValueError, match=key + '=2.*decoder adds its own'):
      online.OnlinePreprocessor(ho.make(dict(good, **{key: 2})))
  with pytest.raises(ValueError, match='data_mean.*depends on the cut'):
    online.OnlinePreprocessor(ho.make(dict(good, data_mean=None)))
  for std in (None, 0.0):
    prep = ho.make(good)
    prep._data_std = std                     # (the constructor refuses these itself; an object can still hold them)
    with pytest.raises(ValueError, match='data_std'):
      online.OnlinePreprocessor(prep)
  with pytest.raises(ValueError, match='at most 16 second-order sections, not 17'):
    online.OnlinePreprocessor(ho.make(dict(good, fs_out=1000, highpass_cutoff=1, highpass_order=17, lowpass_cutoff=40,
                                           lowpass_order=16)))
  with pytest.raises(ValueError, match='preprocess.Preprocessor, not a dict'):
    online.OnlinePreprocessor(good)
  with pytest.raises(ValueError, match='1 to 128 channels, not 129'):
    online.OnlinePreprocessor(ho.make(good)).push(np.zeros((5, 129), np.float32))
  with pytest.raises(ValueError, match='A push is raw'):
    online.OnlinePreprocessor(ho.make(good)).push(np.zeros((5,), np.float32))
  for key, value in (('channel_numbers', [0, 4]), ('ref_channels', [[0, 7]]), ('channels_to_ref', [[1, -1]])):
    with pytest.raises(ValueError, match=key + '.*outside a row of 4 channels'):
      online.OnlinePreprocessor(ho.make(dict(good, **{key: value}))).push(x)
  # a bank shares everything except data_mean / data_std; a mismatch names the parameter
  for key, value in (('fs_out', 64), ('highpass_cutoff', 1.0), ('channel_numbers', [0, 1]), ('ref_channels', [[0]])):
    with pytest.raises(ValueError, match='share everything except data_mean and data_std: %s is' % key):
      online.OnlinePreprocessor([ho.make(good), ho.make(dict(good, **{key: value}))])
  with pytest.raises(ValueError, match='2 preprocessors for num_sessions=3'):
    online.OnlinePreprocessor([ho.make(good)] * 2, num_sessions=3)
  bank = online.OnlinePreprocessor([ho.make(good), ho.make(dict(good, data_mean=1.0, data_std=2.0))])
  assert bank.sessions == 2 and online.OnlinePreprocessor(ho.make(good), num_sessions=4).sessions == 4
  with pytest.raises(ValueError, match=r'raw \[2, n, C\]'):
    bank.push(x)
  # the object is read, never written: a global re-reference leaves ref_channels as the caller gave it
  prep = ho.make(dict(good, channels_to_ref=[[0, 1]]))
  front = online.OnlinePreprocessor(prep)
  assert front.push(x).shape == (1, 2, 4) and prep.ref_channels is None and prep.filter_state is None


CASES = [(7, 1000, 100, 5), (7, 1000, 64, 64), (0, 64, 100, 3), (16, 250, 250, 4), (1, 250, 250, 1), (2, 64, 100, 2)]


@pytest.mark.parametrize('sections,fs_in,fs_out,c', CASES)
def test_numpy_session_is_cut_invariant_and_the_oracle(host_only, sections, fs_in, fs_out, c):
  """Every cut of ho.cuts (one push, one-row pushes for the small cases, the edge sizes, seeded random sizes with
  empty pushes) gives the arrays of one push, state included; the float64 output and the filter state sit within
  1e-12 max|x| of HostPreprocessor on the whole recording (both are float64 NumPy with the multiply-adds rounded
  twice, in different orders; measured here: <= 5e-13.  The 0.01 Hz + 1 Hz order-16 cascade of
  s16_hard_0p01_1hz sits at 4e-12 and is held to the GPU tests' 1e-9 there); the float32 output is its cast."""
  from telluride_decoding_amd import online
  kw = ho.config(sections, fs_in, fs_out, c)
  assert ho.sections_of(kw) == sections
  x = ho.recording(c, fs_in, np.float64)
  want, want_state = ho.oracle(kw, x)
  scale = float(np.max(np.abs(x)))
  cuts = ho.cuts(ho.ROWS, seed=c)
  names = ['whole', 'edges', 'random'] + (['ones'] if sections <= 2 else [])
  got = {}
  for name in names:
    front = online.OnlinePreprocessor(ho.make(kw))
    got[name] = ho.run_front(front, x, cuts[name][0]) + (front.state,)
    assert (front.rows_pushed, front.frames_emitted) == (ho.ROWS, want.shape[0])
  out32, out64, state = got['whole']
  assert out64.shape == (1,) + want.shape and out32.dtype == np.float32
  np.testing.assert_array_equal(out32, out64.astype(np.float32))
  assert np.max(np.abs(out64[0] - want)) <= 1e-12 * scale
  assert state.shape == (1, 2 * sections + 2, c)
  if sections:
    assert np.max(np.abs(state[0, :-2].reshape(want_state.shape) - want_state)) <= 1e-12 * scale
  for name in names[1:]:
    for a, b in zip(got[name], got['whole']):
      np.testing.assert_array_equal(a, b, err_msg=name)


def test_a_bank_is_its_sessions_with_their_own_mean_and_std(host_only):
  from telluride_decoding_amd import online
  base = ho.config(7, 1000, 100, 5)
  stats = [(0.25, 1.5), (-1.0, 0.5), (0.0, 2.0)]
  preps = [ho.make(dict(base, data_mean=m, data_std=s)) for m, s in stats]
  x = np.stack([ho.recording(5, 1000) * np.float32(g) for g in (1.0, 2.0, -0.5)])
  sizes = [37, 0, 250, 1, 2712]
  bank = online.OnlinePreprocessor(preps)
  got32, got64 = ho.run_front(bank, x, sizes)
  for i, prep in enumerate(preps):
    one = online.OnlinePreprocessor(prep)
    want32, want64 = ho.run_front(one, x[i], sizes)
    np.testing.assert_array_equal(got64[i], want64[0])
    np.testing.assert_array_equal(got32[i], want32[0])
    np.testing.assert_array_equal(bank.state[i], one.state[0])
  # per-session statistics: session 1 is session 0's frames of twice the signal on its own mean / std
  raw = got64[0] * 1.5 + 0.25
  np.testing.assert_allclose(got64[1], (2.0 * raw + 1.0) / 0.5, rtol=0, atol=1e-9)
  shared = online.OnlinePreprocessor(preps[0], num_sessions=3)
  copies = online.OnlinePreprocessor([preps[0]] * 3)
  np.testing.assert_array_equal(ho.run_front(shared, x, sizes)[1], ho.run_front(copies, x, sizes)[1])


def test_flush_and_reset(host_only):
  from telluride_decoding_amd import online
  kw = ho.config(7, 1000, 100, 5)
  x = ho.recording(5, 1000)
  front = online.OnlinePreprocessor(ho.make(kw))
  assert front.state is None and (front.rows_pushed, front.frames_emitted) == (0, 0)
  assert front.push(x[:0]).shape == (1, 0, 2)
  first = front.push(x[:14])
  assert first.shape == (1, 1, 2) and first.dtype == np.float32          # (14 rows: 1 frame, frame 1 is held)
  assert front.push(x[14:16]).shape == (1, 1, 2)                         # (... and emitted with row 16)
  assert front.flush().shape == (1, 0, 2)
  for call in (lambda: front.push(x[:5]), front.flush):
    with pytest.raises(ValueError, match='flushed.*reset'):
      call()
  front.reset()
  assert (front.rows_pushed, front.frames_emitted) == (0, 0) and not front.state.any()
  again = ho.run_front(front, x, [1500, 1500])
  fresh = ho.run_front(online.OnlinePreprocessor(ho.make(kw)), x, [1500, 1500])
  np.testing.assert_array_equal(again[1], fresh[1])
  # a reset in the middle of a recording: what follows is a fresh recording
  front.reset()
  front.push(x[:777])
  front.reset()
  np.testing.assert_array_equal(ho.run_front(front, x, [3000])[1], fresh[1])
  # the hold-back dropped by a flush, and the clamp: N = 14 at 1000 -> 100 is 1 frame, N = 1 at 64 -> 100 is 2 frames
  # of row 0
  front.reset()
  assert front.push(x[:14]).shape[1] + front.flush().shape[1] == 1
  up = online.OnlinePreprocessor(ho.make(dict(fs_in=64, fs_out=100, data_mean=0.0, data_std=1.0)))
  a, b = up.push(x[:1]), up.flush()
  assert a.shape == b.shape == (1, 1, 5)
  np.testing.assert_array_equal(a, x[None, :1])
  np.testing.assert_array_equal(b, x[None, :1])
  # tensors in, tensors out; a flush answers as the last push did
  import torch
  t = online.OnlinePreprocessor(ho.make(kw))
  out = t.push(torch.from_numpy(np.array(x[:100])))
  assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (1, 10, 2)
  assert isinstance(t.flush(), torch.Tensor)
  np.testing.assert_array_equal(out.numpy(), fresh[0][:, :10])
