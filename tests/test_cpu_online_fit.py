"""The online ridge fit without a GPU: the ctypes prototypes of td_fit_online_* against the header, the state size,
every refusal by name, online.OnlineRidgeFit's NumPy session -- its moments against [oracle.lag.lag_matrix | 1] in
float64, cut into pushes every way and flushed both ways with and without forgetting, its solve against
oracle.regression.linear_regressor_from_batches, as a bank, into a BrainModelLinearRegression -- and
OnlineDecoder.set_weights on the host session."""
import ctypes
import re

import numpy as np
import pytest

from oracle import lag as olag
from oracle import regression as oreg
from tests import host_online
from tests import host_online_fit as hof
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_fit_online_moments', 'td_fit_online_push', 'td_fit_online_solve', 'td_fit_online_state_bytes']
SHAPES = [(5, 2, 9, 1), (3, 0, 0, 2), (7, 4, 0, 1), (4, 0, 6, 1), (16, 3, 4, 1)]
FRAMES = 300


@pytest.fixture
def host_only(monkeypatch):
  """OnlineRidgeFit's (and OnlineDecoder's) NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def test_argtypes_match_the_header_prototypes():
  """td_fit_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py); the family stays out of the closed td_online_*,
  td_cca_online_*, td_fc_online_* and td_audio_online_* sets; the header's limits are the module's."""
  from telluride_decoding_amd import _lib, device, online
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_fit_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert not re.fullmatch(r'td_(online|cca_online|fc_online|audio_online)_\w+', name)
    assert name in _lib.header_symbols()
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
  for macro, value in (('TD_ONLINE_FIT_MAX_CHANNELS', device.ONLINE_FIT_MAX_CHANNELS),
                       ('TD_ONLINE_FIT_MAX_LAGS', device.ONLINE_FIT_MAX_LAGS),
                       ('TD_ONLINE_FIT_MAX_K', device.ONLINE_FIT_MAX_K),
                       ('TD_ONLINE_FIT_MAX_OUTPUTS', device.ONLINE_FIT_MAX_OUTPUTS),
                       ('TD_ONLINE_MAX_PUSH', online.MAX_FIT_PUSH)):
    found = re.search(r'#define\s+%s\s+(\d+)' % macro, raw)
    assert found and int(found.group(1)) == value, macro
  assert (device.ONLINE_FIT_MAX_CHANNELS, device.ONLINE_FIT_MAX_LAGS, device.ONLINE_FIT_MAX_K,
          device.ONLINE_FIT_MAX_OUTPUTS, online.MAX_FIT_PUSH) == (128, 64, 2048, 8, 1048576)


def test_state_bytes_hold_what_a_session_carries():
  """A full square of float64, B, and TWO copies of the float32 tails; a multiple of 8; the limits by name."""
  from telluride_decoding_amd import device
  for c, pre, post, d in SHAPES + [(63, 1, 0, 1), (16, 3, 0, 8), (64, 0, 20, 1), (128, 0, 15, 1), (1, 0, 0, 1),
                                   (1, 31, 32, 3), (32, 63, 0, 8)]:
    n1 = (pre + 1 + post) * c + 1
    need = 8 * (n1 * n1 + n1 * d) + 2 * 4 * ((pre + post) * c + post * d)
    nbytes = device.online_fit_state_bytes(c, pre, post, d)
    assert nbytes % 8 == 0 and need <= nbytes < need + 8, (c, pre, post, d, nbytes)
  for bad in ((0, 0, 0, 1), (129, 0, 0, 1), (4, -1, 0, 1), (4, 0, -1, 1), (4, 32, 32, 1), (128, 0, 16, 1),
              (33, 0, 62, 1), (4, 0, 0, 0), (4, 0, 0, 9)):
    with pytest.raises(ValueError, match='td_fit_online_state_bytes'):
      device.online_fit_state_bytes(*bad)


def test_every_refusal_is_raised_by_name(host_only):
  from telluride_decoding_amd import online
  for kwargs, match in ((dict(channels=129), '128 channels'), (dict(channels=0), '128 channels'),
                        (dict(pre_context=32, post_context=32), '64 lags'), (dict(pre_context=-1), '64 lags'),
                        (dict(post_context=-1), '64 lags'),
                        (dict(channels=128, post_context=16), '2048 lagged inputs'),
                        (dict(outputs=0), '8 outputs'), (dict(outputs=9), '8 outputs'),
                        (dict(forgetting=0.0), 'forgetting'), (dict(forgetting=1.5), 'forgetting'),
                        (dict(forgetting=float('nan')), 'forgetting'), (dict(num_sessions=0), 'at least one session')):
    args = dict(channels=4, pre_context=1, post_context=2)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
      online.OnlineRidgeFit(**args)
  online.OnlineRidgeFit(128, 0, 15)                                    # K = 2048: the limit itself
  fit = online.OnlineRidgeFit(4, 1, 2, outputs=2, num_sessions=2)
  assert (fit.delay, fit.frames, fit.inputs, fit.lags) == (2, 0, 16, 4)
  z = lambda *shape: np.zeros(shape, np.float32)
  for eeg, target in ((z(10, 4), z(10, 2)),                            # two sessions need [S, n, c]
                      (z(2, 10, 5), z(2, 10, 2)), (z(2, 10, 4), z(2, 10, 3)), (z(2, 10, 4), z(2, 9, 2)),
                      (z(3, 10, 4), z(3, 10, 2)), (z(2, 10, 4), z(2, 10))):
    with pytest.raises(ValueError, match='A push is'):
      fit.push(eeg, target)
  with pytest.raises(ValueError, match='no frame counted yet'):
    fit.solve([0.1])
  assert fit.push(z(2, 2, 4), z(2, 2, 2)) == 0                         # two rows, two behind: still nothing counted
  with pytest.raises(ValueError, match='no frame counted yet'):
    fit.solve([0.1])
  with pytest.raises(ValueError, match='at least one lambda'):
    fit.solve([])
  assert fit.push(z(2, 1, 4), z(2, 1, 2)) == 1
  with pytest.raises(np.linalg.LinAlgError):                           # all-zero EEG, lambda 0: singular
    fit.solve([0.0])
  with pytest.raises(ValueError, match='eeg AND target'):
    fit.flush(z(2, 1, 4))
  assert fit.flush() == 3
  for call in (lambda: fit.push(z(2, 1, 4), z(2, 1, 2)), fit.flush):
    with pytest.raises(ValueError, match='flushed'):
      call()
  one = online.OnlineRidgeFit(1, 0, 0)
  with pytest.raises(ValueError, match='1048576 rows'):
    one.push(z(1048577, 1), z(1048577))
  assert one.push(z(5, 1), z(5)) == 5 and one.push(z(5, 1), z(5, 1)) == 10      # [n] and [n, 1] targets


def _session_moments(fit):
  a, b = fit.moments()
  return np.array(a[0]), np.array(b[0])


@pytest.mark.parametrize('c,pre,post,d', SHAPES)
def test_the_moments_are_those_of_the_lag_matrix(host_only, c, pre, post, d):
  """A = X^T X and B = X^T y of X = [oracle.lag.lag_matrix(x, pre, post) | 1] in float64, within 1e-12 of the
  largest element (a frame-by-frame sum against a matrix product: measured <= 1.2e-16); A[K][K] the frame count,
  A symmetric to the bit."""
  from telluride_decoding_amd import online
  eeg, target = hof.recording(c, d, FRAMES)
  want_a, want_b = hof.reference_moments(c, pre, post, d, FRAMES)
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d)
  hof.run(fit, eeg, target, [100, 0, 37, 163])
  a, b = _session_moments(fit)
  k = fit.inputs
  assert a.shape == (k + 1, k + 1) and b.shape == (k + 1, d) and a.dtype == b.dtype == np.float64
  print('moments vs the lag matrix: A %.3g, B %.3g of the largest element' % (hof.rel(a, want_a), hof.rel(b, want_b)))
  assert hof.rel(a, want_a) <= 1e-12 and hof.rel(b, want_b) <= 1e-12
  assert a[k, k] == FRAMES
  np.testing.assert_array_equal(a, a.T)
  # before the flush the last `post` frames are missing: the moments of the recording's first FRAMES - post rows
  # of the lag matrix (which still see the rows behind them)
  fit.reset()
  assert fit.push(eeg, target) == FRAMES - post
  x = hof.lagged_ones(eeg, pre, post)[:FRAMES - post]
  assert hof.rel(_session_moments(fit)[0], x.T @ x) <= 1e-12
  tails = fit.tails
  np.testing.assert_array_equal(tails[0][0], eeg[FRAMES - (pre + post):])
  np.testing.assert_array_equal(tails[1][0], target[FRAMES - post:])


@pytest.mark.parametrize('forget', hof.FORGETS)
@pytest.mark.parametrize('c,pre,post,d', SHAPES)
def test_numpy_session_is_chunk_invariant(host_only, c, pre, post, d, forget):
  """Pushes of 1, 7, random 0 .. 40 and whole (and pre + post - 1, and an empty push in the middle), flushed by a
  flushing last push and by an empty flushing push, g = 1 and 0.99: the same bytes."""
  from telluride_decoding_amd import online
  eeg, target = hof.recording(c, d, FRAMES)
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d, forgetting=forget)
  hof.run(fit, eeg, target, [FRAMES])
  whole = _session_moments(fit)
  if forget == 1.0:
    assert whole[0][-1, -1] == FRAMES
  else:
    # the effective count: sum of g^m in the order the frames arrive
    count = 0.0
    for _ in range(FRAMES):
      count = count * forget + 1.0
    assert whole[0][-1, -1] == count
  for name, sizes in hof.cuts(FRAMES, pre, post).items():
    for flush_last in (False, True):
      hof.run(fit, eeg, target, sizes, flush_last=flush_last)
      got = _session_moments(fit)
      np.testing.assert_array_equal(got[0], whole[0], err_msg='%s %s' % (name, flush_last))
      np.testing.assert_array_equal(got[1], whole[1], err_msg='%s %s' % (name, flush_last))


@pytest.mark.parametrize('c,pre,post,d', SHAPES)
def test_solve_is_the_references_regression(host_only, c, pre, post, d):
  """oracle.regression.linear_regressor_from_batches on the lagged whole recording as ONE minibatch (float64), for
  lambda 1e-3, 0.1 and 10: W and b within 1e-9 of the largest weight."""
  from telluride_decoding_amd import online
  eeg, target = hof.recording(c, d, FRAMES)
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d)
  hof.run(fit, eeg, target, [7] * 42 + [6])
  w, b = fit.solve(hof.LAMBDAS)
  assert w.shape == (1, 3, fit.inputs, d) and b.shape == (1, 3, d)
  x = olag.lag_matrix(eeg.astype(np.float64), pre, post)
  for li, lam in enumerate(hof.LAMBDAS):
    want_w, want_b, _, _, _ = oreg.linear_regressor_from_batches([({'input_1': x}, target.astype(np.float64))],
                                                                 lamb=lam)
    err_w, err_b = hof.rel(w[0, li], want_w), hof.rel(b[0, li], np.reshape(want_b, -1))
    print('lambda %g: W %.3g, b %.3g' % (lam, err_w, err_b))
    assert err_w <= 1e-9
    assert np.max(np.abs(b[0, li] - np.reshape(want_b, -1))) <= 1e-9 * np.max(np.abs(want_w))


def test_a_bank_is_its_sessions(host_only):
  from telluride_decoding_amd import online
  c, pre, post, d = 5, 2, 9, 1
  recs = [hof.recording(c, d, FRAMES, seed=s) for s in range(3)]
  eeg, target = np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs])
  bank = online.OnlineRidgeFit(c, pre, post, outputs=d, num_sessions=3, forgetting=0.99)
  hof.run(bank, eeg, target, [130, 1, 0, 169])
  a, b = bank.moments()
  w, bias = bank.solve([0.1])
  assert a.shape == (3, 61, 61) and b.shape == (3, 61, 1) and w.shape == (3, 1, 60, 1) and bias.shape == (3, 1, 1)
  for i in range(3):
    single = online.OnlineRidgeFit(c, pre, post, outputs=d, forgetting=0.99)
    hof.run(single, recs[i][0], recs[i][1][:, 0], [FRAMES])            # (a [n] target)
    np.testing.assert_array_equal(a[i], single.moments()[0][0])
    np.testing.assert_array_equal(b[i], single.moments()[1][0])
    np.testing.assert_array_equal(w[i], single.solve([0.1])[0][0])
  assert not np.array_equal(a[0], a[1])
  bank.reset()
  assert bank.frames == 0 and not bank.moments()[0].any() and not bank.tails[0].any()


def test_update_model_checks_the_model_and_sets_its_weights(host_only):
  from telluride_decoding_amd import brain_model, online
  c, pre, post, d = 5, 2, 9, 1
  eeg, target = hof.recording(c, d, FRAMES)
  fit = online.OnlineRidgeFit(c, pre, post, outputs=d)
  hof.run(fit, eeg, target, [FRAMES])
  model = brain_model.BrainModelLinearRegression(brain_model._shape_dataset(c, 1, d, pre, post))
  assert fit.update_model(model, 0.1) is model
  w, b = fit.solve([0.1])
  np.testing.assert_array_equal(model.w_estimate, w[0, 0].astype(np.float32))
  np.testing.assert_array_equal(model.b_estimate, b[0, 0].astype(np.float32))
  assert model.w_estimate.shape == (60, 1) and model.w_estimate.dtype == np.float32
  for args, match in (((4, 1, d, pre, post), 'channels'), ((c, 1, d, 1, post), 'pre_context'),
                      ((c, 1, d, pre, 8), 'post_context'), ((c, 1, 2, pre, post), 'outputs')):
    other = brain_model.BrainModelLinearRegression(brain_model._shape_dataset(*args))
    with pytest.raises(ValueError, match=match):
      fit.update_model(other, 0.1)
    assert other.w_estimate is None
  with pytest.raises(ValueError, match='session 1 of 1'):
    fit.update_model(model, 0.1, session=1)
  with pytest.raises(ValueError, match='BrainModelLinearRegression'):
    fit.update_model(object(), 0.1)


def _frames(dec, rec, lo, hi):
  r = dec.push(rec['eeg'][lo:hi], rec['env'][lo:hi, 0], rec['env'][lo:hi, 1])
  return r.scores[0]


def test_set_weights_swaps_the_model_between_pushes(host_only):
  """Windows of one frame are the per-frame scores: weights swapped in after k emitted frames give, from frame k
  on, the scores of a decoder built with those weights, and before it those of the old one; the bank forms, the
  refusals."""
  from telluride_decoding_amd import infer_decoder, online
  c, pre, post = 4, 2, 3
  rec = host_online.recipe(c, pre, post)
  rng = np.random.default_rng(5)
  w1, b1 = rec['w'], rec['b']
  w2 = (0.5 * np.asarray(w1) + 0.1 * rng.standard_normal(np.shape(w1))).astype(np.float32)
  b2 = np.float32(0.25)
  make = lambda w, b: host_online.linear_decoder(c, pre, post, w, b, rec['corr'][0], 'mean-squared')
  old, new = online.OnlineDecoder(make(w1, b1), 1, 1), online.OnlineDecoder(make(w2, b2), 1, 1)
  dec = online.OnlineDecoder(make(w1, b1), 1, 1)
  cut, end = 130, 400
  k = cut - post                                                       # frames emitted before the swap
  head = _frames(dec, rec, 0, cut)
  dec.set_weights(np.reshape(w2, -1), b2)
  rest = np.concatenate([_frames(dec, rec, cut, end), dec.flush().scores[0]])
  want_old = _frames(old, rec, 0, cut)
  want_new = np.concatenate([_frames(new, rec, 0, cut), _frames(new, rec, cut, end), new.flush().scores[0]])
  assert head.shape == (k, 2) and rest.shape == (end - k, 2)
  np.testing.assert_array_equal(head, want_old)
  np.testing.assert_array_equal(rest, want_new[k:])
  assert not np.array_equal(rest, np.concatenate([_frames(old, rec, cut, end), old.flush().scores[0]]))
  # a bank: [S, K] rows with [S] biases, or one row for every session
  bank = online.OnlineDecoder([make(w1, b1)] * 2, 1, 1)
  bank.set_weights(np.stack([np.reshape(w1, -1), np.reshape(w2, -1)]), np.array([np.reshape(b1, -1)[0], b2]))
  eeg2 = np.stack([rec['eeg'][:cut]] * 2)
  env = [np.stack([rec['env'][:cut, s]] * 2) for s in (0, 1)]
  got = bank.push(eeg2, env[0], env[1]).scores
  np.testing.assert_array_equal(got[0], want_old)
  np.testing.assert_array_equal(got[1], want_new[:k])
  bank.reset()
  bank.set_weights(np.reshape(w2, -1), b2)
  got = bank.push(eeg2, env[0], env[1]).scores
  np.testing.assert_array_equal(got[0], want_new[:k])
  np.testing.assert_array_equal(got[1], want_new[:k])
  for w, b in ((np.zeros(23, np.float32), 0.0), (np.zeros((3, 24), np.float32), np.zeros(3)),
               (np.zeros((2, 24), np.float32), 0.0), (np.zeros(24, np.float32), np.zeros(2))):
    with pytest.raises(ValueError, match='set_weights takes'):
      bank.set_weights(w, b)
  cca = online.OnlineDecoder.__new__(online.OnlineDecoder)
  cca.kind = 'cca'
  with pytest.raises(ValueError, match='linear bank only'):
    cca.set_weights(np.zeros(24, np.float32), 0.0)
  assert 'out of scope' in online.OnlineDecoder.set_weights.__doc__
  del infer_decoder
