"""The online decoder without a GPU: td_online_plan / td_online_state_bytes through ctypes (the library
loads without a device) against a brute-force count, the ctypes prototypes against the header, and
online.OnlineDecoder's NumPy session -- against the oracle chain, and cut into pushes every way."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online
from tests.test_cpu_dnn import _kind_of_ctype

ONLINE_ENTRY_POINTS = ['td_online_plan', 'td_online_push', 'td_online_state_bytes']


def test_plan_is_the_brute_force_count():
  from telluride_decoding_amd import device
  checked = 0
  for post in (0, 5):
    for width, hop in ((1, 1), (10, 5), (37, 11), (5, 9)):
      for flush in (0, 1):
        for n in (0, 1, 7, 100):
          for before in range(0, 301):
            want = host_online.brute_plan(before, n, post, width, hop, flush)
            got = device.online_plan(before, n, post, width, hop, bool(flush))
            assert tuple(got) == want, (before, n, post, width, hop, flush)
            checked += 1
  assert checked == 2 * 4 * 2 * 4 * 301


def test_plan_refuses_what_it_cannot_count():
  from telluride_decoding_amd import device
  for args in ((-1, 1, 0, 1, 1), (0, -1, 0, 1, 1), (0, 1, -1, 1, 1), (0, 1, 0, 0, 1), (0, 1, 0, 1, 0)):
    with pytest.raises(ValueError, match='td_online_plan'):
      device.online_plan(*args)


def test_state_bytes_hold_what_a_session_carries():
  from telluride_decoding_amd import device
  for c, pre, post, width in ((5, 2, 9, 100), (64, 0, 31, 10), (63, 40, 5, 37), (128, 3, 12, 1), (1, 0, 0, 1),
                              (128, 31, 32, 65536), (3, 0, 63, 4096)):
    nbytes = device.online_state_bytes(c, pre, post, width)
    # the tails, the ring of both speakers' scores, the stepped decoder's state
    need = 4 * c * (pre + post) + 4 * 2 * post + 8 * 2 * width + 8
    assert nbytes % 8 == 0 and need <= nbytes < need + 8, (c, pre, post, width, nbytes)
  for bad in ((0, 0, 0, 1), (129, 0, 0, 1), (4, -1, 0, 1), (4, 0, -1, 1), (4, 32, 32, 1), (4, 0, 0, 0),
              (4, 0, 0, 65537)):
    with pytest.raises(ValueError, match='td_online_state_bytes'):
      device.online_state_bytes(*bad)


def test_argtypes_match_the_header_prototypes():
  """td_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_dnn_many.py).  The names stay out of the patterns other
  tests pin (td_mlp_*, td_mlpc_*, td_dnn_*), and the header's limits are the module's."""
  from telluride_decoding_amd import _lib, online
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ONLINE_ENTRY_POINTS
  for name in ONLINE_ENTRY_POINTS:
    assert not re.fullmatch(r'td_(mlpc?|dnn)_\w+', name)
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
  cap = re.search(r'#define\s+TD_ONLINE_MAX_WIDTH\s+(\d+)', raw)
  assert cap and int(cap.group(1)) == online.MAX_WINDOW
  lib = _lib.load()
  for name in ONLINE_ENTRY_POINTS:
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


@pytest.fixture
def host_only(monkeypatch):
  """OnlineDecoder's NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


LDA = (1.7, -0.8, 0.25)


def _run(decoder, rec, sizes, width, hop, kind):
  from telluride_decoding_amd import online
  dec = online.OnlineDecoder(decoder, width, hop, decoder_type=kind)
  scores, decisions, firsts, at = [], [], [], 0
  for i, n in enumerate(sizes):
    r = dec.push(rec['eeg'][at:at + n], rec['env'][at:at + n, 0], rec['env'][at:at + n, 1])
    at += n
    scores.append(r.scores[0]); decisions.append(r.decisions[0]); firsts.append(r.first_window)
  r = dec.flush()
  scores.append(r.scores[0]); decisions.append(r.decisions[0]); firsts.append(r.first_window)
  assert firsts == list(np.cumsum([0] + [len(s) for s in scores[:-1]]))
  with pytest.raises(ValueError, match='flushed'):
    dec.push(rec['eeg'][:1], rec['env'][:1, 0], rec['env'][:1, 1])
  return np.concatenate(scores), np.concatenate(decisions)


@pytest.mark.parametrize('reduction', ['first', 'mean', 'mean-squared', 'lda'])
@pytest.mark.parametrize('width,hop', [(100, 50), (10, 5), (37, 11), (1, 1), (5, 9)])
def test_numpy_session_matches_the_oracle_chain(host_only, width, hop, reduction):
  rec = host_online.recipe(5, 2, 9)
  lda = LDA if reduction == 'lda' else None
  decoder = host_online.linear_decoder(5, 2, 9, rec['w'], rec['b'], rec['corr'][0], reduction, lda)
  want, wta, step = host_online.oracle_chain(rec, width, hop, reduction, lda)
  assert want.shape[0] == (host_online.FRAMES - width) // hop + 1
  for kind, truth in (('wta', wta), ('stepped', step)):
    got, decisions = _run(decoder, rec, [400, 0, 37, 1063], width, hop, kind)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    clear = np.abs(want[:, 0] - want[:, 1]) > 1e-10 * np.max(np.abs(want))
    if kind == 'wta':
      np.testing.assert_array_equal(decisions[clear].astype(bool), truth[clear])
    elif clear.all():
      np.testing.assert_array_equal(decisions.astype(bool), truth)


@pytest.mark.parametrize('c,pre,post,width,hop', [(5, 2, 9, 37, 11), (3, 0, 4, 5, 9), (4, 6, 0, 1, 1),
                                                   (2, 3, 3, 100, 50)])
def test_numpy_session_is_chunk_invariant(host_only, c, pre, post, width, hop):
  rec = host_online.recipe(c, pre, post)
  decoder = host_online.linear_decoder(c, pre, post, rec['w'], rec['b'], rec['corr'][0], 'mean-squared')
  cuts = host_online.chunkings(host_online.FRAMES, pre, post, width)
  rng = np.random.default_rng(7)
  cuts['random 0..300'] = []
  while sum(cuts['random 0..300']) < host_online.FRAMES:
    cuts['random 0..300'].append(int(min(rng.integers(0, 301), host_online.FRAMES - sum(cuts['random 0..300']))))
  for kind in ('wta', 'stepped'):
    whole = _run(decoder, rec, cuts['whole'], width, hop, kind)
    for name in ('ones', 'sevens', 'random 0..300', 'random', 'width+1'):
      got = _run(decoder, rec, cuts[name], width, hop, kind)
      np.testing.assert_array_equal(got[0], whole[0], err_msg=name)
      np.testing.assert_array_equal(got[1], whole[1], err_msg=name)


def test_a_bank_of_numpy_sessions_is_its_sessions(host_only):
  from telluride_decoding_amd import online
  rec = host_online.recipe(4, 2, 3)
  decoders = [host_online.linear_decoder(4, 2, 3, rec['w'] * scale, rec['b'], rec['corr'][0] * scale, 'first')
              for scale in (1.0, 0.5, 2.0)]
  bank = online.OnlineDecoder(decoders, 20, 10, decoder_type='stepped')
  singles = [online.OnlineDecoder(d, 20, 10, decoder_type='stepped') for d in decoders]
  eeg = np.stack([rec['eeg'][:300] * s for s in (1.0, 2.0, 3.0)])
  env1, env2 = np.stack([rec['env'][:300, 0]] * 3), np.stack([rec['env'][:300, 1]] * 3)
  for lo, hi in ((0, 130), (130, 131), (131, 300)):
    got = bank.push(eeg[:, lo:hi], env1[:, lo:hi], env2[:, lo:hi])
    for i, single in enumerate(singles):
      want = single.push(eeg[i, lo:hi], env1[i, lo:hi], env2[i, lo:hi])
      np.testing.assert_array_equal(got.scores[i], want.scores[0])
      np.testing.assert_array_equal(got.decisions[i], want.decisions[0])
  assert got.scores.shape[0] == 3 and got.scores.shape[2] == 2
  bank.reset()
  again = bank.push(eeg[:, :130], env1[:, :130], env2[:, :130])
  first = singles[0]
  first.reset()
  np.testing.assert_array_equal(again.scores[0], first.push(eeg[0, :130], env1[0, :130], env2[0, :130]).scores[0])


def test_constructor_refuses_what_the_online_path_does_not_do(host_only):
  from telluride_decoding_amd import brain_model, infer_decoder, online
  rec = host_online.recipe(4, 2, 3)
  good = host_online.linear_decoder(4, 2, 3, rec['w'], rec['b'], rec['corr'][0], 'first')
  online.OnlineDecoder(good, 100)
  assert online.OnlineDecoder(good, 100).window_step == 50
  # a CCA decoder, a DNN model, an unfitted model
  with pytest.raises(ValueError, match='CCA'):
    online.OnlineDecoder(infer_decoder.CCADecoder(None, reduction='first'), 100)
  dnn = brain_model.BrainModelDNN(brain_model._shape_dataset(4 * 6, 1, 1), [8])
  with pytest.raises(ValueError, match='DNN'):
    online.OnlineDecoder(infer_decoder.LinearRegressionDecoder(dnn, reduction='first'), 100)
  unfitted = brain_model.BrainModelLinearRegression(brain_model._shape_dataset(4, 1, 1, 2, 3))
  with pytest.raises(ValueError, match='fitted'):
    online.OnlineDecoder(infer_decoder.LinearRegressionDecoder(unfitted, reduction='first'), 100)
  # more than one output
  two = brain_model.BrainModelLinearRegression(brain_model._shape_dataset(4, 1, 2, 2, 3))
  two.set_weights([np.zeros((24, 2), np.float32), np.zeros(2, np.float32)])
  with pytest.raises(ValueError, match='one model output'):
    online.OnlineDecoder(infer_decoder.LinearRegressionDecoder(two, reduction='first'), 100)
  # reductions that need several outputs
  for reduction in ('all', 'second'):
    bad = host_online.linear_decoder(4, 2, 3, rec['w'], rec['b'], rec['corr'][0], reduction)
    with pytest.raises(ValueError, match=reduction):
      online.OnlineDecoder(bad, 100)
  # the kernel's limits, by name
  wide = host_online.linear_decoder(129, 0, 0, np.zeros(129), 0.0, (0.0, 0.0, 1.0))
  with pytest.raises(ValueError, match='128 channels'):
    online.OnlineDecoder(wide, 100)
  long = host_online.linear_decoder(2, 32, 32, np.zeros(130), 0.0, (0.0, 0.0, 1.0))
  with pytest.raises(ValueError, match='64 lags'):
    online.OnlineDecoder(long, 100)
  with pytest.raises(ValueError, match='65536'):
    online.OnlineDecoder(good, 65537)
  with pytest.raises(ValueError, match='window step'):
    online.OnlineDecoder(good, 1)                       # 1 // 2 = 0
  with pytest.raises(ValueError, match='Unknown type'):
    online.OnlineDecoder(good, 100, decoder_type='majority')
  with pytest.raises(ValueError, match='same channels'):
    online.OnlineDecoder([good, host_online.linear_decoder(4, 1, 3, rec['w'][:20], rec['b'], rec['corr'][0])], 100)
  with pytest.raises(ValueError, match='state-space'):
    online.OnlineDecoder(good, 100).tune([0.1, 0.2], [0.0, 0.1])
  # a push of the wrong shape
  dec = online.OnlineDecoder(good, 100)
  with pytest.raises(ValueError, match='A push is'):
    dec.push(np.zeros((10, 5), np.float32), np.zeros(10), np.zeros(10))
  with pytest.raises(ValueError, match='A push is'):
    dec.push(np.zeros((10, 4), np.float32), np.zeros(9), np.zeros(9))


def test_from_model_dir_is_the_live_decoder(host_only, tmp_path):
  from telluride_decoding_amd import infer_decoder, online
  rec = host_online.recipe(4, 2, 3)
  live = host_online.linear_decoder(4, 2, 3, rec['w'], rec['b'], rec['corr'][0], 'lda', LDA)
  model_dir = tmp_path / 'linear_model'
  model_dir.mkdir()
  live.save_parameters(str(model_dir / infer_decoder.DECODER_PARAM_FILE_NAME), decoding_model=live.decoding_model)
  loaded = online.OnlineDecoder.from_model_dir(str(model_dir), 'lda', 20, window_step=10, decoder_type='stepped')
  direct = online.OnlineDecoder(live, 20, 10, decoder_type='stepped')
  assert (loaded.channels, loaded.pre, loaded.post, loaded.reduction) == (4, 2, 3, 'lda')
  for lo, hi in ((0, 77), (77, 400)):
    got = loaded.push(rec['eeg'][lo:hi], rec['env'][lo:hi, 0], rec['env'][lo:hi, 1])
    want = direct.push(rec['eeg'][lo:hi], rec['env'][lo:hi, 0], rec['env'][lo:hi, 1])
    assert got.first_window == want.first_window
    np.testing.assert_array_equal(got.scores, want.scores)
    np.testing.assert_array_equal(got.decisions, want.decisions)
  assert got.scores.shape[1] > 0
