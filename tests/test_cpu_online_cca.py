"""The online CCA decoder without a GPU: the ctypes prototypes of td_cca_online_* against the header, the state
and LDS sizes against their formulas, and online.OnlineDecoder's NumPy CCA session -- against the oracle chain,
cut into pushes every way, as a bank -- and everything the constructor refuses."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online
from tests import host_online_cca as hc
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_cca_online_lds_bytes', 'td_cca_online_push', 'td_cca_online_state_bytes']
SMALL = hc.SHAPES[0]                      # (5,2,9 | 3,1,4 | 2)


def test_argtypes_match_the_header_prototypes():
  """td_cca_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py).  The names stay out of the td_online_* set that
  test pins, and the header's budget is the module's."""
  from telluride_decoding_amd import _lib, device
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_cca_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  assert sorted(set(re.findall(r'\bint\s+(td_online_\w+)\s*\(', text))) == sorted(
      ['td_online_plan', 'td_online_push', 'td_online_state_bytes'])
  for name in ENTRY_POINTS:
    assert not name.startswith('td_online_')
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
  cap = re.search(r'#define\s+TD_CCA_ONLINE_LDS_BYTES\s+(\d+)', raw)
  assert cap and int(cap.group(1)) == device.CCA_ONLINE_LDS_BYTES == 160 * 1024
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


def _lds_formula(c1, pre1, post1, c2, pre2, post2, dims, pass_):
  post = max(post1, post2)
  k1, k2 = c1 * (pre1 + 1 + post1), c2 * (pre2 + 1 + post2)
  r1 = max(pass_ + pre1 + post1, pre1 + post)
  r2 = max(pass_ + pre2 + post2, pre2 + post)
  return 32 * pass_ + 4 * ((dims + 1) * (k1 + k2) + r1 * c1 + 2 * r2 * c2 + 3 * dims * pass_)


def test_state_and_lds_bytes_are_the_formulas():
  from telluride_decoding_amd import device
  shapes = hc.SHAPES + [((64, 0, 20), (8, 0, 15), 5), ((1, 0, 0), (1, 0, 0), 1), ((128, 31, 32), (32, 31, 32), 1),
                        ((128, 10, 9), (32, 0, 63), 4)]
  for ((c1, pre1, post1), (c2, pre2, post2), dims), width in zip(shapes, (100, 10, 37, 1, 5, 65536, 100, 1, 4096, 7)):
    post = max(post1, post2)
    nbytes = device.cca_online_state_bytes(c1, pre1, post1, c2, pre2, post2, width)
    # the stepped decoder's state, the ring of both speakers' scores, the EEG tail, both speakers' feature tails
    need = 8 + 8 * 2 * width + 4 * c1 * (pre1 + post) + 4 * 2 * c2 * (pre2 + post)
    assert nbytes % 8 == 0 and need <= nbytes < need + 8, (c1, pre1, post1, c2, pre2, post2, width, nbytes)
    for emitted in (0, 1, 10, 64, 1500):
      pass_, lds = device.cca_online_lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, emitted)
      want = min(64, max(emitted, 1))
      while want > 1 and _lds_formula(c1, pre1, post1, c2, pre2, post2, dims, want) > device.CCA_ONLINE_LDS_BYTES:
        want = (want + 1) // 2
      assert pass_ == want and lds == _lds_formula(c1, pre1, post1, c2, pre2, post2, dims, pass_)
      assert lds <= device.CCA_ONLINE_LDS_BYTES
  # every test shape and the bench's lagged CCA shape run whole passes of 64 frames
  for (v1, v2, dims) in hc.SHAPES + [((64, 0, 20), (8, 0, 15), 5)]:
    assert device.cca_online_lds_bytes(*v1, *v2, dims, 1500)[0] == 64, (v1, v2, dims)
  # a pass shrinks before a shape is refused ...
  assert device.cca_online_lds_bytes(128, 20, 19, 32, 0, 0, 5, 1500)[0] == 16
  # ... and the refusal names the budget
  with pytest.raises(ValueError, match='budget 163840 bytes'):
    device.cca_online_lds_bytes(128, 31, 32, 32, 0, 0, 16, 1500)
  for bad in ((0, 0, 0, 1, 0, 0, 1), (129, 0, 0, 1, 0, 0, 1), (4, -1, 0, 1, 0, 0, 1), (4, 32, 32, 1, 0, 0, 1),
              (4, 0, 0, 0, 0, 0, 1), (4, 0, 0, 33, 0, 0, 1), (4, 0, 0, 1, 0, -1, 1), (4, 0, 0, 1, 60, 4, 1),
              (4, 0, 0, 1, 0, 0, 0), (4, 0, 0, 1, 0, 0, 65537)):
    with pytest.raises(ValueError, match='td_cca_online_state_bytes'):
      device.cca_online_state_bytes(*bad)


@pytest.fixture
def host_only(monkeypatch):
  """OnlineDecoder's NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def _push(dec, rec, lo, hi):
  return dec.push(rec['eeg'][lo:hi], rec['feat'][0, lo:hi], rec['feat'][1, lo:hi])


def _run(decoder, rec, sizes, width, hop, kind, **context):
  from telluride_decoding_amd import online
  dec = online.OnlineDecoder(decoder, width, hop, decoder_type=kind, **context)
  scores, decisions, firsts, at = [], [], [], 0
  for n in sizes:
    r = _push(dec, rec, at, at + n)
    at += n
    scores.append(r.scores[0]); decisions.append(r.decisions[0]); firsts.append(r.first_window)
  r = dec.flush()
  scores.append(r.scores[0]); decisions.append(r.decisions[0]); firsts.append(r.first_window)
  assert firsts == list(np.cumsum([0] + [len(s) for s in scores[:-1]]))
  with pytest.raises(ValueError, match='flushed'):
    _push(dec, rec, 0, 1)
  return np.concatenate(scores), np.concatenate(decisions)


@pytest.mark.parametrize('reduction', hc.REDUCTIONS)
@pytest.mark.parametrize('width,hop', hc.WINDOWS[:5])
def test_numpy_session_matches_the_oracle_chain(host_only, width, hop, reduction):
  rec = hc.recipe(*SMALL)
  decoder = hc.decoder_of(rec, reduction)
  want, wta, step = hc.oracle_chain(rec, width, hop, reduction)
  assert want.shape[0] == (hc.FRAMES - width) // hop + 1
  for kind, truth in (('wta', wta), ('stepped', step)):
    got, decisions = _run(decoder, rec, [400, 0, 37, 1063], width, hop, kind)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    clear = np.abs(want[:, 0] - want[:, 1]) > 1e-10 * np.max(np.abs(want))
    if kind == 'wta':
      np.testing.assert_array_equal(decisions[clear].astype(bool), truth[clear])
    elif clear.all():
      np.testing.assert_array_equal(decisions.astype(bool), truth)


@pytest.mark.parametrize('view1,view2,dims,width,hop', [((5, 2, 9), (3, 1, 4), 2, 37, 11), ((3, 0, 4), (2, 3, 6), 2, 5, 9),
                                                        ((4, 6, 0), (1, 1, 0), 1, 1, 1), ((2, 3, 3), (4, 0, 3), 4, 100, 50),
                                                        ((5, 0, 0), (16, 0, 0), 16, 10, 5)])
def test_numpy_session_is_chunk_invariant(host_only, view1, view2, dims, width, hop):
  """Array equality for pushes of 1, of 7, one row short of each view's tail, one push of width + 1, seeded
  random sizes with zeros and the whole recording -- the view that sets the delay being either one."""
  rec = hc.recipe(view1, view2, dims)
  decoder = hc.decoder_of(rec, 'lda')
  cuts = hc.chunkings(view1, view2, width)
  for kind in ('wta', 'stepped'):
    whole = _run(decoder, rec, cuts['whole'], width, hop, kind)
    assert whole[0].shape == ((hc.FRAMES - width) // hop + 1, 2)
    for name in sorted(set(cuts) - {'whole'}):
      got = _run(decoder, rec, cuts[name], width, hop, kind)
      np.testing.assert_array_equal(got[0], whole[0], err_msg=name)
      np.testing.assert_array_equal(got[1], whole[1], err_msg=name)


def test_a_bank_of_numpy_sessions_is_its_sessions(host_only):
  from telluride_decoding_amd import online
  view1, view2, dims = (4, 2, 3), (2, 1, 5), 2
  rec = hc.recipe(view1, view2, dims)
  decoders = [hc.cca_decoder(view1, view2, rec['mean_x'] * scale, rec['rot_x'] * scale, rec['mean_y'],
                             rec['rot_y'], rec['corr'][0] * scale, 'lda', rec['lda'] * scale)
              for scale in (1.0, 0.5, 2.0)]
  bank = online.OnlineDecoder(decoders, 20, 10, decoder_type='stepped')
  singles = [online.OnlineDecoder(d, 20, 10, decoder_type='stepped') for d in decoders]
  assert (bank.kind, bank.sessions, bank.delay) == ('cca', 3, 5)
  eeg = np.stack([rec['eeg'][:300] * s for s in (1.0, 2.0, 3.0)])
  f1, f2 = np.stack([rec['feat'][0, :300]] * 3), np.stack([rec['feat'][1, :300]] * 3)
  for lo, hi in ((0, 130), (130, 131), (131, 300)):
    got = bank.push(eeg[:, lo:hi], f1[:, lo:hi], f2[:, lo:hi])
    for i, single in enumerate(singles):
      want = single.push(eeg[i, lo:hi], f1[i, lo:hi], f2[i, lo:hi])
      np.testing.assert_array_equal(got.scores[i], want.scores[0])
      np.testing.assert_array_equal(got.decisions[i], want.decisions[0])
  assert got.scores.shape[0] == 3 and got.scores.shape[2] == 2 and got.scores.shape[1] > 0
  bank.reset()
  again = bank.push(eeg[:, :130], f1[:, :130], f2[:, :130])
  first = singles[0]
  first.reset()
  np.testing.assert_array_equal(again.scores[0], first.push(eeg[0, :130], f1[0, :130], f2[0, :130]).scores[0])


def test_the_context_comes_from_the_decoder_or_from_keywords(host_only):
  rec = hc.recipe(*SMALL)
  carried = _run(hc.decoder_of(rec, 'mean'), rec, [700, 800], 37, 11, 'wta')
  by_keyword = _run(hc.decoder_of(rec, 'mean', carry=False), rec, [700, 800], 37, 11, 'wta',
                    **hc.context_of(SMALL[0], SMALL[1]))
  np.testing.assert_array_equal(carried[0], by_keyword[0])
  np.testing.assert_array_equal(carried[1], by_keyword[1])
  from telluride_decoding_amd import online
  with pytest.raises(TypeError, match='unknown context argument'):
    online.OnlineDecoder(hc.decoder_of(rec, 'mean', carry=False), 37, 11, pre_contxt=2)
  # without a context the 60 columns of the EEG view are 60 channels at one lag
  assert online.OnlineDecoder(hc.decoder_of(rec, 'mean', carry=False), 37, 11).channels == 60


def test_from_model_dir_is_the_live_decoder(host_only, tmp_path):
  from telluride_decoding_amd import infer_decoder, online
  rec = hc.recipe(*SMALL)
  live = hc.decoder_of(rec, 'lda')
  live.decoding_model.add_metadata(hc.context_of(SMALL[0], SMALL[1]))
  model_dir = tmp_path / 'cca_model'
  model_dir.mkdir()
  live.save_parameters(str(model_dir / infer_decoder.DECODER_PARAM_FILE_NAME), decoding_model=live.decoding_model)
  loaded = online.OnlineDecoder.from_model_dir(str(model_dir), 'lda', 20, window_step=10, decoder_type='stepped')
  direct = online.OnlineDecoder(live, 20, 10, decoder_type='stepped')
  assert (loaded.kind, loaded.channels, loaded.pre, loaded.post, loaded.reduction) == ('cca', 5, 2, 9, 'lda')
  assert (loaded.features, loaded.pre2, loaded.post2, loaded.dims) == (3, 1, 4, 2)
  for lo, hi in ((0, 77), (77, 400)):
    got, want = _push(loaded, rec, lo, hi), _push(direct, rec, lo, hi)
    assert got.first_window == want.first_window
    np.testing.assert_array_equal(got.scores, want.scores)
    np.testing.assert_array_equal(got.decisions, want.decisions)
  assert got.scores.shape[1] > 0


def test_constructor_refuses_what_the_online_path_does_not_do(host_only):
  from telluride_decoding_amd import brain_model, cca, infer_decoder, online
  rec = hc.recipe(*SMALL)
  view1, view2, dims = SMALL
  good = hc.decoder_of(rec, 'first')
  assert online.OnlineDecoder(good, 100).window_step == 50
  stats = rec['corr'][0]

  def shaped(v1, v2, d, reduction='first', lda=None):
    k1, k2 = v1[0] * (v1[1] + 1 + v1[2]), v2[0] * (v2[1] + 1 + v2[2])
    return hc.cca_decoder(v1, v2, np.zeros(k1), np.zeros((k1, d)), np.zeros(k2), np.zeros((k2, d)),
                          np.ones((3, d)), reduction, lda)

  # no model, an unfitted model: the messages tests/test_cpu_online.py pins
  with pytest.raises(ValueError, match='CCA'):
    online.OnlineDecoder(infer_decoder.CCADecoder(None, reduction='first'), 100)
  unfitted = cca.BrainModelCCA(brain_model._shape_dataset(60, 18, 1), cca_dims=2)
  with pytest.raises(ValueError, match='fitted CCA'):
    online.OnlineDecoder(infer_decoder.CCADecoder(unfitted, reduction='first'), 100)
  # a bank is all linear or all CCA, with one shape
  linear = host_online.linear_decoder(5, 2, 9, np.zeros(60), 0.0, (0.0, 0.0, 1.0))
  with pytest.raises(ValueError, match='all linear or all CCA'):
    online.OnlineDecoder([good, linear], 100)
  with pytest.raises(ValueError, match='all linear or all CCA'):
    online.OnlineDecoder([linear, good], 100)
  for other in (shaped((5, 2, 9), (3, 1, 4), 3), shaped((5, 2, 9), (3, 2, 3), 2), shaped((5, 2, 9), (6, 1, 1), 2),
                shaped((6, 1, 8), (3, 1, 4), 2), hc.decoder_of(rec, 'mean')):
    with pytest.raises(ValueError, match='same channels, features, contexts, dims and reduction'):
      online.OnlineDecoder([good, other], 100)
  with pytest.raises(ValueError, match='same channels'):        # (the linear bank's message stays)
    online.OnlineDecoder([linear, host_online.linear_decoder(5, 1, 9, np.zeros(55), 0.0, (0.0, 0.0, 1.0))], 100)
  # reductions
  with pytest.raises(ValueError, match='all'):
    online.OnlineDecoder(hc.decoder_of(rec, 'all'), 100)
  with pytest.raises(ValueError, match='\'second\' needs at least 2 dims'):
    online.OnlineDecoder(shaped((3, 31, 32), (1, 5, 2), 1, 'second'), 100)
  with pytest.raises(ValueError, match='LDA'):
    online.OnlineDecoder(shaped((5, 2, 9), (3, 1, 4), 2, 'lda'), 100)
  # the kernel's limits, by name
  with pytest.raises(ValueError, match='128 channels'):
    online.OnlineDecoder(shaped((129, 0, 0), (3, 0, 0), 2), 100)
  with pytest.raises(ValueError, match='32 features'):
    online.OnlineDecoder(shaped((5, 0, 0), (33, 0, 0), 2), 100)
  with pytest.raises(ValueError, match='64 lags'):
    online.OnlineDecoder(shaped((2, 32, 32), (3, 0, 0), 2), 100)
  with pytest.raises(ValueError, match='64 lags'):
    online.OnlineDecoder(shaped((2, 0, 0), (3, 60, 4), 2), 100)
  with pytest.raises(ValueError, match='16 dims'):
    online.OnlineDecoder(shaped((5, 2, 9), (3, 1, 4), 17), 100)
  with pytest.raises(ValueError, match='budget 163840 bytes'):
    online.OnlineDecoder(shaped((128, 31, 32), (3, 0, 0), 16), 100)
  with pytest.raises(ValueError, match='rotations of'):          # (60 columns are not 7 lags of anything)
    online.OnlineDecoder(hc.decoder_of(rec, 'first', carry=False), 100, pre_context=3, post_context=3)
  with pytest.raises(ValueError, match='65536'):
    online.OnlineDecoder(good, 65537)
  with pytest.raises(ValueError, match='window step'):
    online.OnlineDecoder(good, 1)
  with pytest.raises(ValueError, match='Unknown type'):
    online.OnlineDecoder(good, 100, decoder_type='majority')
  with pytest.raises(ValueError, match='state-space'):
    online.OnlineDecoder(good, 100).tune([0.1, 0.2], [0.0, 0.1])
  # pushes of the wrong shape
  dec = online.OnlineDecoder(good, 100)
  n = 10
  eeg, feat = np.zeros((n, 5), np.float32), np.zeros((n, 3), np.float32)
  dec.push(eeg, feat, feat)
  for bad in ((np.zeros((n, 6), np.float32), feat, feat), (eeg, np.zeros((n, 2), np.float32), feat),
              (eeg, feat, np.zeros((n - 1, 3), np.float32)), (eeg, np.zeros(n), np.zeros(n)),
              (np.zeros((2, n, 5), np.float32), feat, feat)):
    with pytest.raises(ValueError, match='A push is'):
      dec.push(*bad)
