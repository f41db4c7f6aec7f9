"""The online DNN decoder without a GPU: the ctypes prototypes of td_fc_online_* against the header, the LDS size
against its formula, what session_parameters takes from a LinearRegressionDecoder around a BrainModelDNN and what
it refuses, and online.OnlineDecoder's NumPy DNN session -- against the oracle chain, against the linear session,
cut into pushes every way, as a bank, from a saved model directory."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_dnn
from tests import host_online
from tests import host_online_dnn as hd
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_fc_online_lds_bytes', 'td_fc_online_push']
SMALL = hd.SHAPES[0]                      # (5, 2, 9), [16]


def test_argtypes_match_the_header_prototypes():
  """td_fc_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py).  The names stay out of the td_online_*, td_mlp_* and
  td_dnn_* sets other tests pin, and the header's budget is the module's."""
  from telluride_decoding_amd import _lib, device
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_fc_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  for name in ENTRY_POINTS:
    assert not re.fullmatch(r'td_(mlpc?|dnn|online)_\w+', name)
    assert name in _lib.header_symbols()
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
  cap = re.search(r'#define\s+TD_FC_ONLINE_LDS_BYTES\s+(\d+)', raw)
  assert cap and int(cap.group(1)) == device.DNN_ONLINE_LDS_BYTES == 160 * 1024
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


def _lds_formula(c, pre, post, hidden, pass_):
  k = c * (pre + 1 + post)
  widths = [k] + list(hidden) + [1]
  ks, slices = hd.slices_of(k)
  nj = -(-widths[1] // 4) * 4
  g = min(slices, 4096 // (ks * nj))
  n_small = sum(widths[i] * widths[i + 1] + widths[i + 1] for i in range(len(widths) - 1)) - k * widths[1]
  lda = max(list(hidden) + [1]) | 1
  return 32 * pass_ + 4 * (2 * g * ks * nj + -(-n_small // 4) * 4 + (pass_ + pre + post) * (c | 1) +
                           2 * max(pass_, post) + pass_ + 2 * pass_ * lda)


def test_lds_bytes_are_the_formula_and_the_limits_are_named():
  from telluride_decoding_amd import device
  shapes = hd.SHAPES + [((64, 0, 20), [64, 64]), ((128, 31, 32), [64, 64, 64, 64]), ((128, 31, 32), [])]
  for (c, pre, post), hidden in shapes:
    for emitted in (0, 1, 10, 64, 1500):
      pass_, lds = device.dnn_online_lds_bytes(c, pre, post, hidden, emitted)
      want = min(64, max(emitted, 1))
      while want > 1 and _lds_formula(c, pre, post, hidden, want) > device.DNN_ONLINE_LDS_BYTES:
        want = (want + 1) // 2
      assert pass_ == want and lds == _lds_formula(c, pre, post, hidden, pass_), ((c, pre, post), hidden, emitted)
      assert lds <= device.DNN_ONLINE_LDS_BYTES
  # the timed model runs whole passes of 64 frames; the largest input under the largest head halves them
  assert device.dnn_online_lds_bytes(64, 0, 20, [64, 64], 1500)[0] == 64
  assert device.dnn_online_lds_bytes(128, 31, 32, [64, 64, 64, 64], 1500)[0] == 32
  for bad, what in (((0, 0, 0, [4]), 'channels'), ((129, 0, 0, [4]), 'channels'), ((4, -1, 0, [4]), 'lags'),
                    ((4, 0, -1, [4]), 'lags'), ((4, 32, 32, [4]), 'lags'), ((4, 0, 0, [4] * 5), 'hidden layers'),
                    ((4, 0, 0, [0]), 'units'), ((4, 0, 0, [4, 65]), 'units')):
    with pytest.raises(ValueError, match='td_fc_online_lds_bytes.*' + what):
      device.dnn_online_lds_bytes(*bad)
  with pytest.raises(ValueError, match='td_fc_online_lds_bytes'):
    device.dnn_online_lds_bytes(4, 0, 0, [4], -1)
  assert device.dnn_param_count(60, [16]) == 60 * 16 + 16 + 16 + 1
  assert device.dnn_param_count(60, []) == 61


@pytest.fixture
def host_only(monkeypatch):
  """OnlineDecoder's NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def _run(decoder, rec, sizes, width, hop, kind, **context):
  from telluride_decoding_amd import online
  dec = online.OnlineDecoder(decoder, width, hop, decoder_type=kind, **context)
  assert dec.kind == 'dnn'
  scores, decisions, firsts, at = [], [], [], 0
  for n in sizes:
    r = dec.push(rec['eeg'][at:at + n], rec['env'][at:at + n, 0], rec['env'][at:at + n, 1])
    at += n
    scores.append(r.scores[0]); decisions.append(r.decisions[0]); firsts.append(r.first_window)
  r = dec.flush()
  scores.append(r.scores[0]); decisions.append(r.decisions[0]); firsts.append(r.first_window)
  assert firsts == list(np.cumsum([0] + [len(s) for s in scores[:-1]]))
  with pytest.raises(ValueError, match='flushed'):
    dec.push(rec['eeg'][:1], rec['env'][:1, 0], rec['env'][:1, 1])
  return np.concatenate(scores), np.concatenate(decisions)


def test_session_parameters_takes_the_context_from_each_of_its_sources(host_only):
  from telluride_decoding_amd import online
  rec = hd.model(*SMALL)
  got = {}
  for carry, context in (('params', {}), ('metadata', {}), (None, dict(pre_context=2, post_context=9))):
    p = online.session_parameters(hd.decoder_of(rec, 'mean', carry=carry), **context)
    assert (p['kind'], p['c'], p['pre'], p['post'], p['hidden'], p['reduction']) == ('dnn', 5, 2, 9, [16], 'mean')
    assert p['params'].dtype == np.float32 and p['params'].tobytes() == hd.packed(rec['weights']).tobytes()
    np.testing.assert_array_equal(p['corr'], rec['corr'])
    assert p['lda'] is None
    got[carry] = _run(hd.decoder_of(rec, 'mean', carry=carry), rec, [700, 800], 37, 11, 'wta', **context)
  for carry in ('metadata', None):
    np.testing.assert_array_equal(got[carry][0], got['params'][0])
    np.testing.assert_array_equal(got[carry][1], got['params'][1])
  assert got['params'][0].shape == ((hd.FRAMES - 37) // 11 + 1, 2)
  # what the decoder carries wins over the keywords; the lda parameters are the decoder's
  p = online.session_parameters(hd.decoder_of(rec, 'lda', hd.LDA), pre_context=0, post_context=11)
  assert (p['pre'], p['post']) == (2, 9)
  np.testing.assert_array_equal(p['lda'], np.array(hd.LDA))
  # the linear session's context stays its own
  lin = host_online.recipe(*SMALL[0])
  with pytest.raises(TypeError, match='carries its own'):
    online.session_parameters(host_online.linear_decoder(5, 2, 9, lin['w'], lin['b'], lin['corr'][0]), pre_context=2)


def test_session_parameters_refuses_by_name(host_only):
  from telluride_decoding_amd import brain_model, infer_decoder, online
  rec = hd.model(*SMALL)
  stats = rec['corr'][0]

  def shaped(c, pre, post, hidden, **kwargs):
    return hd.dnn_decoder(c, pre, post, hidden, host_dnn.glorot([c * (pre + 1 + post)] + hidden +
                                                                [kwargs.get('outputs', 1)], 0), stats, **kwargs)

  # no context anywhere: the message names the model kind and the two keywords (tests/test_cpu_online.py's case)
  bare = infer_decoder.LinearRegressionDecoder(brain_model.BrainModelDNN(brain_model._shape_dataset(24, 1, 1), [8]),
                                               reduction='first')
  for context in ({}, dict(pre_context=2), dict(post_context=3)):
    with pytest.raises(ValueError, match='DNN model does not carry its context.*pre_context=.*post_context='):
      online.OnlineDecoder(bare, 100, **context)
  assert online.OnlineDecoder(bare, 100, pre_context=2, post_context=3).channels == 4
  with pytest.raises(TypeError, match='unknown context argument input2_pre_context'):
    online.OnlineDecoder(bare, 100, pre_context=2, post_context=3, input2_pre_context=0)
  with pytest.raises(ValueError, match='input_offset of 0, not 3'):
    online.OnlineDecoder(shaped(5, 2, 9, [16], input_offset=3), 100)
  with pytest.raises(ValueError, match='24 inputs: no multiple of the 2 \\+ 1 \\+ 2 lags'):
    online.OnlineDecoder(bare, 100, pre_context=2, post_context=2)
  with pytest.raises(ValueError, match='one model output, not 2'):
    online.OnlineDecoder(shaped(5, 2, 9, [16], outputs=2), 100)
  with pytest.raises(ValueError, match='1 to 128 channels, not 129'):
    online.OnlineDecoder(shaped(129, 0, 0, [4]), 100)
  with pytest.raises(ValueError, match='at most 64 lags, not 32 \\+ 1 \\+ 32'):
    online.OnlineDecoder(shaped(2, 32, 32, [4]), 100)
  with pytest.raises(ValueError, match='at most 64 lags'):
    online.OnlineDecoder(bare, 100, pre_context=-1, post_context=0)
  with pytest.raises(ValueError, match='at most 4 hidden layers, not 5'):
    online.OnlineDecoder(shaped(5, 2, 9, [4] * 5), 100)
  with pytest.raises(ValueError, match='hidden layers of 1 to 64 units'):
    online.OnlineDecoder(shaped(5, 2, 9, [16, 65]), 100)
  for reduction in ('all', 'second'):
    with pytest.raises(ValueError, match='reduces one output with'):
      online.OnlineDecoder(hd.decoder_of(rec, reduction), 100)
  # the session's own limits keep their messages
  good = hd.decoder_of(rec)
  assert online.OnlineDecoder(good, 100).window_step == 50
  with pytest.raises(ValueError, match='65536'):
    online.OnlineDecoder(good, 65537)
  with pytest.raises(ValueError, match='Unknown type'):
    online.OnlineDecoder(good, 100, decoder_type='majority')
  with pytest.raises(_lib_unavailable(), match='state-space'):
    online.OnlineDecoder(good, 100, decoder_type='ssd')
  dec = online.OnlineDecoder(good, 100)
  with pytest.raises(ValueError, match='A push is'):
    dec.push(np.zeros((10, 6), np.float32), np.zeros(10), np.zeros(10))


def _lib_unavailable():
  from telluride_decoding_amd import _lib
  return _lib.HotPathUnavailable


@pytest.mark.parametrize('shape,hidden,width,hop', [((5, 2, 9), [16], 37, 11), ((3, 0, 4), [5, 3], 5, 9),
                                                    ((4, 6, 0), [], 1, 1), ((2, 3, 3), [7, 1, 6], 100, 50),
                                                    ((1, 0, 0), [3], 10, 5)])
def test_numpy_session_is_chunk_invariant(host_only, shape, hidden, width, hop):
  """Array equality with one push for every cut of host_online.chunkings: pushes of 1, of 7, one row short of the
  tail, one push of width + 1, seeded random sizes with zeros."""
  rec = hd.model(shape, hidden)
  decoder = hd.decoder_of(rec, 'lda', hd.LDA)
  cuts = host_online.chunkings(hd.FRAMES, shape[1], shape[2], width, seed=shape[0])
  for kind in ('wta', 'stepped'):
    whole = _run(decoder, rec, cuts['whole'], width, hop, kind)
    assert whole[0].shape == ((hd.FRAMES - width) // hop + 1, 2)
    for name in sorted(set(cuts) - {'whole'}):
      got = _run(decoder, rec, cuts[name], width, hop, kind)
      np.testing.assert_array_equal(got[0], whole[0], err_msg=name)
      np.testing.assert_array_equal(got[1], whole[1], err_msg=name)


@pytest.mark.parametrize('reduction', ['first', 'mean', 'mean-squared', 'lda'])
@pytest.mark.parametrize('width,hop', hd.WINDOWS)
def test_numpy_session_matches_the_oracle_chain(host_only, width, hop, reduction):
  """host_dnn.forward -> Correlator.correlate -> reduction -> windowed_means -> wta_sequence / step_sequence, all
  float64, on dnn_recipe: 1e-9."""
  rec = hd.dnn_recipe(host_online.recipe(*SMALL[0]), SMALL[1])
  lda = hd.LDA if reduction == 'lda' else None
  decoder = hd.decoder_of(rec, reduction, lda)
  want, wta, step = host_online.oracle_chain(rec, width, hop, reduction, lda)
  assert want.shape[0] == (hd.FRAMES - width) // hop + 1
  if (width, hop, reduction) == (100, 50, 'first'):
    # the recipe is a real non-linear model that decodes: its prediction follows the linear recipe's (the +-w pair)
    # without being it (the other units), and the oracle's decisions follow the attended speaker
    lin = host_online.recipe(*SMALL[0])
    p, q = rec['pred64'][:, 0], np.reshape(lin['pred64'], -1)
    assert np.corrcoef(p, q)[0, 1] > 0.9 and np.max(np.abs(p - q)) > 1e-3 * np.max(np.abs(q))
    attended_first = (np.arange(len(wta)) * hop + hop) < host_online.SWITCH
    assert np.mean(np.asarray(wta).astype(bool) == attended_first) > 0.8
  for kind, truth in (('wta', wta), ('stepped', step)):
    got, decisions = _run(decoder, rec, [400, 0, 37, 1063], width, hop, kind)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.max(np.abs(want)))
    clear = np.abs(want[:, 0] - want[:, 1]) > 1e-8 * np.max(np.abs(want))
    if kind == 'wta':
      np.testing.assert_array_equal(decisions[clear].astype(bool), truth[clear])
    elif clear.all():
      np.testing.assert_array_equal(decisions.astype(bool), truth)


def test_a_hidden_pair_holding_the_linear_model_is_the_linear_session(host_only):
  """hidden [2] with units +w / -w and output weights (+1, -1): relu(z) - relu(-z) = z, so the DNN session agrees
  with the linear _HostSession at 1e-9."""
  from telluride_decoding_amd import online
  c, pre, post = SMALL[0]
  lin = host_online.recipe(c, pre, post)
  dnn = hd.dnn_decoder(c, pre, post, [2], hd.linear_as_dnn(lin), lin['corr'][0], 'mean-squared')
  linear = host_online.linear_decoder(c, pre, post, lin['w'], lin['b'], lin['corr'][0], 'mean-squared')
  for kind, (width, hop) in (('wta', (37, 11)), ('stepped', (10, 5))):
    a = online.OnlineDecoder(dnn, width, hop, decoder_type=kind)
    b = online.OnlineDecoder(linear, width, hop, decoder_type=kind)
    assert (a.kind, b.kind) == ('dnn', 'linear')
    at = 0
    for n in (333, 7, 0, 1160):
      args = (lin['eeg'][at:at + n], lin['env'][at:at + n, 0], lin['env'][at:at + n, 1])
      ra, rb = a.push(*args), b.push(*args)
      at += n
      assert ra.first_window == rb.first_window and ra.scores.shape == rb.scores.shape
      np.testing.assert_allclose(ra.scores, rb.scores, rtol=1e-9, atol=1e-9 * np.max(np.abs(lin['corr'])))
      np.testing.assert_array_equal(ra.decisions, rb.decisions)
    ra, rb = a.flush(), b.flush()
    np.testing.assert_allclose(ra.scores, rb.scores, rtol=1e-9, atol=1e-9)


def test_a_bank_of_numpy_sessions_is_its_sessions(host_only):
  from telluride_decoding_amd import online
  shape, hidden = (4, 2, 3), [6, 3]
  rec = hd.model(shape, hidden)
  decoders = [hd.dnn_decoder(*shape, hidden, hd.glorot_model(*shape, hidden, seed), rec['corr'][0] * scale, 'lda',
                             np.array(hd.LDA) * scale) for seed, scale in ((5, 1.0), (6, 0.5), (7, 2.0))]
  bank = online.OnlineDecoder(decoders, 20, 10, decoder_type='stepped')
  singles = [online.OnlineDecoder(d, 20, 10, decoder_type='stepped') for d in decoders]
  assert (bank.kind, bank.sessions, bank.delay, bank.hidden) == ('dnn', 3, 3, [6, 3])
  eeg = np.stack([rec['eeg'][:300] * s for s in (1.0, 2.0, 3.0)])
  e1, e2 = np.stack([rec['env'][:300, 0]] * 3), np.stack([rec['env'][:300, 1]] * 3)
  for lo, hi in ((0, 130), (130, 131), (131, 300)):
    got = bank.push(eeg[:, lo:hi], e1[:, lo:hi], e2[:, lo:hi])
    for i, single in enumerate(singles):
      want = single.push(eeg[i, lo:hi], e1[i, lo:hi], e2[i, lo:hi])
      np.testing.assert_array_equal(got.scores[i], want.scores[0])
      np.testing.assert_array_equal(got.decisions[i], want.decisions[0])
  assert got.scores.shape[0] == 3 and got.scores.shape[2] == 2 and got.scores.shape[1] > 0
  assert not np.array_equal(got.scores[0], got.scores[1])
  bank.reset()
  again = bank.push(eeg[:, :130], e1[:, :130], e2[:, :130])
  singles[0].reset()
  np.testing.assert_array_equal(again.scores[0], singles[0].push(eeg[0, :130], e1[0, :130], e2[0, :130]).scores[0])


def test_mixed_banks_are_refused(host_only):
  from telluride_decoding_amd import online
  rec = hd.model(*SMALL)
  good = hd.decoder_of(rec)
  lin = host_online.recipe(*SMALL[0])
  linear = host_online.linear_decoder(5, 2, 9, lin['w'], lin['b'], lin['corr'][0])
  for pair in ([good, linear], [linear, good]):
    with pytest.raises(ValueError, match='all linear or all CCA or all DNN'):
      online.OnlineDecoder(pair, 100)
  stats = rec['corr'][0]
  other = lambda c, pre, post, hidden, **kw: hd.dnn_decoder(
      c, pre, post, hidden, host_dnn.glorot([c * (pre + 1 + post)] + hidden + [1], 0), stats, **kw)
  with pytest.raises(ValueError, match='same hidden layers: \\[16\\] and \\[16, 4\\]'):
    online.OnlineDecoder([good, other(5, 2, 9, [16, 4])], 100)
  with pytest.raises(ValueError, match='same hidden layers'):
    online.OnlineDecoder([good, other(5, 2, 9, [8])], 100)
  for mate in (other(6, 1, 8, [16]), other(5, 3, 8, [16]), other(5, 2, 9, [16], reduction='mean')):
    with pytest.raises(ValueError, match='same channels, context and reduction'):
      online.OnlineDecoder([good, mate], 100)


def test_from_model_dir_is_the_live_decoder(host_only, tmp_path):
  """model.save + save_parameters into a directory whose name holds `fullyconnected` (create_decoder's tag rule):
  the loaded session is the live one, with the context from the saved add_metadata entry."""
  from telluride_decoding_amd import infer_decoder, online
  rec = hd.model(*SMALL)
  live = hd.decoder_of(rec, 'lda', hd.LDA, carry='metadata')
  model_dir = tmp_path / 'fullyconnected_model'
  model_dir.mkdir()
  live.decoding_model.save(str(model_dir))
  live.save_parameters(str(model_dir / infer_decoder.DECODER_PARAM_FILE_NAME))
  loaded = online.OnlineDecoder.from_model_dir(str(model_dir), 'lda', 20, window_step=10, decoder_type='stepped')
  direct = online.OnlineDecoder(live, 20, 10, decoder_type='stepped')
  assert (loaded.kind, loaded.channels, loaded.pre, loaded.post, loaded.hidden, loaded.reduction) == (
      'dnn', 5, 2, 9, [16], 'lda')
  for lo, hi in ((0, 77), (77, 400)):
    args = (rec['eeg'][lo:hi], rec['env'][lo:hi, 0], rec['env'][lo:hi, 1])
    got, want = loaded.push(*args), direct.push(*args)
    assert got.first_window == want.first_window
    np.testing.assert_array_equal(got.scores, want.scores)
    np.testing.assert_array_equal(got.decisions, want.decisions)
  assert got.scores.shape[1] > 0


def test_device_tensor_inputs_reach_the_numpy_session(host_only):
  import torch
  from telluride_decoding_amd import online
  rec = hd.model(*SMALL)
  a = online.OnlineDecoder(hd.decoder_of(rec), 10, 5)
  b = online.OnlineDecoder(hd.decoder_of(rec), 10, 5)
  args = (rec['eeg'][:200], rec['env'][:200, 0], rec['env'][:200, 1])
  ra, rb = a.push(*[torch.as_tensor(v) for v in args]), b.push(*args)
  np.testing.assert_array_equal(ra.scores, rb.scores)
  with pytest.raises(ValueError, match='state-space'):
    a.tune([0.1, 0.2], [0.0, 0.1])
