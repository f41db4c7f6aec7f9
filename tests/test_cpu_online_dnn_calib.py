"""The online DNN calibration without a GPU: the ctypes prototypes of td_fccalib_online_* against the header, the state
size against td_calib_online_state_bytes, the LDS of a launch against the restated formula, every limit by name,
online.OnlineDNNCalibration's NumPy session -- against the frame-order twin fed its own float64 predictions bit for
bit, cut into pushes every way and flushed both ways, finish against the closed form and the two-pass float64 route,
refusing by name and going on, as a bank of three models, into a LinearRegressionDecoder -- and
OnlineDecoder.set_statistics on the host DNN bank with what finish gives."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online_calib as hoc
from tests import host_online_dnn as hd
from tests import host_online_dnn_calib as hdc
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_fccalib_online_lds_bytes', 'td_fccalib_online_push', 'td_fccalib_online_state_bytes']
SMALL = ((5, 2, 9), [16])


@pytest.fixture
def host_only(monkeypatch):
  """OnlineDNNCalibration's (and OnlineDecoder's) NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def test_argtypes_match_the_header_prototypes():
  """td_fccalib_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online_calib.py); the three names stay out of the td_online_*,
  td_fc_online_* and td_calib_online_* sets, which other tests pin as closed and which still hold what they held."""
  from telluride_decoding_amd import _lib
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_fccalib_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert not re.fullmatch(r'td_(online|cca_online|fc_online|calib_online|ccacalib_online|fit_online)_\w+', name)
    assert name in _lib.header_symbols()
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
  for family, names in (('td_online_', ['td_online_plan', 'td_online_push', 'td_online_state_bytes']),
                        ('td_fc_online_', ['td_fc_online_lds_bytes', 'td_fc_online_push']),
                        ('td_calib_online_', ['td_calib_online_finish', 'td_calib_online_push',
                                              'td_calib_online_state_bytes', 'td_calib_online_sums'])):
    assert sorted(set(re.findall(r'\bint\s+(%s\w+)\s*\(' % family, text))) == names, family


def test_state_bytes_are_the_linear_calibrations():
  """The state block is td_calib_online_push's: the same byte count at every shape, the limits by name."""
  from telluride_decoding_amd import device
  for shape in ((3, 0, 0), (1, 0, 0), (5, 2, 9), (64, 0, 20), (128, 31, 32)):
    assert device.online_dnn_calib_state_bytes(*shape) == device.online_calib_state_bytes(*shape), shape
  for bad in ((0, 0, 0), (129, 0, 0), (4, -1, 0), (4, 0, -1), (4, 32, 32), (4, 0, 64)):
    with pytest.raises(ValueError, match='td_fccalib_online_state_bytes'):
      device.online_dnn_calib_state_bytes(*bad)


def test_lds_bytes_are_the_formula_and_every_limit_is_named():
  """(pass, bytes) at tests/host_online_dnn.SHAPES and the two largest heads: the restated formula, 64 frames halved
  until 160 KB hold.  The limits by name: channels and lags (with at most 128 channels and 64 lags K = 8192 is the
  most a shape can reach, so `K > 8192` arrives as one of these two), 5 hidden layers, layers of 0 and 65 units.  No
  shape inside these limits exceeds the budget at a pass of one frame -- the largest takes 117 300 bytes -- so that
  refusal cannot be provoked; the formula's value is asserted under the budget instead."""
  from telluride_decoding_amd import device
  shapes = hd.SHAPES + [((64, 0, 20), [64, 64]), ((128, 31, 32), [64, 64, 64, 64]), ((63, 40, 5), [64, 64, 64, 64])]
  halved = []
  for (c, pre, post), hidden in shapes:
    for emitted in (0, 1, 10, 64, 1500):
      got = device.online_dnn_calib_lds_bytes(c, pre, post, hidden, emitted)
      assert got == hdc.lds_plan(c, pre, post, hidden, emitted), ((c, pre, post), hidden, emitted)
      assert got == device.dnn_online_lds_bytes(c, pre, post, hidden, emitted)
      assert got[1] <= hdc.LDS_BUDGET
      if emitted >= 64 and got[0] < 64:
        halved.append(((c, pre, post), hidden))
  # (the largest head alone does not halve a pass -- 138 588 bytes at 63 channels x 46 lags --, the largest input under it does)
  assert ((63, 40, 5), [64, 64, 64, 64]) not in halved and ((128, 31, 32), [64, 64, 64, 64]) in halved
  assert device.online_dnn_calib_lds_bytes(128, 31, 32, [64, 64, 64, 64], 130)[0] == 32
  assert hdc.lds_formula(128, 0, 63, [64, 64, 64, 64], 1) <= hdc.LDS_BUDGET
  assert device.online_dnn_calib_lds_bytes(128, 31, 32, [64], 64)[0] >= 1           # K = 8192: the limit itself
  for bad, what in (((0, 0, 0, [4]), 'channels'), ((129, 31, 32, [4]), 'channels'), ((4, -1, 0, [4]), 'lags'),
                    ((4, 0, -1, [4]), 'lags'), ((128, 32, 32, [4]), 'lags'), ((4, 0, 0, [4] * 5), 'hidden layers'),
                    ((4, 0, 0, [0]), 'units'), ((4, 0, 0, [4, 65]), 'units')):
    with pytest.raises(ValueError, match='td_fccalib_online_lds_bytes.*' + what):
      device.online_dnn_calib_lds_bytes(*bad)
  with pytest.raises(ValueError, match='td_fccalib_online_lds_bytes'):
    device.online_dnn_calib_lds_bytes(4, 0, 0, [4], -1)


def test_the_constructor_refuses_by_name(host_only):
  from telluride_decoding_amd import online
  st = hdc.stretch(*SMALL, 60)
  bank = hdc.bank(st, weights=[st['weights']] * 2)
  with pytest.raises(ValueError, match='65536 frames'):
    online.OnlineDNNCalibration(bank, 65537)
  with pytest.raises(ValueError, match='OnlineDNNCalibration calibrates an OnlineDecoder bank, not a object'):
    online.OnlineDNNCalibration(object())
  for kind in ('linear', 'cca'):
    other = online.OnlineDecoder.__new__(online.OnlineDecoder)
    other.kind = kind
    with pytest.raises(ValueError, match='OnlineDNNCalibration calibrates a DNN bank, not a %s bank' % kind):
      online.OnlineDNNCalibration(other)
  # the two other calibrations name this class where they refuse a DNN bank
  other = online.OnlineDecoder.__new__(online.OnlineDecoder)
  other.kind = 'dnn'
  for klass in (online.OnlineCalibration, online.OnlineCCACalibration):
    with pytest.raises(ValueError, match='not a dnn bank .*OnlineDNNCalibration'):
      klass(other)
  assert online.OnlineDNNCalibration(bank, 0).window_size == 1 and online.OnlineDNNCalibration(bank).window_size == 100
  calib = online.OnlineDNNCalibration(bank, 7)
  assert (calib.sessions, calib.channels, calib.pre, calib.post, calib.delay, calib.hidden, calib.frames_emitted,
          calib.windows) == (2, 5, 2, 9, 9, [16], 0, 0)
  z = lambda *shape: np.zeros(shape, np.float32)
  for eeg, att, unatt in ((z(10, 5), z(10), z(10)), (z(2, 10, 4), z(2, 10), z(2, 10)), (z(2, 10, 5), z(2, 9), z(2, 9))):
    with pytest.raises(ValueError, match='A push is'):
      calib.push(eeg, att, unatt)
  assert calib.push(z(2, 9, 5), z(2, 9), z(2, 9)) == 0                   # nine rows, nine behind: nothing counted
  with pytest.raises(ValueError, match='OnlineDNNCalibration.finish: session 0: No data for class'):
    calib.finish()
  with pytest.raises(ValueError, match='OnlineDNNCalibration.flush takes the last rows as eeg AND both envelopes'):
    calib.flush(z(2, 1, 5))
  assert calib.flush() == 9
  for call in (lambda: calib.push(z(2, 1, 5), z(2, 1), z(2, 1)), calib.flush):
    with pytest.raises(ValueError, match='flushed'):
      call()


@pytest.mark.parametrize('width', hoc.WIDTHS)
def test_numpy_session_is_the_twin_and_chunk_invariant(host_only, width):
  """The host session's sums are hoc.twin_sums of _HostDnnSession's own float64 prediction, bit for bit; pushes of 1,
  W - 1, W, W + 1, random 0 .. 40 and whole, an empty push in the middle, flushed by a flushing last push and by an
  empty flushing push: the same arrays; finish gives closed_form of them."""
  from telluride_decoding_amd import online
  (c, pre, post), hidden = SMALL
  frames = 230
  st = hdc.stretch(*SMALL, frames)
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
  pred = st['pred64']
  seen = []
  hoc.run(calib, st['eeg'], st['att'], st['unatt'], [100, 0, 37, 93], after_push=lambda at: seen.append(at))
  whole = calib.sums().copy()
  assert whole.shape == (1, 29) and whole.dtype == np.float64 and seen == [100, 100, 137, 230]
  np.testing.assert_array_equal(whole[0], hoc.twin_sums(pred, st['att'], st['unatt'], width))
  assert whole[0, 0] != 0.0 and (frames % width == 0) == (not whole[0, 24:].any())
  for name, sizes in hoc.cuts(frames, width).items():
    for flush_last in (False, True):
      hoc.run(calib, st['eeg'], st['att'], st['unatt'], sizes, flush_last=flush_last)
      np.testing.assert_array_equal(calib.sums(), whole, err_msg='%s %s' % (name, flush_last))
  # before the flush the last `post` frames are missing: the twin of the first frames - post
  calib.reset()
  assert calib.push(st['eeg'], st['att'], st['unatt']) == frames - post
  m = frames - post
  np.testing.assert_array_equal(calib.sums()[0], hoc.twin_sums(pred[:m], st['att'][:m], st['unatt'][:m], width))
  r = calib.finish()
  want = hoc.closed_form(calib.sums()[0], m, width)
  assert r.corr.shape == (1, 2, 3) and r.lda.shape == (1, 3) and r.dprime.shape == (1,)
  np.testing.assert_array_equal(r.corr[0, 0], r.corr[0, 1])
  got = dict(corr=tuple(r.corr[0, 0]), lda=tuple(r.lda[0]), dprime=r.dprime[0])
  err, err_d = hoc.distances(got, want)
  assert err <= 1e-13 and err_d <= 1e-13 and r.lda[0, 0] == 1.0
  assert calib.flush() == frames                                       # (calibration goes on after a look)
  np.testing.assert_array_equal(calib.sums(), whole)


@pytest.mark.parametrize('frames,width', [(700, 100), (700, 7), (300, 1)])
def test_finish_is_the_two_pass_route(host_only, frames, width):
  """finish on the host session against Decoder.train's two passes in float64 on the same predictions (oracle
  Correlator, average_data, scaled_lda_fit, calculate_dprime) at tests/test_cpu_online_calib.py's own bars: <= 1e-10
  on the statistics and the LDA, <= 1e-9 on d', for stream means of about one standard deviation and at least 6
  windows per class."""
  from telluride_decoding_amd import online
  st = hdc.stretch(*SMALL, frames)
  assert frames // width >= 6
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
  hoc.run(calib, st['eeg'], st['att'], st['unatt'], [frames // 2, frames - frames // 2])
  r = calib.finish()
  got = dict(corr=tuple(r.corr[0, 0]), lda=tuple(r.lda[0]), dprime=r.dprime[0])
  err, err_d = hoc.distances(got, hoc.closed_form(calib.sums()[0], frames, width))
  assert err <= 1e-13 and err_d <= 1e-13
  want = hoc.two_pass(st['pred64'], st['att'], st['unatt'], width)
  err, err_d = hoc.distances(got, want)
  print('N = %d W = %d: corr / lda %.3g, d\' %.3g (d\' = %.4g)' % (frames, width, err, err_d, want['dprime']))
  assert err <= 1e-10
  assert err_d <= 1e-9


def test_finish_refuses_by_name_and_the_session_goes_on(host_only):
  """No completed window, constant predictions (zero power), attended == unattended: each a ValueError naming the
  session and the reason; the sums are untouched and the session still works afterwards."""
  from telluride_decoding_amd import online
  frames, width = 80, 10
  st = hdc.stretch(*SMALL, frames)
  post = st['post']
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
  calib.push(st['eeg'][:18], st['att'][:18], st['unatt'][:18])         # 9 frames counted: no window of 10
  before = calib.sums().copy()
  assert calib.frames_emitted == 18 - post == 9
  with pytest.raises(ValueError, match='session 0: No data for class 0'):
    calib.finish()
  np.testing.assert_array_equal(calib.sums(), before)
  calib.push(st['eeg'][18:], st['att'][18:], st['unatt'][18:])
  calib.flush()
  np.testing.assert_array_equal(calib.sums()[0], hoc.twin_sums(st['pred64'], st['att'], st['unatt'], width))
  assert calib.finish().dprime[0] > 0
  # zero weights: the prediction is the output bias, 0.5, and every sum is exact
  calib = online.OnlineDNNCalibration(hdc.bank(st, weights=hdc.constant_model(st)), width)
  calib.push(st['eeg'], st['att'], st['unatt'])
  assert calib.sums()[0, 0] == 0.5 * (frames - post)
  with pytest.raises(ValueError, match='session 0: the correlation power'):
    calib.finish()
  # the same envelope for both speakers: the class means are equal to the bit
  calib = online.OnlineDNNCalibration(hdc.bank(st, weights=[st['weights']] * 2), width)
  eeg2 = np.stack([st['eeg']] * 2)
  calib.push(eeg2, np.stack([st['att'], st['att']]), np.stack([st['unatt'], st['att']]))
  with pytest.raises(ValueError, match='session 1: X0 and X1 in Scaled LDA are identical'):
    calib.finish()
  dec = hd.dnn_decoder(st['c'], st['pre'], post, st['hidden'], st['weights'], (0, 0, 1))
  with pytest.raises(ValueError, match='session 1: X0 and X1'):
    calib.update_decoder(dec, session=1)
  assert calib.update_decoder(dec) > 0


def test_a_bank_of_three_models_is_its_three_sessions(host_only):
  from telluride_decoding_amd import online
  frames, width = 230, 7
  sts = [hdc.stretch(*SMALL, frames, seed=s, offset=0.5 + 0.5 * s) for s in range(3)]
  bank = hdc.bank(sts[0], weights=[s['weights'] for s in sts])
  calib = online.OnlineDNNCalibration(bank, width)
  stack = lambda key: np.stack([s[key] for s in sts])
  hoc.run(calib, stack('eeg'), stack('att'), stack('unatt'), [130, 1, 0, 99])
  sums, r = calib.sums(), calib.finish()
  assert sums.shape == (3, 29) and r.corr.shape == (3, 2, 3) and r.lda.shape == (3, 3) and r.dprime.shape == (3,)
  for i, s in enumerate(sts):
    single = online.OnlineDNNCalibration(hdc.bank(s), width)
    hoc.run(single, s['eeg'], s['att'], s['unatt'], [frames])
    np.testing.assert_array_equal(sums[i], single.sums()[0])
    np.testing.assert_array_equal(sums[i], hoc.twin_sums(s['pred64'], s['att'], s['unatt'], width))
    one = single.finish()
    np.testing.assert_array_equal(r.corr[i], one.corr[0])
    np.testing.assert_array_equal(r.lda[i], one.lda[0])
    np.testing.assert_array_equal(r.dprime[i], one.dprime[0])
  assert not np.array_equal(sums[0], sums[1])
  calib.reset()
  assert calib.frames_emitted == 0 and not calib.sums().any()


def _windows(dec, st, lo, hi):
  return dec.push(st['eeg'][lo:hi], st['att'][lo:hi], st['unatt'][lo:hi]).scores[0]


@pytest.mark.parametrize('reduction,kind', [('first', 'wta'), ('lda', 'stepped')])
def test_set_statistics_takes_finish_on_the_host_dnn_bank(host_only, reduction, kind):
  """The loop closed on the host: a DNN bank trained with other statistics takes OnlineDNNCalibration.finish's corr
  and lda between pushes; with windows of one frame every score from the swap on is that of a bank built with them,
  and before it the old bank's."""
  from telluride_decoding_amd import online
  frames, cut = 300, 130
  st = hdc.stretch(*SMALL, frames)
  post = st['post']
  old_lda = (1.0, 2.0, -0.5) if reduction == 'lda' else None
  dec = hdc.bank(st, reduction=reduction, lda=old_lda, width=1, hop=1, kind=kind)
  old = hdc.bank(st, reduction=reduction, lda=old_lda, width=1, hop=1, kind=kind)
  calib = online.OnlineDNNCalibration(dec, 20)
  hoc.run(calib, st['eeg'], st['att'], st['unatt'], [frames])
  r = calib.finish()
  new = hdc.bank(st, reduction=reduction, lda=tuple(r.lda[0]) if reduction == 'lda' else None, width=1, hop=1,
                 kind=kind, stats=tuple(r.corr[0, 0]))
  k = cut - post
  head = _windows(dec, st, 0, cut)
  dec.set_statistics(r.corr, r.lda)
  rest = np.concatenate([_windows(dec, st, cut, frames), dec.flush().scores[0]])
  want = np.concatenate([_windows(new, st, 0, cut), _windows(new, st, cut, frames), new.flush().scores[0]])
  np.testing.assert_array_equal(head, _windows(old, st, 0, cut))
  np.testing.assert_array_equal(rest, want[k:])
  assert not np.array_equal(head, want[:k])


def test_update_decoder_round_trips_through_save_parameters(host_only, tmp_path):
  """update_decoder leaves in a LinearRegressionDecoder around the network what save_parameters writes and
  restore_parameters reads back: the correlator's sums and statistics, the one-column LDA with its slope and
  intercept -- and the session parameters of the restored decoder are finish's."""
  from telluride_decoding_amd import online
  frames, width = 300, 20
  st = hdc.stretch(*SMALL, frames)
  calib = online.OnlineDNNCalibration(hdc.bank(st), width)
  hoc.run(calib, st['eeg'], st['att'], st['unatt'], [frames])
  r = calib.finish()
  fresh = lambda: hd.dnn_decoder(st['c'], st['pre'], st['post'], st['hidden'], st['weights'], (0.0, 0.0, 1.0), 'lda',
                                 (1.0, 1.0, 0.0))
  dec = fresh()
  assert calib.update_decoder(dec) == r.dprime[0]
  sums = calib.sums()[0]
  params = dec.correlation_params
  assert params.count == 2 * frames and params.sum_x[0] == sums[4] + sums[2] and params.sum_y2[0] == 2 * sums[1]
  path = str(tmp_path / 'decoder_model.json')
  dec.save_parameters(path)
  back = fresh()
  back.restore_parameters(path)
  p = online.session_parameters(back)
  assert p['kind'] == 'dnn'
  np.testing.assert_array_equal(p['corr'], r.corr[0])
  np.testing.assert_array_equal(p['lda'], r.lda[0])
  with pytest.raises(ValueError, match='session 1 of 1'):
    calib.update_decoder(dec, session=1)
  with pytest.raises(ValueError, match='LinearRegressionDecoder'):
    calib.update_decoder(object())
