"""The online calibration without a GPU: the ctypes prototypes of td_calib_online_* against the header, the state size,
every refusal by name, the closed form on the frame-order twin's sums against the two-pass float64 route of
Decoder.train, online.OnlineCalibration's NumPy session -- against the twin bit for bit, cut into pushes every way and
flushed both ways, refusing by name and going on, as a bank, into a LinearRegressionDecoder -- and
OnlineDecoder.set_statistics on the host bank."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online
from tests import host_online_calib as hoc
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_calib_online_finish', 'td_calib_online_push', 'td_calib_online_state_bytes',
                'td_calib_online_sums']


@pytest.fixture
def host_only(monkeypatch):
  """OnlineCalibration's (and OnlineDecoder's) NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def _bank(st, sessions=1, reduction='first', lda=None, width=20, hop=10, kind='wta', stats=(0.1, 0.2, 0.9)):
  from telluride_decoding_amd import online
  decs = [host_online.linear_decoder(st['c'], st['pre'], st['post'], st['w'], st['b'], stats, reduction, lda)
          for _ in range(sessions)]
  return online.OnlineDecoder(decs, width, hop, decoder_type=kind)


def test_argtypes_match_the_header_prototypes():
  """td_calib_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py); the family stays out of the closed td_online_* set; the
  header's limits and statuses are the module's."""
  from telluride_decoding_amd import _lib, device, online
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_calib_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert not re.fullmatch(r'td_(online|cca_online|fc_online|audio_online|fit_online)_\w+', name)
    assert name in _lib.header_symbols()
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
  for macro, value in (('TD_CALIB_ONLINE_MAX_CHANNELS', device.ONLINE_CALIB_MAX_CHANNELS),
                       ('TD_CALIB_ONLINE_MAX_LAGS', device.ONLINE_CALIB_MAX_LAGS),
                       ('TD_CALIB_ONLINE_SUMS', device.ONLINE_CALIB_SUMS), ('TD_CALIB_OK', device.CALIB_OK),
                       ('TD_CALIB_NO_WINDOW', device.CALIB_NO_WINDOW), ('TD_CALIB_NO_POWER', device.CALIB_NO_POWER),
                       ('TD_CALIB_SAME_MEANS', device.CALIB_SAME_MEANS), ('TD_ONLINE_MAX_WIDTH', online.MAX_WINDOW),
                       ('TD_ONLINE_MAX_PUSH', online.MAX_FIT_PUSH)):
    found = re.search(r'#define\s+%s\s+(\d+)' % macro, raw)
    assert found and int(found.group(1)) == value, macro
  assert (device.ONLINE_CALIB_MAX_CHANNELS, device.ONLINE_CALIB_MAX_LAGS, device.ONLINE_CALIB_SUMS,
          online.CALIB_SUMS, hoc.SUMS) == (128, 64, 29, 29, 29)


def test_state_bytes_hold_what_a_session_carries():
  """29 float64 sums, the EEG tail and the envelope tail in float32; a multiple of 8; the limits by name."""
  from telluride_decoding_amd import device
  for c, pre, post in ((3, 0, 0), (1, 0, 0), (5, 2, 9), (64, 0, 20), (128, 31, 32), (7, 0, 1), (1, 63, 0)):
    need = 8 * 29 + 4 * c * (pre + post) + 4 * 2 * post
    nbytes = device.online_calib_state_bytes(c, pre, post)
    assert nbytes % 8 == 0 and need <= nbytes < need + 8, (c, pre, post, nbytes)
  for bad in ((0, 0, 0), (129, 0, 0), (4, -1, 0), (4, 0, -1), (4, 32, 32), (4, 0, 64)):
    with pytest.raises(ValueError, match='td_calib_online_state_bytes'):
      device.online_calib_state_bytes(*bad)


def test_every_refusal_is_raised_by_name(host_only):
  from telluride_decoding_amd import online
  st = hoc.stretch(4, 1, 2, 60)
  bank = _bank(st, sessions=2)
  for window, match in ((65537, '65536 frames'),):
    with pytest.raises(ValueError, match=match):
      online.OnlineCalibration(bank, window)
  with pytest.raises(ValueError, match='an OnlineDecoder bank'):
    online.OnlineCalibration(object())
  for kind in ('cca', 'dnn'):
    other = online.OnlineDecoder.__new__(online.OnlineDecoder)
    other.kind = kind
    with pytest.raises(ValueError, match='a linear bank, not a %s bank' % kind):
      online.OnlineCalibration(other)
  assert online.OnlineCalibration(bank, 0).window_size == 1 == online.OnlineCalibration(bank, -3).window_size
  assert online.OnlineCalibration(bank).window_size == 100
  calib = online.OnlineCalibration(bank, 7)
  assert (calib.sessions, calib.channels, calib.pre, calib.post, calib.delay, calib.frames_emitted) == (2, 4, 1, 2, 2, 0)
  z = lambda *shape: np.zeros(shape, np.float32)
  for eeg, att, unatt in ((z(10, 4), z(10), z(10)),                      # two sessions need [S, n, c]
                          (z(2, 10, 5), z(2, 10), z(2, 10)), (z(2, 10, 4), z(2, 9), z(2, 9)),
                          (z(3, 10, 4), z(3, 10), z(3, 10))):
    with pytest.raises(ValueError, match='A push is'):
      calib.push(eeg, att, unatt)
  assert calib.push(z(2, 2, 4), z(2, 2), z(2, 2)) == 0                   # two rows, two behind: nothing counted
  with pytest.raises(ValueError, match='session 0: No data for class'):
    calib.finish()
  with pytest.raises(ValueError, match='eeg AND both envelopes'):
    calib.flush(z(2, 1, 4))
  assert calib.flush() == 2
  for call in (lambda: calib.push(z(2, 1, 4), z(2, 1), z(2, 1)), calib.flush):
    with pytest.raises(ValueError, match='flushed'):
      call()
  one = online.OnlineCalibration(_bank(hoc.stretch(1, 0, 0, 60)), 1)
  with pytest.raises(ValueError, match='1048576 rows'):
    one.push(z(1048577, 1), z(1048577), z(1048577))


@pytest.mark.parametrize('frames,width', [(3000, 100), (3000, 1), (600, 100), (700, 7)])
@pytest.mark.parametrize('offset', [0.0, 1.0, 3.3])
def test_the_closed_form_is_the_two_pass_route(frames, width, offset):
  """closed_form(twin_sums) against Decoder.train's two passes in float64 (oracle Correlator, average_data,
  scaled_lda_fit, calculate_dprime): <= 1e-10 relative on {mean_x, mean_y, power, lda_w, slope, intercept} and <= 1e-9
  on d' -- the <= 4.3e-13 of the issue's NumPy restatement plus margin for other seeds -- for means up to 3.3
  standard deviations and at least 6 windows per class."""
  st = hoc.stretch(5, 2, 9, frames, offset=offset)
  pred = hoc.host_pred(st['eeg'], st['w'], st['b'], 2, 9).astype(np.float32)
  assert frames // width >= 6
  got = hoc.closed_form(hoc.twin_sums(pred, st['att'], st['unatt'], width), frames, width)
  want = hoc.two_pass(pred, st['att'], st['unatt'], width)
  err, err_d = hoc.distances(got, want)
  print('N = %d W = %d mean = %g std: corr / lda %.3g, d\' %.3g (d\' = %.4g)' %
        (frames, width, offset, err, err_d, want['dprime']))
  assert err <= 1e-10
  assert err_d <= 1e-9


def test_the_cancellation_grows_with_the_squared_mean():
  """The documented case: at means of 33 standard deviations the closed form's differences cancel (mean / std)^2 =
  100 times more than at 3.3.  Its own bars: 100 x the bars above on the statistics and the LDA (1e-8), and for d',
  whose variances sum_w m^2 / n - mbar^2 cancel a second time, 1e-6 -- the issue's reference restatement is off by
  3.6e-9 there, and the bar keeps the margin the other bars keep over their 4.3e-13.  The error is larger than at
  mean 0: that is the growth DESIGN section 35 describes; a centring shift is out of scope."""
  frames, width = 3000, 100
  errs = {}
  for offset in (0.0, 33.0):
    st = hoc.stretch(5, 2, 9, frames, offset=offset)
    pred = hoc.host_pred(st['eeg'], st['w'], st['b'], 2, 9).astype(np.float32)
    got = hoc.closed_form(hoc.twin_sums(pred, st['att'], st['unatt'], width), frames, width)
    errs[offset] = hoc.distances(got, hoc.two_pass(pred, st['att'], st['unatt'], width))
    print('mean = %g std: corr / lda %.3g, d\' %.3g' % ((offset,) + errs[offset]))
  assert errs[33.0][0] <= 1e-8
  assert errs[33.0][1] <= 1e-6
  assert errs[33.0][1] > errs[0.0][1]


@pytest.mark.parametrize('width', hoc.WIDTHS)
def test_numpy_session_is_the_twin_and_chunk_invariant(host_only, width):
  """The host session's sums are twin_sums of its own float64 prediction, bit for bit; pushes of 1, W - 1, W, W + 1,
  random 0 .. 40 and whole, an empty push in the middle, flushed by a flushing last push and by an empty flushing
  push: the same arrays; finish gives closed_form of them."""
  from telluride_decoding_amd import online
  c, pre, post, frames = 5, 2, 9, 230
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  calib = online.OnlineCalibration(_bank(st), width)
  pred = hoc.host_pred(st['eeg'], st['w'], st['b'], pre, post)
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


def test_finish_refuses_by_name_and_the_session_goes_on(host_only):
  """No completed window, constant predictions (zero power), attended == unattended: each a ValueError naming the
  session and the reason; the sums are untouched and the session still works afterwards."""
  from telluride_decoding_amd import online
  c, pre, post, frames, width = 4, 1, 2, 80, 10
  st = hoc.stretch(c, pre, post, frames)
  calib = online.OnlineCalibration(_bank(st), width)
  calib.push(st['eeg'][:11], st['att'][:11], st['unatt'][:11])         # 9 frames counted: no window of 10
  before = calib.sums().copy()
  with pytest.raises(ValueError, match='session 0: No data for class 0'):
    calib.finish()
  np.testing.assert_array_equal(calib.sums(), before)
  calib.push(st['eeg'][11:], st['att'][11:], st['unatt'][11:])
  calib.flush()
  pred = hoc.host_pred(st['eeg'], st['w'], st['b'], pre, post)
  np.testing.assert_array_equal(calib.sums()[0], hoc.twin_sums(pred, st['att'], st['unatt'], width))
  assert calib.finish().dprime[0] > 0
  # zero weights: the prediction is the bias, 0.5, and every sum is exact
  flat = dict(st, w=np.zeros_like(st['w']), b=np.float32(0.5))
  calib = online.OnlineCalibration(_bank(flat), width)
  calib.push(st['eeg'], st['att'], st['unatt'])
  with pytest.raises(ValueError, match='session 0: the correlation power'):
    calib.finish()
  # the same envelope for both speakers: the class means are equal to the bit
  calib = online.OnlineCalibration(_bank(st, sessions=2), width)
  eeg2 = np.stack([st['eeg']] * 2)
  calib.push(eeg2, np.stack([st['att'], st['att']]), np.stack([st['unatt'], st['att']]))
  with pytest.raises(ValueError, match='session 1: X0 and X1 in Scaled LDA are identical'):
    calib.finish()
  with pytest.raises(ValueError, match='session 1: X0 and X1'):
    calib.update_decoder(host_online.linear_decoder(c, pre, post, st['w'], st['b'], (0, 0, 1)), session=1)
  assert calib.update_decoder(host_online.linear_decoder(c, pre, post, st['w'], st['b'], (0, 0, 1))) > 0


def test_a_bank_is_its_sessions_and_follows_set_weights(host_only):
  from telluride_decoding_amd import online
  c, pre, post, frames, width = 5, 2, 9, 230, 7
  sts = [hoc.stretch(c, pre, post, frames, seed=s, offset=0.5 * s) for s in range(3)]
  bank = _bank(sts[0], sessions=3)
  bank.set_weights(np.stack([s['w'] for s in sts]), np.array([s['b'] for s in sts]))
  calib = online.OnlineCalibration(bank, width)
  stack = lambda key: np.stack([s[key] for s in sts])
  hoc.run(calib, stack('eeg'), stack('att'), stack('unatt'), [130, 1, 0, 99])
  sums, r = calib.sums(), calib.finish()
  assert sums.shape == (3, 29) and r.corr.shape == (3, 2, 3) and r.lda.shape == (3, 3) and r.dprime.shape == (3,)
  for i, s in enumerate(sts):
    single = online.OnlineCalibration(_bank(s), width)
    hoc.run(single, s['eeg'], s['att'], s['unatt'], [frames])
    np.testing.assert_array_equal(sums[i], single.sums()[0])
    one = single.finish()
    np.testing.assert_array_equal(r.corr[i], one.corr[0])
    np.testing.assert_array_equal(r.lda[i], one.lda[0])
    np.testing.assert_array_equal(r.dprime[i], one.dprime[0])
  assert not np.array_equal(sums[0], sums[1])
  calib.reset()
  assert calib.frames_emitted == 0 and not calib.sums().any()


def _windows(dec, st, lo, hi):
  r = dec.push(st['eeg'][lo:hi], st['att'][lo:hi], st['unatt'][lo:hi])
  return r.scores[0], r.decisions[0]


@pytest.mark.parametrize('reduction,kind', [('first', 'wta'), ('lda', 'stepped')])
def test_set_statistics_on_the_host_bank(host_only, reduction, kind):
  """After set_statistics the frames a push emits are scored with the new parameters: with windows of one frame every
  score from the swap on is that of a bank built with them (and before it the old bank's); the forms corr and lda
  take; the shapes and the CCA bank refused."""
  from telluride_decoding_amd import online
  c, pre, post, frames = 4, 2, 3, 300
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  old_lda, new_lda = (1.0, 2.0, -0.5), (1.0, 3.5, 0.25)
  new_stats = (0.9, 1.1, 0.4)
  lda = lambda v: v if reduction == 'lda' else None
  dec = _bank(st, reduction=reduction, lda=lda(old_lda), width=1, hop=1, kind=kind)
  old = _bank(st, reduction=reduction, lda=lda(old_lda), width=1, hop=1, kind=kind)
  new = _bank(st, reduction=reduction, lda=lda(new_lda), width=1, hop=1, kind=kind, stats=new_stats)
  cut = 130
  k = cut - post
  head = _windows(dec, st, 0, cut)[0]
  dec.set_statistics(np.array(new_stats), np.array(new_lda))           # (an lda a bank does not reduce with is not read)
  rest = np.concatenate([_windows(dec, st, cut, frames)[0], dec.flush().scores[0]])
  want = np.concatenate([_windows(new, st, 0, cut)[0], _windows(new, st, cut, frames)[0], new.flush().scores[0]])
  np.testing.assert_array_equal(head, _windows(old, st, 0, cut)[0])
  np.testing.assert_array_equal(rest, want[k:])
  assert not np.array_equal(head, want[:k])
  # the forms: [S, 3] and [S, 2, 3] for corr, [S, 3] for lda
  bank = _bank(st, sessions=2, reduction=reduction, lda=lda(old_lda), width=1, hop=1, kind=kind)
  corr = np.array([[0.1, 0.2, 0.9], new_stats])
  bank.set_statistics(corr, np.array([old_lda, new_lda]))
  eeg2 = np.stack([st['eeg'][:cut]] * 2)
  env = [np.stack([st[key][:cut]] * 2) for key in ('att', 'unatt')]
  got = bank.push(eeg2, env[0], env[1]).scores
  np.testing.assert_array_equal(got[0], head)
  np.testing.assert_array_equal(got[1], want[:k])
  bank.reset()
  bank.set_statistics(np.stack([corr, corr], axis=1)[::-1], np.array([new_lda, old_lda]))
  got = bank.push(eeg2, env[0], env[1]).scores
  np.testing.assert_array_equal(got[0], want[:k])
  np.testing.assert_array_equal(got[1], head)
  for bad in (np.zeros(2), np.zeros((3, 3)), np.zeros((2, 2)), np.zeros((2, 3, 3)), np.zeros((2, 2, 3, 1))):
    with pytest.raises(ValueError, match=r'set_statistics takes corr \[3\]'):
      bank.set_statistics(bad, np.array(new_lda))
  for bad in (np.zeros(2), np.zeros((3, 3)), np.zeros((2, 2, 3))):
    with pytest.raises(ValueError, match=r'set_statistics takes lda \[3\]'):
      bank.set_statistics(np.array(new_stats), bad)
  if reduction == 'lda':
    with pytest.raises(ValueError, match='needs lda'):
      bank.set_statistics(np.array(new_stats))
  else:
    bank.set_statistics(np.array(new_stats))
  cca = online.OnlineDecoder.__new__(online.OnlineDecoder)
  cca.kind = 'cca'
  with pytest.raises(ValueError, match='not of a cca bank'):
    cca.set_statistics(np.zeros(3))
  assert 'OnlineCalibration' in online.OnlineDecoder.set_weights.__doc__


def test_update_decoder_round_trips_through_save_parameters(host_only, tmp_path):
  """update_decoder leaves in a LinearRegressionDecoder what save_parameters writes and restore_parameters reads
  back: the correlator's sums and statistics, the one-column LDA with its slope and intercept -- and an OnlineDecoder
  built around the restored decoder scores with finish's parameters."""
  from telluride_decoding_amd import infer_decoder, online
  c, pre, post, frames, width = 4, 2, 3, 300, 20
  st = hoc.stretch(c, pre, post, frames, offset=1.0)
  calib = online.OnlineCalibration(_bank(st), width)
  hoc.run(calib, st['eeg'], st['att'], st['unatt'], [frames])
  r = calib.finish()
  dec = host_online.linear_decoder(c, pre, post, st['w'], st['b'], (0.0, 0.0, 1.0), 'lda')
  dprime = calib.update_decoder(dec)
  assert dprime == r.dprime[0]
  sums = calib.sums()[0]
  params = dec.correlation_params
  assert params.count == 2 * frames and params.sum_x[0] == sums[4] + sums[2] and params.sum_y2[0] == 2 * sums[1]
  path = str(tmp_path / 'decoder_model.json')
  dec.save_parameters(path)
  back = host_online.linear_decoder(c, pre, post, st['w'], st['b'], (0.0, 0.0, 1.0), 'lda')
  back.restore_parameters(path)
  p = online.session_parameters(back)
  np.testing.assert_array_equal(p['corr'], r.corr[0])
  np.testing.assert_array_equal(p['lda'], r.lda[0])
  assert np.asarray(back.lda_params.mean_vectors).shape == (2, 1) and list(back.lda_params.labels) == [1, 2]
  with pytest.raises(ValueError, match='session 1 of 1'):
    calib.update_decoder(dec, session=1)
  with pytest.raises(ValueError, match='LinearRegressionDecoder'):
    calib.update_decoder(object())
  del infer_decoder
