"""The online CCA calibration without a GPU: the ctypes prototypes of td_ccacalib_online_* against the header, the
state size T(D) = 9 D^2 + 20 D, the closed form on the frame-order twin's sums against the two-pass float64 route of
Decoder.train with a CCADecoder, online.OnlineCCACalibration's NumPy session -- against the twin bit for bit, cut into
pushes every way and flushed both ways, refusing by name and going on, as a bank, into a CCADecoder through a
save / restore round trip -- and OnlineDecoder.set_cca_statistics on the host bank."""
import ctypes
import re

import numpy as np
import pytest

from tests import host_online_cca_calib as hcal
from tests.test_cpu_dnn import _kind_of_ctype

ENTRY_POINTS = ['td_ccacalib_online_finish', 'td_ccacalib_online_lds_bytes', 'td_ccacalib_online_push',
                'td_ccacalib_online_state_bytes', 'td_ccacalib_online_sums']
SMALL = [((5, 2, 9), (3, 1, 4), 2), ((3, 1, 2), (2, 0, 6), 3)]


@pytest.fixture
def host_only(monkeypatch):
  """OnlineCCACalibration's (and OnlineDecoder's) NumPy session, whatever the machine has."""
  from telluride_decoding_amd import device
  monkeypatch.setattr(device, 'gpu_available', lambda: False)


def _bank(st, sessions=1, reduction='first', lda=None, width=20, hop=10, kind='wta'):
  from telluride_decoding_amd import online
  decs = [hcal.decoder_of(st, reduction, lda) for _ in range(sessions)]
  return online.OnlineDecoder(decs, width, hop, decoder_type=kind)


def test_argtypes_match_the_header_prototypes():
  """td_ccacalib_online_*: as many argtypes as the prototypes of include/td_hotpath.h have parameters, each of the
  parameter's kind (the method of tests/test_cpu_online.py); the family stays out of the closed td_*_online_* sets;
  the new status is the module's."""
  from telluride_decoding_amd import _lib, device
  with open(_lib.HEADER) as f:
    raw = f.read()
  text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
  protos = dict(re.findall(r'\bint\s+(td_ccacalib_online_\w+)\s*\(([^)]*)\)\s*;', text))
  assert sorted(protos) == ENTRY_POINTS
  lib = _lib.load()
  for name in ENTRY_POINTS:
    assert not re.fullmatch(r'td_(online|cca_online|fc_online|audio_online|fit_online|ccafit_online|calib_online)_\w+',
                            name)
    assert name in _lib.header_symbols()
    kinds = []
    for param in protos[name].split(','):
      words = param.replace('*', ' * ').split()
      assert len(words) >= 2 and words[-1].isidentifier(), param
      kinds.append('pointer' if '*' in words else ' '.join(w for w in words[:-1] if w != 'const'))
    assert set(kinds) <= {'pointer', 'int64_t', 'int', 'float', 'double'}, kinds
    assert [_kind_of_ctype(t) for t in _lib.SIGNATURES[name]] == kinds, name
    assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
  found = re.search(r'#define\s+TD_CALIB_NOT_POSITIVE\s+(\d+)', raw)
  assert found and int(found.group(1)) == device.CALIB_NOT_POSITIVE == 4
  assert len({device.CALIB_OK, device.CALIB_NO_WINDOW, device.CALIB_NO_POWER, device.CALIB_SAME_MEANS,
              device.CALIB_NOT_POSITIVE}) == 5


def test_state_bytes_hold_what_a_session_carries():
  """T(D) = 9 D^2 + 20 D float64 sums (29 at D = 1, the linear calibrator's count; 2624 at D = 16), the EEG tail and
  the two feature tails in float32; a multiple of 8; the limits by name; the LDS of a launch within the budget."""
  from telluride_decoding_amd import device, online
  assert [device.online_ccacalib_sums_count(d) for d in (1, 2, 16)] == [29, 76, 2624]
  assert device.online_ccacalib_sums_count(1) == device.ONLINE_CALIB_SUMS
  for d in (1, 2, 3, 5, 16):
    per_class, class0, open0, total = online.cca_calibration_layout(d)
    assert total == 9 * d * d + 20 * d == hcal.sums_count(d) == open0 + 5 * d
    assert class0 == 6 * d and per_class == 3 * d + 3 * d * (3 * d + 1) // 2
  for (c1, pre1, post1), (c2, pre2, post2), d in (((3, 0, 0), (2, 0, 0), 1), ((5, 2, 9), (3, 1, 4), 2),
                                                  ((3, 1, 2), (2, 0, 6), 3), ((64, 0, 20), (8, 0, 15), 5),
                                                  ((5, 0, 0), (16, 0, 0), 16), ((128, 3, 12), (32, 0, 0), 8)):
    post = max(post1, post2)
    need = 8 * (9 * d * d + 20 * d) + 4 * c1 * (pre1 + post) + 4 * 2 * c2 * (pre2 + post)
    nbytes = device.online_ccacalib_state_bytes(c1, pre1, post1, c2, pre2, post2, d)
    assert nbytes % 8 == 0 and need <= nbytes < need + 8, (c1, c2, d, nbytes)
    for emitted in (1, 10, 64, 1000):
      step, lds = device.online_ccacalib_lds_bytes(c1, pre1, post1, c2, pre2, post2, d, emitted)
      assert 1 <= step <= min(64, emitted) and lds <= device.CCA_ONLINE_LDS_BYTES
  # the pass is halved where the whole of it does not fit, and a shape that does not fit at a pass of one is refused
  assert device.online_ccacalib_lds_bytes(128, 3, 12, 32, 0, 0, 16, 64)[0] < 64
  for bad in ((0, 0, 0, 1, 0, 0, 1), (129, 0, 0, 1, 0, 0, 1), (4, -1, 0, 1, 0, 0, 1), (4, 0, 64, 1, 0, 0, 1),
              (4, 0, 0, 33, 0, 0, 1), (4, 0, 0, 2, 40, 40, 1), (4, 0, 0, 2, 0, 0, 0), (4, 0, 0, 2, 0, 0, 17),
              (128, 0, 63, 32, 0, 63, 16)):
    with pytest.raises(ValueError, match='td_ccacalib_online_state_bytes'):
      device.online_ccacalib_state_bytes(*bad)
  with pytest.raises(ValueError, match='td_ccacalib_online_lds_bytes.*bytes of LDS'):
    device.online_ccacalib_lds_bytes(128, 0, 63, 32, 0, 63, 16)


def _frames_for(dims, width):
  return width * max(2 * dims, 30) if width > 1 else 300


@pytest.mark.parametrize('width', hcal.WIDTHS)
@pytest.mark.parametrize('dims', [1, 2, 3, 5, 16])
def test_the_closed_form_is_the_two_pass_route(dims, width):
  """closed_form(twin_sums) -- the helper's and the library's host evaluation -- against Decoder.train's two passes in
  float64 on the same float32 projections: <= 1e-10 on the statistics, on slope w (relative to its largest entry) and
  on the intercept, <= 1e-9 on d'.  slope w, never w: the reference's eigenvector sign is arbitrary.  Every case has
  at least 2 dims windows per class."""
  from telluride_decoding_amd import device, online
  frames = _frames_for(dims, width)
  assert frames // width >= 2 * dims
  a, b1, b0 = hcal.projections(dims, frames)
  sums = hcal.twin_sums(a, b1, b0, width)
  assert sums.shape == (hcal.sums_count(dims),)
  want = hcal.two_pass(a, b1, b0, width)
  got = hcal.closed_form(sums, frames, width, dims)
  err, err_d = hcal.distances(got, want)
  o = online.cca_calibration_closed_form(sums, frames, width, dims)
  assert o['status'] == device.CALIB_OK and o['count'] == 2 * frames
  lib = dict(corr=np.stack([o['mean_a'], o['mean_b'], o['power']]), axis=o['slope'] * o['w'],
             intercept=o['intercept'], dprime=o['dprime'])
  lib_err, lib_err_d = hcal.distances(lib, want)
  print('D = %d W = %d: closed form %.3g, d\' %.3g; library %.3g, d\' %.3g' % (dims, width, err, err_d, lib_err,
                                                                             lib_err_d))
  if dims == 1:
    assert o['w'].tolist() == [1.0]
  else:
    assert abs(np.linalg.norm(o['w']) - 1.0) < 1e-14
  assert max(err, lib_err) <= 1e-10
  assert max(err_d, lib_err_d) <= 1e-9
  # the walk the host session uses is the twin, bit for bit
  mine = np.zeros_like(sums)
  online.cca_calibration_walk(mine, a[:frames // 2], b1[:frames // 2], b0[:frames // 2], 0, width)
  online.cca_calibration_walk(mine, a[frames // 2:], b1[frames // 2:], b0[frames // 2:], frames // 2, width)
  assert np.array_equal(mine, sums)


@pytest.mark.parametrize('width', [1, 7])
@pytest.mark.parametrize('shape', SMALL, ids=['d2', 'd3'])
def test_the_host_session_is_the_twin_under_every_cut(host_only, shape, width):
  """sums() after every push of every cut equals twin_sums of the host projections up to the frames counted, by array
  equality: ones, W - 1, W, W + 1, random 0 .. 40, whole, an empty push in the middle; a flushing last push and an
  empty flushing push."""
  from telluride_decoding_amd import online
  view1, view2, dims = shape
  frames = 300
  st = hcal.stretch(view1, view2, dims, frames)
  calib = online.OnlineCCACalibration(_bank(st), width)
  assert calib.delay == max(view1[2], view2[2]) and calib.window_size == width
  whole = hcal.twin_sums(st['a'], st['b1'], st['b0'], width)

  def check(at):
    m = max(0, at - calib.delay)
    assert np.array_equal(calib.sums()[0], hcal.twin_sums(st['a'][:m], st['b1'][:m], st['b0'][:m], width)), at

  for name, sizes in hcal.cuts(frames, width).items():
    for flush_last in (False, True):
      after = check if name in ('random', 'empty-middle') and not flush_last else None
      assert hcal.run(calib, st['eeg'], st['att'], st['unatt'], sizes, flush_last=flush_last,
                      after_push=after) == frames
      assert np.array_equal(calib.sums()[0], whole), (name, flush_last)
      assert calib.windows == frames // width
      with pytest.raises(ValueError, match='flushed'):
        calib.push(st['eeg'][:1], st['att'][:1], st['unatt'][:1])
  # finish on the host is the closed form, and it matches the two-pass route on the host projections
  r = calib.finish()
  assert r.corr.shape == (1, 2, 3, dims) and r.lda.shape == (1, dims + 2) and r.dprime.shape == (1,)
  assert np.array_equal(r.corr[0, 0], r.corr[0, 1])
  err, err_d = hcal.distances(hcal.result_of(r.corr[0], r.lda[0], r.dprime[0]),
                              hcal.two_pass(st['a'], st['b1'], st['b0'], width))
  assert err <= 1e-10 and err_d <= 1e-9


def test_each_status_is_raised_by_name_and_the_session_goes_on(host_only):
  from telluride_decoding_amd import device, online
  view1, view2, dims = SMALL[1]
  st = hcal.stretch(view1, view2, dims, 300)
  delay = max(view1[2], view2[2])
  calib = online.OnlineCCACalibration(_bank(st), 10)
  eeg, att, unatt = st['eeg'], st['att'], st['unatt']
  calib.push(eeg[:delay + 9], att[:delay + 9], unatt[:delay + 9])              # 9 frames: no window of 10
  with pytest.raises(ValueError, match='session 0: No data for class 0'):
    calib.finish()
  calib.push(eeg[delay + 9:delay + 20], att[delay + 9:delay + 20], unatt[delay + 9:delay + 20])
  assert calib.windows == 2                                                      # 4 windows in all < dims + 2
  before = calib.sums().copy()
  with pytest.raises(ValueError, match='session 0: the pooled scatter .* not positive definite'):
    calib.finish()
  dec = hcal.decoder_of(st)
  with pytest.raises(ValueError, match='not positive definite'):
    calib.update_decoder(dec)
  assert np.array_equal(calib.sums(), before)
  calib.push(eeg[delay + 20:], att[delay + 20:], unatt[delay + 20:])
  calib.flush()
  assert float(calib.finish().dprime[0]) > 0
  # attended == unattended: the class means are equal; a zero rotation: every EEG projection is 0.0, no power
  calib.reset()
  calib.push(eeg, att, att)
  with pytest.raises(ValueError, match='session 0: X0 and X1 in Scaled LDA are identical'):
    calib.finish()
  calib.reset()
  calib.decoder.set_cca_model(st['mean_x'], np.zeros_like(st['rot_x']), st['mean_y'], st['rot_y'])
  calib.push(eeg, att, unatt)
  with pytest.raises(ValueError, match='session 0: the correlation power of a dim'):
    calib.finish()
  o = online.cca_calibration_closed_form(calib.sums()[0], calib.frames_emitted, 10, dims)
  assert o['status'] == device.CALIB_NO_POWER and np.isnan(o['dprime']) and np.isnan(o['power']).all()
  # the constructor's and the pushes' refusals
  for window, match in ((65537, '65536 frames'),):
    with pytest.raises(ValueError, match=match):
      online.OnlineCCACalibration(_bank(st), window)
  with pytest.raises(ValueError, match='an OnlineDecoder bank'):
    online.OnlineCCACalibration(object())
  from tests import host_online
  from tests import host_online_calib as hoc
  lin = hoc.stretch(4, 1, 2, 20)
  linear = online.OnlineDecoder(host_online.linear_decoder(4, 1, 2, lin['w'], lin['b'], (0.1, 0.2, 0.9), 'first', None),
                                20, 10)
  with pytest.raises(ValueError, match='calibrates a CCA bank, not a linear bank'):
    online.OnlineCCACalibration(linear)
  with pytest.raises(ValueError, match='not of a linear bank'):
    linear.set_cca_statistics(np.zeros((3, 1)))
  calib.reset()
  with pytest.raises(ValueError, match='A push is eeg'):
    calib.push(eeg[:5], att[:4], unatt[:5])
  with pytest.raises(ValueError, match='eeg AND both feature blocks'):
    calib.flush(eeg[:5])
  with pytest.raises(ValueError, match='takes a CCADecoder'):
    calib.update_decoder(object())
  with pytest.raises(ValueError, match='session 3 of 1'):
    calib.update_decoder(dec, 3)


def test_a_bank_is_its_sessions(host_only):
  """Three sessions with their own rows and their own models in one bank against three single sessions."""
  from telluride_decoding_amd import online
  view1, view2, dims = SMALL[0]
  frames, width = 200, 7
  sts = [hcal.stretch(view1, view2, dims, frames, seed=s) for s in range(3)]
  bank = online.OnlineDecoder([hcal.decoder_of(s) for s in sts], 20, 10)
  calib = online.OnlineCCACalibration(bank, width)
  stack = lambda key: np.stack([s[key] for s in sts])
  hcal.run(calib, stack('eeg'), stack('att'), stack('unatt'), [90, 0, 1, 109])
  r = calib.finish()
  for i, s in enumerate(sts):
    single = online.OnlineCCACalibration(online.OnlineDecoder(hcal.decoder_of(s), 20, 10), width)
    hcal.run(single, s['eeg'], s['att'], s['unatt'], [frames])
    assert np.array_equal(calib.sums()[i], single.sums()[0])
    assert np.array_equal(calib.sums()[i], hcal.twin_sums(s['a'], s['b1'], s['b0'], width))
    one = single.finish()
    for got, want in zip(r, one):
      assert np.array_equal(got[i], want[0])
  assert not np.array_equal(calib.sums()[0], calib.sums()[1])


def test_the_calibrator_follows_set_cca_model(host_only):
  from telluride_decoding_amd import online
  view1, view2, dims = SMALL[0]
  frames, width, cut = 200, 7, 90
  st = hcal.stretch(view1, view2, dims, frames)
  other = hcal.stretch(view1, view2, dims, frames, seed=1)
  bank = _bank(st)
  calib = online.OnlineCCACalibration(bank, width)
  calib.push(st['eeg'][:cut], st['att'][:cut], st['unatt'][:cut])
  bank.set_cca_model(other['mean_x'], other['rot_x'], other['mean_y'], other['rot_y'])
  calib.flush(st['eeg'][cut:], st['att'][cut:], st['unatt'][cut:])
  k = cut - calib.delay
  proj = lambda rows, m, view, mean, rot: hcal.host_proj(rows, view[0], view[1], view[2], m[mean], m[rot])
  a = np.concatenate([st['a'][:k], proj(st['eeg'], other, view1, 'mean_x', 'rot_x')[k:]])
  b1 = np.concatenate([st['b1'][:k], proj(st['att'], other, view2, 'mean_y', 'rot_y')[k:]])
  b0 = np.concatenate([st['b0'][:k], proj(st['unatt'], other, view2, 'mean_y', 'rot_y')[k:]])
  assert np.array_equal(calib.sums()[0], hcal.twin_sums(a, b1, b0, width))
  assert not np.array_equal(a, st['a'])


@pytest.mark.parametrize('reduction', ['first', 'mean', 'lda'])
def test_set_cca_statistics_on_the_host_bank(host_only, reduction):
  """Every shape of corr and lda, every refusal; after the swap the bank scores the frames the next push emits as a
  fresh bank built with the new parameters does, from the first window wholly behind the swap."""
  from telluride_decoding_amd import online
  view1, view2, dims = SMALL[0]
  frames, width, hop, cut = 300, 20, 10, 130
  st = hcal.stretch(view1, view2, dims, frames)
  calib = online.OnlineCCACalibration(_bank(st), 20)
  hcal.run(calib, st['eeg'], st['att'], st['unatt'], [frames])
  r = calib.finish()
  old_lda = np.array([1.0] * dims + [2.0, -0.5]) if reduction == 'lda' else None
  bank = _bank(st, sessions=2, reduction=reduction, lda=old_lda, width=width, hop=hop)
  s = 2
  with pytest.raises(ValueError, match=r'takes corr \[3, 2\], \[2, 3, 2\] or \[2, 2, 3, 2\], not \(3,\)'):
    bank.set_cca_statistics(np.zeros(3), r.lda[0])
  with pytest.raises(ValueError, match=r'takes lda \[4\] or \[2, 4\], not \(3,\)'):
    bank.set_cca_statistics(r.corr[0, 0], np.zeros(3))
  if reduction == 'lda':
    with pytest.raises(ValueError, match='needs lda'):
      bank.set_cca_statistics(r.corr[0, 0])
  for corr in (r.corr[0, 0], np.stack([r.corr[0, 0]] * s), np.stack([r.corr[0]] * s)):
    for lda in (r.lda[0], np.stack([r.lda[0]] * s)):
      bank.set_cca_statistics(np.zeros_like(corr) + 1.0, np.zeros_like(lda))
      bank.set_cca_statistics(corr, lda if reduction == 'lda' else None)
      for p in bank._params:
        assert np.array_equal(p['corr'], r.corr[0])
        if reduction == 'lda':
          assert np.array_equal(p['lda'], r.lda[0])
  # a running bank: old parameters up to the cut, the new ones behind it
  running = _bank(st, reduction=reduction, lda=old_lda, width=width, hop=hop)
  trained = hcal.decoder_of(st, reduction, r.lda[0] if reduction == 'lda' else None, stats=r.corr[0, 0])
  fresh = online.OnlineDecoder(trained, width, hop)
  push = lambda bank, lo, hi: bank.push(st['eeg'][lo:hi], st['att'][lo:hi], st['unatt'][lo:hi])
  head = push(running, 0, cut)
  rot = running._params[0]['rot_x'].copy()
  running.set_cca_statistics(r.corr, r.lda if reduction == 'lda' else None)
  assert np.array_equal(running._params[0]['rot_x'], rot)
  got = np.concatenate([head.scores[0], push(running, cut, frames).scores[0], running.flush().scores[0]])
  want = np.concatenate([push(fresh, 0, cut).scores[0], push(fresh, cut, frames).scores[0], fresh.flush().scores[0]])
  first = -(-(cut - running.delay) // hop)
  assert got.shape == want.shape and 0 < first < got.shape[0] - 5
  assert got[first:].tobytes() == want[first:].tobytes()
  assert got[:first].tobytes() != want[:first].tobytes()


def test_update_decoder_through_a_save_and_restore_round_trip(host_only, tmp_path):
  """update_decoder leaves the correlator's sums and statistics and the scaled LDA in a CCADecoder; save_parameters
  and restore_parameters carry them into another, and an OnlineDecoder built from that one holds finish's values."""
  from telluride_decoding_amd import online
  view1, view2, dims = SMALL[1]
  frames, width = 300, 7
  st = hcal.stretch(view1, view2, dims, frames)
  calib = online.OnlineCCACalibration(_bank(st), width)
  hcal.run(calib, st['eeg'], st['att'], st['unatt'], [frames])
  r = calib.finish()
  dec = hcal.decoder_of(st, 'lda', np.ones(dims + 2))
  dprime = calib.update_decoder(dec)
  assert dprime == float(r.dprime[0])
  cp = dec.correlation_params
  assert cp.count == 2 * frames and np.array_equal(cp.mean_x, r.corr[0, 0, 0]) and np.array_equal(cp.power,
                                                                                                   r.corr[0, 0, 2])
  assert np.allclose(cp.sum_x, 2.0 * st['a'].sum(axis=0), rtol=1e-12)
  assert np.allclose(cp.sum_y, st['b0'].sum(axis=0) + st['b1'].sum(axis=0), rtol=1e-12)
  path = str(tmp_path / 'decoder_model.json')
  dec.save_parameters(path)
  other = hcal.decoder_of(st, 'lda', np.ones(dims + 2))
  other.restore_parameters(path)
  p = online.cca_session_parameters(other)
  assert np.array_equal(p['corr'][0], r.corr[0, 0]) and np.array_equal(p['corr'][1], r.corr[0, 1])
  assert np.array_equal(p['lda'], r.lda[0])
  # the restored decoder maps a correlation row as finish's LDA does
  row = np.arange(1.0, dims + 1.0).reshape(1, -1)
  assert np.allclose(other._lda.transform(row)[0, 0], r.lda[0, -2] * (row[0] @ r.lda[0, :-2]) + r.lda[0, -1],
                     rtol=1e-13)
