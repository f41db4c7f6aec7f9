"""The device side of the raw-recording readers: td_raw_decode (both routes, both sample kinds, both arithmetics),
td_columns_assemble, and BrainVision / EDF files end to end through BrainExperiment.

Every comparison is bitwise (NaN inputs: the NaN positions) against NumPy on the same bytes: the readers of
tests/host_raw.py, the expressions `float32(x) * float32(scale)` and `scale * (offset + float64(x))` written out
here, and for the assemble the strided-copy loop ingest keeps for NumPy inputs."""
import ctypes
import os

import numpy as np
import pytest

from telluride_decoding_amd import _lib
from telluride_decoding_amd import ingest
from telluride_decoding_amd import ingest_brainvision
from telluride_decoding_amd import ingest_edf
from tests import host_raw as hr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
CHANNELS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 200)
FRAMES = (1, 2, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
GUARD32, GUARD64 = 12345.0, -54321.0


@pytest.fixture(scope='module')
def torch():
  import torch as t
  return t


@pytest.fixture(scope='module')
def device():
  from telluride_decoding_amd import device as module
  assert module.gpu_available()
  return module


def upload(torch, device, blob, guard=64):
  """(image of len(blob) bytes, the whole buffer): the file's bytes followed by `guard` bytes of 0xa5, which as
  samples would be large numbers."""
  h = device.default_handle()
  whole = torch.from_numpy(np.frombuffer(bytes(blob) + b'\xa5' * guard, np.uint8).copy()).to(h.device)
  return whole[:len(blob)], whole


def guarded(torch, device, rows, cols, f64):
  """(the [rows, cols] view the kernel fills, the whole matrix): one guard row above and below, one guard column
  before and two after, so the row stride exceeds cols and the view starts off the allocation's alignment."""
  h = device.default_handle()
  whole = torch.full((rows + 2, cols + 3), GUARD64 if f64 else GUARD32, dtype=torch.float64 if f64 else torch.float32,
                     device=h.device)
  return whole[1:1 + rows, 1:1 + cols], whole


def guards_intact(whole, rows, cols):
  host = whole.cpu().numpy().copy()
  value = host[0, 0]
  host[1:1 + rows, 1:1 + cols] = value
  return bool((host == value).all())


def numpy_decode(blob, data_offset, records, record_bytes, n, w, offsets, scales, adds):
  """The oracle for any layout: one strided gather per signal, then the NumPy expression."""
  body = np.frombuffer(blob, np.uint8, count=records * record_bytes, offset=data_offset).reshape(records, record_bytes)
  out = []
  for s, off in enumerate(offsets):
    raw = np.ascontiguousarray(body[:, off:off + n * w]).view('<i2' if w == 2 else '<f4').reshape(-1)
    with np.errstate(all='ignore'):
      if adds is None:
        out.append(raw.astype(np.float32) * np.float32(scales[s]))
      else:
        out.append(np.float64(scales[s]) * (np.float64(adds[s]) + raw.astype(np.float64)))
  return np.stack(out)


def decode_and_check(torch, device, blob, data_offset, records, record_bytes, n, w, offsets, scales, adds, route):
  assert device.raw_route(n, w, record_bytes)[0] == route
  image, whole_image = upload(torch, device, blob)
  out, whole = guarded(torch, device, len(offsets), records * n, adds is not None)
  kind = device.RAW_INT16 if w == 2 else device.RAW_FLOAT32
  got = device.raw_decode(image, data_offset, records, record_bytes, n, kind, offsets, scales, adds, out=out)
  want = numpy_decode(blob, data_offset, records, record_bytes, n, w, offsets, scales, adds)
  assert hr.same_bits(got.cpu().numpy(), want), (records, record_bytes, n, w, len(offsets))
  assert guards_intact(whole, len(offsets), records * n)


# ---------------------------------------------------------------- the transposing route
@pytest.mark.parametrize('channels', CHANNELS)
def test_multiplexed_float32(torch, device, channels):
  rng = np.random.default_rng(channels)
  factors = hr.resolutions(channels)
  for frames in FRAMES:
    samples = hr.float_patterns(rng, frames * channels).reshape(frames, channels)
    decode_and_check(torch, device, samples.astype('<u4').tobytes(), 0, frames, 4 * channels, 1, 4,
                     [4 * c for c in range(channels)], factors, None, route=True)


@pytest.mark.parametrize('channels,frames', list(zip(CHANNELS, FRAMES)))
def test_multiplexed_int16(torch, device, channels, frames):
  rng = np.random.default_rng(1000 + channels)
  samples = hr.int16_patterns(rng, frames * channels).reshape(frames, channels)
  decode_and_check(torch, device, samples.astype('<i2').tobytes(), 0, frames, 2 * channels, 1, 2,
                   [2 * c for c in range(channels)], hr.resolutions(channels), None, route=True)


def test_subnormal_products_are_kept(torch, device):
  values = np.array([[1e-38, -3e-38, 2e-37, 1.1754944e-38], [5e-39, 1e-30, -1e-38, 7e-45]], np.float32)
  scales = [0.0488281, 0.3, 0.01, 0.5]
  want = numpy_decode(values.tobytes(), 0, 2, 16, 1, 4, [0, 4, 8, 12], scales, None)
  tiny = (want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)
  assert tiny.sum() >= 6                                       # (the case is what it says)
  decode_and_check(torch, device, values.tobytes(), 0, 2, 16, 1, 4, [0, 4, 8, 12], scales, None, route=True)


def layout_with_a_gap(n, w, signals, gap_bytes):
  """`signals` signals of n samples around one skipped block of gap_bytes in the middle: (offsets, record bytes)."""
  offsets, at = [], 0
  for s in range(signals + 1):
    if s == (signals + 1) // 2:
      at += gap_bytes
    else:
      offsets.append(at)
      at += n * w
  return offsets, at


def ranges(signals):
  """EDF-style (bitvalue, offset) pairs that are not exact in binary."""
  scale = [(3276.7 + 0.25 * s + 3276.8) / 65535.0 for s in range(signals)]
  return scale, [(3276.7 + 0.25 * s) / scale[s] - 32767.0 for s in range(signals)]


def test_route_threshold(torch, device):
  """Both sides of td_raw_route's own threshold, with more than one sample per record on the transposing side."""
  for w in (2, 4):
    threshold = next(n for n in range(1, 200) if not device.raw_route(n, w, 3 * n * w)[0])
    assert threshold > 2
    rng = np.random.default_rng(w)
    for n in (2, threshold - 1, threshold):
      offsets, record_bytes = layout_with_a_gap(n, w, 2, n * w)
      for records in (1, 17, 300):
        blob = b'head' * 5 + (hr.int16_patterns(rng, records * record_bytes // 2).tobytes() if w == 2 else
                              hr.float_patterns(rng, records * record_bytes // 4).tobytes())
        scale, add = ranges(2)
        decode_and_check(torch, device, blob, 20, records, record_bytes, n, w, offsets, scale, None,
                         route=n < threshold)
        decode_and_check(torch, device, blob, 20, records, record_bytes, n, w, offsets, scale, add,
                         route=n < threshold)


# ---------------------------------------------------------------- the direct route
@pytest.mark.parametrize('n', [1, 2, 7, 63, 64, 65, 256, 1000])
def test_direct_route(torch, device, n):
  rng = np.random.default_rng(n)
  for w in (2, 4):
    for signals in (1, 3, 33):
      # (a skipped signal large enough that short runs do not fit the transposing route's staging area)
      offsets, record_bytes = layout_with_a_gap(n, w, signals, 3076 if n * w < 64 else 2 * w)
      scale, add = ranges(signals)
      for records in (1, 2, 3, 17):
        count = records * record_bytes // w
        blob = b'\x11' * 256 + (hr.int16_patterns(rng, count) if w == 2 else hr.float_patterns(rng, count)).tobytes()
        decode_and_check(torch, device, blob, 256, records, record_bytes, n, w, offsets, scale, None, route=False)
        decode_and_check(torch, device, blob, 256, records, record_bytes, n, w, offsets, scale, add, route=False)


# ---------------------------------------------------------------- argument checks
def raw_call(device, image_ptr, image_bytes, data_offset, records, record_bytes, n, kind, offsets, scales, adds, arith,
             out_ptr, ld_out, num=None):
  h = device.default_handle()
  keep_off, off_p = _lib.i64_array(offsets)
  keep_scale, scale_p = _lib.f64_array(scales)
  keep_add, add_p = _lib.f64_array(adds)
  return h.lib.td_raw_decode(h.ptr, ctypes.c_void_p(image_ptr), image_bytes, data_offset, records, record_bytes, n, kind,
                             len(offsets) if num is None else num, off_p, scale_p, add_p, arith, ctypes.c_void_p(out_ptr),
                             ld_out)


def test_argument_checks(torch, device):
  h = device.default_handle()
  image, _ = upload(torch, device, bytes(range(256)) * 2)          # 8 records of 64 bytes
  out = torch.full((4, 8), GUARD32, dtype=torch.float32, device=h.device)
  ip, op = image.data_ptr(), out.data_ptr()
  good = dict(image_ptr=ip, image_bytes=512, data_offset=0, records=8, record_bytes=64, n=1, kind=1,
              offsets=[0, 4, 8, 60], scales=[1.5] * 4, adds=[0.0] * 4, arith=0, out_ptr=op, ld_out=8)
  bad = {
      'a NULL image': dict(image_ptr=0),
      'a NULL output': dict(out_ptr=0),
      'an image off 16 bytes': dict(image_ptr=ip + 4, image_bytes=508, records=7),
      'records past the image': dict(records=9, ld_out=9),
      'a data offset that pushes the records past the image': dict(data_offset=4),
      'a signal past its record': dict(offsets=[0, 4, 8, 64]),
      'a signal of n samples past its record': dict(n=2, records=4, offsets=[0, 8, 16, 60]),
      'a signal off the sample size': dict(offsets=[0, 4, 8, 58]),
      'a row stride below the samples': dict(ld_out=7),
      'arith 0 with an offset': dict(adds=[0.0, 0.0, 1.0, 0.0]),
      'too many signals': dict(offsets=[0] * 1025, scales=[1.0] * 1025, adds=[0.0] * 1025),
      'no signals': dict(num=0),
      'an unknown sample kind': dict(kind=2),
  }
  for what, change in bad.items():
    assert raw_call(device, **dict(good, **change)) == _lib.TD_ERR_INVALID, what
    assert h.lib.td_last_error(h.ptr).decode().startswith('td_raw_decode'), what
  assert raw_call(device, **dict(good, records=0)) == _lib.TD_OK
  assert bool((out == GUARD32).all())
  assert raw_call(device, **good) == _lib.TD_OK
  with np.errstate(all='ignore'):
    want = np.frombuffer(bytes(range(256)) * 2, '<f4').reshape(8, 16)[:, [0, 1, 2, 15]].T * np.float32(1.5)
  assert hr.same_bits(out.cpu().numpy(), want)
  with pytest.raises(ValueError):
    device.raw_decode(image, 0, 8, 64, 1, device.RAW_FLOAT32, [0, 4, 8, 64], [1.0] * 4)
  with pytest.raises(ValueError):
    device.raw_decode(image, 0, 8, 64, 1, device.RAW_FLOAT32, [0], [1.0], out=out[:, :7])


# ---------------------------------------------------------------- columns_assemble
def loop_result(sources, frames):
  return ingest._assemble_columns_loop(sources, frames, sum(int(s.shape[1]) for s in sources)).cpu().numpy()


@pytest.mark.parametrize('count', [1, 2, 15, 16, 33, 64, 65, 129, 256])
def test_columns_of_one_matrix(torch, device, count):
  """Width-1 sources, float32 and float64 mixed, rows of one matrix sliced as fix_offset slices them (3 elements
  in: not 16-byte aligned), both sides of td_columns_route's threshold."""
  h = device.default_handle()
  assert device.columns_route(count, 1) == (count >= 16)
  rng = np.random.default_rng(count)
  for frames in (1, 63, 64, 65, 257, 1000):
    bits = hr.float_patterns(rng, count * (frames + 3)).reshape(count, frames + 3)
    m32 = torch.from_numpy(bits.view(np.float32)).to(h.device)
    wide = rng.standard_normal((count, frames + 3)) * 10.0 ** rng.integers(-48, 42, size=(count, frames + 3))
    wide[:, -1] = -1e-60                                        # (beyond float32's range at both ends)
    wide[:, 3] = 1e300
    m64 = torch.from_numpy(wide).to(h.device)
    sources = [(m64 if k % 3 == 1 else m32)[k, 3:].reshape(-1, 1) for k in range(count)]
    got = device.columns_assemble(sources, frames)
    assert got.shape == (frames, count) and got.dtype == torch.float32
    want = loop_result(sources, frames)
    assert hr.same_bits(got.cpu().numpy(), want)
    if count > 1:
      assert np.isinf(want[0, 1]) and (frames == 1 or (want[-1, 1] == 0 and np.signbit(want[-1, 1])))


def test_columns_of_mixed_widths(torch, device):
  h = device.default_handle()
  rng = np.random.default_rng(5)
  frames = 130
  a = torch.from_numpy(rng.standard_normal((frames + 2, 3)).astype(np.float32)).to(h.device)
  b = torch.from_numpy(rng.standard_normal((frames, 1)) * 1e39).to(h.device)
  c = torch.from_numpy(rng.standard_normal((frames + 5, 8)).astype(np.float32)).to(h.device)[:, 2:7]   # row stride 8
  sources = [a, b, c] + [a[:, 1:2]] * 20
  assert not device.columns_route(len(sources), 5)
  out, whole = guarded(torch, device, frames, 29, False)
  got = device.columns_assemble(sources, frames, out=out)
  assert hr.same_bits(got.cpu().numpy(), loop_result(sources, frames)) and guards_intact(whole, frames, 29)
  assert np.isinf(got.cpu().numpy()[:, 3]).any()
  # the transposing route into a guarded matrix
  sources = [c[:, k % 5:k % 5 + 1] for k in range(70)]
  out, whole = guarded(torch, device, frames, 70, False)
  got = device.columns_assemble(sources, frames, out=out)
  assert hr.same_bits(got.cpu().numpy(), loop_result(sources, frames)) and guards_intact(whole, frames, 70)
  with pytest.raises(ValueError):
    device.columns_assemble(sources, frames + 6)
  with pytest.raises(ValueError):
    device.columns_assemble([])


# ---------------------------------------------------------------- end to end
def experiment_eeg(directory, data_file, names):
  sound = {'audio_data': np.zeros((1000, 1), np.float32), 'audio_sr': 16000}
  experiment = ingest.BrainExperiment({'trial': [sound, data_file]}, directory, directory)
  experiment.load_all_data()
  trial = experiment.trial_data('trial')
  trial.assemble_brain_data(list(names))
  with np.errstate(all='ignore'):
    times = trial.find_eeg_trigger_times()[0]
  return trial.model_features['eeg'], times, experiment.summary()


def both_routes(monkeypatch, device, directory, make, names):
  on_device, times_device, summary_device = experiment_eeg(directory, make(), names)
  assert ingest._is_device_tensor(on_device)
  with monkeypatch.context() as m:
    m.setattr(ingest_brainvision.device, 'gpu_available', lambda: False)
    m.setattr(ingest_edf.device, 'gpu_available', lambda: False)
    on_host, times_host, summary_host = experiment_eeg(directory, make(), names)
  assert isinstance(on_host, np.ndarray) and on_host.dtype == np.float32
  assert hr.same_bits(on_device.cpu().numpy(), on_host)
  assert np.array_equal(times_device, times_host) and summary_device == summary_host
  return on_host


def test_the_reference_recording_end_to_end(monkeypatch, device):
  make = lambda: ingest_brainvision.BvBrainDataFile('brainvision_test.vhdr')
  bv = make()
  bv.load_all_data(GOLDEN)
  values = bv.signal_values('TRIG')
  assert ingest._is_device_tensor(values) and values.dim() == 1 and values.is_contiguous()
  assert bv.signal_values('CH1') is None
  g20 = np.load(os.path.join(GOLDEN, 'g20_brainvision.npz'))
  for i, name in enumerate(bv.signal_names):
    assert hr.same_bits(bv.signal_values(name).cpu().numpy(), g20['values_%02d' % i]), name
  eeg = both_routes(monkeypatch, device, GOLDEN, make, bv.signal_names)
  assert eeg.shape == (5, 65)


@pytest.mark.parametrize('binary_format,orientation', [('IEEE_FLOAT_32', 'MULTIPLEXED'), ('INT_16', 'MULTIPLEXED'),
                                                       ('IEEE_FLOAT_32', 'VECTORIZED'), ('INT_16', 'VECTORIZED')])
def test_synthetic_brainvision_end_to_end(monkeypatch, device, tmp_path, binary_format, orientation):
  path, samples, factors = hr.synth_brainvision(str(tmp_path), 'rec', 65, 1000, binary_format, orientation, seed=9)
  names, _, want = hr.read_brainvision_numpy(path)
  eeg = both_routes(monkeypatch, device, str(tmp_path), lambda: ingest_brainvision.BvBrainDataFile('rec'), names)
  assert hr.same_bits(eeg, np.ascontiguousarray(want.T))


@pytest.mark.parametrize('records,n', [(4, 250), (1000, 1)])
def test_synthetic_edf_end_to_end(monkeypatch, device, tmp_path, records, n):
  path, _ = hr.synth_edf(str(tmp_path / 'rec.edf'), 65, records, n, seed=3, annotations_at=40)
  labels, _, want = hr.read_edf_numpy(path)
  parsed = ingest_edf.parse_edf_file(path)
  assert ingest._is_device_tensor(parsed['signals']) and hr.same_bits(parsed['signals'].cpu().numpy(), want)
  eeg = both_routes(monkeypatch, device, str(tmp_path), lambda: ingest_edf.EdfBrainDataFile('rec'), labels)
  assert hr.same_bits(eeg, np.ascontiguousarray(want.T.astype(np.float32)))
