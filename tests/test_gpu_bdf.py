"""The device side of the BioSemi BDF reader: td_raw24_decode at the C-ABI level (every alignment of a run's first
and last byte, an image that ends off a dword, a guarded output), its argument checks, device.code_onsets against
its NumPy contract at the chunk edges, and a BDF file end to end through BrainExperiment.

Every comparison is bitwise against NumPy on the same bytes (tests/host_bdf.py and the expressions written out
here); the events are compared as equal arrays."""
import ctypes

import numpy as np
import pytest

from telluride_decoding_amd import _lib
from telluride_decoding_amd import ingest
from telluride_decoding_amd import ingest_bdf
from tests import host_bdf as hb
from tests import host_raw as hr

pytestmark = pytest.mark.gpu

DATA_OFFSETS = (0, 1, 2, 3, 768)
SAMPLES = (1, 2, 3, 5, 21, 22, 64, 85, 86, 256, 257, 1000)
RECORDS = (1, 2, 3, 17)
GUARD = -54321.0


@pytest.fixture(scope='module')
def torch():
  import torch as t
  return t


@pytest.fixture(scope='module')
def device():
  from telluride_decoding_amd import device as module
  assert module.gpu_available()
  return module


# ---------------------------------------------------------------- td_raw24_decode
def layouts(n):
  """The layouts decoded for n samples per record: every data offset once, the record counts and 1 .. 5 listed
  signals in turn, one unlisted signal in the middle whose size (1 .. 8 bytes) makes the image end off a dword."""
  at = SAMPLES.index(n)
  out = []
  for k, data_offset in enumerate(DATA_OFFSETS):
    records = RECORDS[(k + at) % len(RECORDS)]
    listed = 1 + (k + at) % 5
    for gap in range(1, 9):
      offsets, pos = [], 0
      for s in range(listed + 1):
        if s == (listed + 1) // 2:
          pos += gap
        else:
          offsets.append(pos)
          pos += 3 * n
      if (data_offset + records * pos) % 4:
        break
    out.append(dict(data_offset=data_offset, records=records, record_bytes=pos, n=n, offsets=offsets))
  return out


def test_the_layouts_cover_every_alignment():
  """From the offsets themselves: a run's first byte and its last byte fall on every residue mod 4, every listed
  value of the issue is used, and every image ends off a dword."""
  first, last, seen = set(), set(), {'offset': set(), 'records': set(), 'listed': set()}
  for n in SAMPLES:
    for L in layouts(n):
      assert (L['data_offset'] + L['records'] * L['record_bytes']) % 4 != 0
      seen['offset'].add(L['data_offset']), seen['records'].add(L['records']), seen['listed'].add(len(L['offsets']))
      for r in range(L['records']):
        for off in L['offsets']:
          b = L['data_offset'] + r * L['record_bytes'] + off
          first.add(b % 4), last.add((b + 3 * n - 1) % 4)
  assert first == last == {0, 1, 2, 3}
  assert seen == {'offset': set(DATA_OFFSETS), 'records': set(RECORDS), 'listed': {1, 2, 3, 4, 5}}


def ranges(signals):
  """BDF-style (bitvalue, offset) pairs that are not exact in binary: both roundings matter."""
  scale = [(262143.0 + 5 * s + 262144.0 + 3 * s) / 16777215.0 for s in range(signals)]
  return scale, [(262143.0 + 5 * s) / scale[s] - 8388607.0 for s in range(signals)]


def numpy_decode24(blob, data_offset, records, record_bytes, n, offsets, scales, adds):
  body = np.frombuffer(blob, np.uint8, count=records * record_bytes, offset=data_offset).reshape(records, record_bytes)
  out = []
  for s, off in enumerate(offsets):
    b = body[:, off:off + 3 * n].reshape(-1, 3).astype(np.int64)
    unsigned = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    digital = np.where(unsigned & 0x800000, unsigned - (1 << 24), unsigned).astype(np.float64)
    out.append(np.float64(scales[s]) * (np.float64(adds[s]) + digital))
  return np.stack(out)


def upload(torch, device, blob, guard=64):
  """(image of len(blob) bytes, the whole buffer): the bytes followed by `guard` bytes of 0xa5."""
  h = device.default_handle()
  whole = torch.from_numpy(np.frombuffer(bytes(blob) + b'\xa5' * guard, np.uint8).copy()).to(h.device)
  return whole[:len(blob)], whole


def guarded(torch, device, rows, cols):
  """(the [rows, cols] view the kernel fills, the whole matrix): one guard row above and below, one guard column
  before and two after: the row stride exceeds cols, and rows start on and off 16 bytes."""
  h = device.default_handle()
  whole = torch.full((rows + 2, cols + 3), GUARD, dtype=torch.float64, device=h.device)
  return whole[1:1 + rows, 1:1 + cols], whole


def guards_intact(whole, rows, cols):
  host = whole.cpu().numpy().copy()
  host[1:1 + rows, 1:1 + cols] = GUARD
  return bool((host == GUARD).all())


def raw24_call(device, image_ptr, image_bytes, data_offset, records, record_bytes, n, offsets, scales, adds, out_ptr,
               ld_out, num=None):
  h = device.default_handle()
  keep_off, off_p = _lib.i64_array(offsets)
  keep_scale, scale_p = _lib.f64_array(scales)
  keep_add, add_p = _lib.f64_array(adds)
  return h.lib.td_raw24_decode(h.ptr, ctypes.c_void_p(image_ptr), image_bytes, data_offset, records, record_bytes, n,
                               len(offsets) if num is None else num, off_p, scale_p, add_p, ctypes.c_void_p(out_ptr),
                               ld_out)


@pytest.mark.parametrize('n', SAMPLES)
def test_raw24_decode(torch, device, n):
  rng = np.random.default_rng(n)
  for L in layouts(n):
    size = L['data_offset'] + L['records'] * L['record_bytes']
    blob = rng.integers(0, 256, size=size, dtype=np.uint8)
    # the first listed signal starts with 0x7fffff, 0x800000, 0xffffff where it has the room
    edge = hb.pack24(hb.EDGES_24[:min(n, 8)]).reshape(-1)
    start = L['data_offset'] + L['offsets'][0]
    blob[start:start + edge.size] = edge
    blob = blob.tobytes()
    listed, cols = len(L['offsets']), L['records'] * n
    scale, add = ranges(listed)
    image, whole_image = upload(torch, device, blob)
    assert image.data_ptr() % 16 == 0 and image.numel() == size and size % 4 != 0
    out, whole = guarded(torch, device, listed, cols)
    assert whole.stride(0) > cols
    rc = raw24_call(device, image.data_ptr(), size, L['data_offset'], L['records'], L['record_bytes'], n, L['offsets'],
                    scale, add, out.data_ptr(), whole.stride(0))
    assert rc == _lib.TD_OK, L
    want = numpy_decode24(blob, L['data_offset'], L['records'], L['record_bytes'], n, L['offsets'], scale, add)
    assert hr.same_bits(out.cpu().numpy(), want), L
    assert guards_intact(whole, listed, cols), L
    # the same through device.raw24_decode, into a matrix of its own
    got = device.raw24_decode(image, L['data_offset'], L['records'], L['record_bytes'], n, L['offsets'], scale, add)
    assert got.shape == (listed, cols) and hr.same_bits(got.cpu().numpy(), want), L


def test_raw24_argument_checks(torch, device):
  h = device.default_handle()
  blob = bytes(range(256)) * 2 + b'\x07'                             # 8 records of 64 bytes from byte 1
  image, _ = upload(torch, device, blob)
  out = torch.full((4, 16), GUARD, dtype=torch.float64, device=h.device)
  ip, op = image.data_ptr(), out.data_ptr()
  good = dict(image_ptr=ip, image_bytes=513, data_offset=1, records=8, record_bytes=64, n=2, offsets=[0, 6, 13, 58],
              scales=[1.5] * 4, adds=[0.25] * 4, out_ptr=op, ld_out=16)
  bad = {
      'a NULL image': dict(image_ptr=0),
      'a NULL output': dict(out_ptr=0),
      'an image off 16 bytes': dict(image_ptr=ip + 4, image_bytes=509, records=7),
      'an output off 8 bytes': dict(out_ptr=op + 4),
      'records past the image': dict(records=9, ld_out=18),
      'a data offset that pushes the records past the image': dict(data_offset=2),
      'a negative data offset': dict(data_offset=-1),
      'a signal past its record': dict(offsets=[0, 6, 13, 59]),
      'a signal before its record': dict(offsets=[-1, 6, 13, 58]),
      'a record smaller than a signal': dict(n=22, records=1, ld_out=22, offsets=[0, 0, 0, 0]),
      'no samples': dict(n=0),
      'a row stride below the samples': dict(ld_out=15),
      'too many signals': dict(offsets=[0] * 1025, scales=[1.0] * 1025, adds=[0.0] * 1025),
      'no signals': dict(num=0),
  }
  for what, change in bad.items():
    assert raw24_call(device, **dict(good, **change)) == _lib.TD_ERR_INVALID, what
    assert h.lib.td_last_error(h.ptr).decode().startswith('td_raw24_decode:'), what
  assert raw24_call(device, **dict(good, records=0)) == _lib.TD_OK
  assert bool((out == GUARD).all())
  assert raw24_call(device, **good) == _lib.TD_OK
  want = numpy_decode24(blob, 1, 8, 64, 2, [0, 6, 13, 58], [1.5] * 4, [0.25] * 4)
  assert hr.same_bits(out.cpu().numpy(), want)
  with pytest.raises(ValueError, match='td_raw24_decode'):
    device.raw24_decode(image, 1, 8, 64, 2, [0, 6, 13, 59], [1.0] * 4, [0.0] * 4)
  with pytest.raises(ValueError, match='raw24_decode'):
    device.raw24_decode(image, 1, 8, 64, 2, [0], [1.0], [0.0], out=out[:, :15])
  with pytest.raises(ValueError, match='raw24_decode'):
    device.raw24_decode(image, 1, 8, 64, 2, [0, 6], [1.0], [0.0, 0.0])


# ---------------------------------------------------------------- code_onsets
MASKS = (0xffff, 0xff, 0x1)


def onset_patterns(n, chunk):
  """{name: (float64 [n], the number of events under mask 0xffff, or None)}."""
  firsts = np.arange(0, n, chunk)
  lasts = np.minimum(firsts + chunk - 1, n - 1)
  edges = np.zeros(n)
  edges[lasts] = 0x101 + 2 * np.arange(lasts.size)                   # (odd, and not 0 under any of the masks)
  edges[firsts] = 0x203 + 2 * np.arange(firsts.size)
  span = np.zeros(n)
  for f in firsts:                                                   # one code from two samples before an edge to one after
    span[max(f - 2, 0):f + 2] = 0x305
  rng = np.random.default_rng(n)
  codes = np.repeat(rng.integers(-(1 << 23), 1 << 23, size=n // 3 + 1), 3)[:n].astype(np.float64)
  codes[rng.random(n) < 0.2] = 0.0
  negative = codes + 0.75 * np.sign(codes)                           # (truncation toward zero gives the codes back)
  negative[::7] = -np.abs(negative[::7])
  return {'none': (np.zeros(n), 0),
          'every': (1.0 + (np.arange(n) % 2), n),
          'edges': (edges, len(set(firsts) | set(lasts))),
          'span': (span, firsts.size),
          'negative': (negative, None)}


def test_code_onsets(torch, device):
  h = device.default_handle()
  chunk = device.code_onsets_plan(1)[0]
  for n in (1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 1):
    assert device.code_onsets_plan(n) == (chunk, -(-n // chunk))
    for name, (values, count) in onset_patterns(n, chunk).items():
      on_device = torch.from_numpy(values).to(h.device)
      for mask in MASKS:
        at, codes = device.code_onsets(on_device, mask)
        want_at, want_codes = hb.code_onsets_numpy(values, mask)
        assert at.dtype == np.int64 and codes.dtype == np.int32, (n, name, mask)
        assert np.array_equal(at, want_at) and np.array_equal(codes, want_codes), (n, name, mask)
      if count is not None:
        assert len(hb.code_onsets_numpy(values, 0xffff)[0]) == count, (n, name)      # (the pattern is what it says)
      if name == 'span' and n > chunk:
        assert not set(hb.code_onsets_numpy(values, 0xffff)[0]) & set(range(chunk, n, chunk))
      if name == 'negative' and n >= 63:
        assert (values < 0).any() and (values != np.trunc(values)).any()


def test_code_onsets_of_a_sliced_column(torch, device):
  """A column of a [frames, 3] matrix sliced 3 rows in, as fix_offset leaves a channel: a stride of 3 elements from
  a pointer that is 8-byte but not 16-byte aligned."""
  h = device.default_handle()
  chunk = device.code_onsets_plan(1)[0]
  frames = 2 * chunk + 5
  rng = np.random.default_rng(3)
  matrix = np.repeat(rng.integers(0, 1 << 16, size=(frames // 2 + 2, 3)), 2, axis=0)[:frames + 3].astype(np.float64)
  on_device = torch.from_numpy(matrix).to(h.device)
  column = on_device[3:, 2]
  assert column.stride(0) == 3 and column.data_ptr() % 16 == 8 and column.shape[0] == frames
  for view in (column, column.reshape(-1, 1)):
    at, codes = device.code_onsets(view, 0xff)
    want_at, want_codes = hb.code_onsets_numpy(matrix[3:, 2], 0xff)
    assert len(want_at) > frames // 4 and np.array_equal(at, want_at) and np.array_equal(codes, want_codes)
  with pytest.raises(ValueError):
    device.code_onsets(column, 0)
  with pytest.raises(ValueError):
    device.code_onsets(column, 0x1000000)
  with pytest.raises(ValueError):
    device.code_onsets(column.to(torch.float32))
  at, codes = device.code_onsets(on_device[:0, 0])
  assert at.shape == (0,) and codes.shape == (0,) and at.dtype == np.int64 and codes.dtype == np.int32


# ---------------------------------------------------------------- end to end
def experiment(directory, names):
  sound = {'audio_data': np.zeros((1000, 1), np.float32), 'audio_sr': 16000}
  exp = ingest.BrainExperiment({'trial': [sound, ingest_bdf.BdfBrainDataFile('trial')]}, directory, directory)
  exp.load_all_data()
  trial = exp.trial_data('trial')
  trial.assemble_brain_data(list(names))
  return trial, exp.summary()


def test_bdf_end_to_end(monkeypatch, device, tmp_path):
  path, _ = hb.synth_bdf(str(tmp_path / 'trial.bdf'), 17, 4, 256, seed=7, annotations_at=9)
  labels, _, want = hb.read_bdf_numpy(path)
  names = labels[:-1]
  trial, summary = experiment(str(tmp_path), names)
  eeg = trial.model_features['eeg']
  status = trial.brain_data['Status'].signal
  assert ingest._is_device_tensor(eeg) and ingest._is_device_tensor(status)
  times, codes = trial.find_status_trigger_times()
  low_times, low_codes = trial.find_status_trigger_times(mask=0xff)
  with monkeypatch.context() as m:
    m.setattr(ingest_bdf.device, 'gpu_available', lambda: False)
    host_trial, host_summary = experiment(str(tmp_path), names)
  host_eeg = host_trial.model_features['eeg']
  assert isinstance(host_eeg, np.ndarray) and isinstance(host_trial.brain_data['Status'].signal, np.ndarray)
  assert hr.same_bits(eeg.cpu().numpy(), host_eeg) and summary == host_summary
  assert hr.same_bits(host_eeg, np.ascontiguousarray(want[:-1].T.astype(np.float32)))
  assert hr.same_bits(status.cpu().numpy().reshape(-1), want[-1])
  for got, host in ((times, host_trial.find_status_trigger_times()[0]), (codes, host_trial.find_status_trigger_times()[1]),
                    (low_times, host_trial.find_status_trigger_times(mask=0xff)[0]),
                    (low_codes, host_trial.find_status_trigger_times(mask=0xff)[1])):
    assert got.dtype == host.dtype and np.array_equal(got, host)
  assert len(times) > 8 and codes.dtype == np.int64 and times.dtype == np.float64
