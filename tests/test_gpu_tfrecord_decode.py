"""The device TFRecord reader (td_tfrecord_decode through device.tfrecord_decode, tfrecord.read_file_device,
tfrecord.dataset_from_files(device=...) and brain_data.TFExampleData).

Every comparison is bitwise: the decoder copies bits.  The truth is tfrecord.read_file(name, fields, verify=True) on
the same file -- its values, or its exception (type and message)."""
import os

import numpy as np
import pytest

from telluride_decoding_amd import tfrecord
from tests import host_ingest as hi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, 'golden', 'meg_subj01_400.tfrecords')
NAMES = ('a', 'bb', 'ccc', 'dddd', 'eeeee')


@pytest.fixture(scope='module')
def torch():
  import torch as t
  return t


@pytest.fixture(scope='module')
def device():
  from telluride_decoding_amd import device as module
  assert module.gpu_available()
  return module


@pytest.fixture
def fallbacks(monkeypatch):
  """The files read_file_device handed to the host reader."""
  calls = []
  inner = tfrecord._device_fallback
  monkeypatch.setattr(tfrecord, '_device_fallback', lambda name, *a, **k: calls.append(name) or inner(name, *a, **k))
  return calls


def read_bytes(path):
  with open(path, 'rb') as f:
    return f.read()


def write_bytes(path, data):
  with open(path, 'wb') as f:
    f.write(bytes(data))
  return path


def outcome(call):
  """('ok', {name: uint32 array}) or ('raised', type, message)."""
  try:
    out = call()
  except Exception as e:   # pylint: disable=broad-except
    return ('raised', type(e), str(e))
  arrays = {}
  for k, v in out.items():
    v = v if isinstance(v, np.ndarray) else v.cpu().numpy()
    assert v.dtype == np.float32 and v.ndim == 2
    arrays[k] = np.ascontiguousarray(v).view(np.uint32)
  return ('ok', arrays)


def same_outcome(got, want):
  if got[0] != want[0]:
    return False
  if got[0] == 'raised':
    return got[1:] == want[1:]
  return set(got[1]) == set(want[1]) and all(got[1][k].shape == want[1][k].shape and
                                             np.array_equal(got[1][k], want[1][k]) for k in want[1])


def check_file(path, fields=None, handle=None):
  """read_file_device against read_file(verify=True); returns the common outcome."""
  want = outcome(lambda: tfrecord.read_file(path, fields, verify=True))
  got = outcome(lambda: tfrecord.read_file_device(path, fields, handle=handle))
  assert same_outcome(got, want), (path, fields, got if got[0] == 'raised' else 'arrays differ', want[0])
  return want


def frames_for(device, stride):
  """Both sides of every group edge of the stride's own route (three records on the large route)."""
  staged, group, _ = device.tfrecord_route(stride)
  if not staged:
    return [1, 2, 3]
  return sorted({n for n in (1, 2, group - 1, group, group + 1, 2 * group + 3) if n >= 1})


def stride_of(widths):
  return len(tfrecord.record_template(widths)[0])


# ---------------------------------------------------------------- valid files
def test_the_reference_file(device, fallbacks):
  want = check_file(GOLDEN_FILE)
  assert want[0] == 'ok' and len(want[1]) == 2
  for name in want[1]:
    one = check_file(GOLDEN_FILE, [name])
    assert set(one[1]) == {name}
  assert fallbacks == []
  missing = check_file(GOLDEN_FILE, ['no_such_feature'])
  assert missing[0] == 'raised' and 'Could not find all desired features' in missing[2]


@pytest.mark.parametrize('width', [1, 2, 3, 63, 64, 65, 4096])
def test_framing_sweep(device, tmp_path, fallbacks, width):
  """One feature, its name 1 to 5 letters long (every residue of payload offset and stride mod 4), over the edges of
  the stride's own group."""
  residues, routes = set(), set()
  for i, name in enumerate(NAMES):
    template, layout = tfrecord.record_template({name: width})
    residues.add((layout[0][1] % 4, len(template) % 4))
    routes.add(device.tfrecord_route(len(template))[0])
    for frames in frames_for(device, len(template)):
      path = str(tmp_path / ('%s_%d.tfrecords' % (name, frames)))
      tfrecord.write_file(path, {name: hi.fill_bits((frames, width), np.float32, 31 * width + 7 * frames + i)})
      assert check_file(path)[0] == 'ok'
  assert {r[0] for r in residues} == {0, 1, 2, 3} and {r[1] for r in residues} == {0, 1, 2, 3}
  assert fallbacks == []
  if width == 4096:
    assert routes == {True, False}          # (an odd stride needs 16 records in a group: more than the staging area)


def test_both_sides_of_the_route_predicate(device, tmp_path, fallbacks):
  """The widest record that is staged, the first that is not, and the record that fills the staging area alone."""
  large = next(w for w in range(1, 13000) if not device.tfrecord_route(stride_of({'x': w}))[0])
  assert large > 1 and device.tfrecord_route(stride_of({'x': large - 1}))[0]
  cases = [('x', large - 1), ('x', large)]
  stride, name, width = max((stride_of({n: w}), n, w) for n in NAMES for w in range(12250, 12290)
                            if device.tfrecord_route(stride_of({n: w}))[0])
  assert stride % 16 == 0 and device.tfrecord_route(stride)[1] == 1
  cases.append((name, width))
  for i, (name, width) in enumerate(cases):
    for frames in (1, 3):
      path = str(tmp_path / ('edge_%d_%d.tfrecords' % (i, frames)))
      tfrecord.write_file(path, {name: hi.fill_bits((frames, width), np.float32, width + frames)})
      assert check_file(path)[0] == 'ok'
  assert fallbacks == []


@pytest.mark.parametrize('count', [1, 2, 5])
def test_several_features(device, tmp_path, fallbacks, count):
  widths = dict(zip(NAMES[:count], (3, 64, 1, 17, 2)))
  stride = stride_of(widths)
  for frames in frames_for(device, stride):
    path = str(tmp_path / ('many_%d.tfrecords' % frames))
    tfrecord.write_file(path, {k: hi.fill_bits((frames, w), np.float32, frames + w) for k, w in widths.items()})
    assert check_file(path)[0] == 'ok'
    for name in widths:
      assert set(check_file(path, [name])[1]) == {name}
    if count == 5:
      assert set(check_file(path, ['bb', 'eeeee'])[1]) == {'bb', 'eeeee'}
  assert fallbacks == []


def test_bit_patterns(device, tmp_path, fallbacks):
  """+-0, +-Inf, quiet and signalling NaNs with payloads, the smallest and largest denormals, FLT_MAX: as uint32."""
  bits = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7fc12345, 0x7f800001,
                   0xffbfffff, 0x7fa00001, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x7f7fffff, 0xff7fffff,
                   0x00800000, 0x3f800000, 0xdeadbeef, 0x01020304], np.uint32)
  data = np.resize(bits, (70, 7)).copy()
  path = str(tmp_path / 'bits.tfrecords')
  # (serialize_example views the float32 bytes: no arithmetic touches a signalling NaN on the way to the file)
  tfrecord.write_file(path, {'v': data.view(np.float32)})
  want = check_file(path)
  assert np.array_equal(want[1]['v'], data)
  assert fallbacks == []


# ---------------------------------------------------------------- destinations
def upload(torch, path):
  return torch.from_numpy(np.fromfile(path, np.uint8)).cuda()


def test_destinations(torch, device, tmp_path):
  """A column offset inside a wider tensor, a row stride above the width, a first row, one payload to two
  destinations, a payload that nobody asks for: everything outside the destinations keeps the sentinel."""
  staged, group, _ = device.tfrecord_route(stride_of({'a': 3, 'bb': 5, 'ccc': 2}))
  assert staged
  frames = group + 3
  data = {'a': hi.fill_bits((frames, 3), np.float32, 1), 'bb': hi.fill_bits((frames, 5), np.float32, 2),
          'ccc': hi.fill_bits((frames, 2), np.float32, 3)}
  path = str(tmp_path / 'dest.tfrecords')
  tfrecord.write_file(path, data)
  plan = tfrecord.decode_plan(path)
  image = upload(torch, path)
  sentinel = np.uint32(0x7fedcba9)
  wide = torch.full((frames + 9, 17), float('nan'), device='cuda')
  wide.view(torch.int32).fill_(int(sentinel))
  other = wide.clone()
  view = other[:, 2:9]                              # rows 17 floats apart, 7 wide
  status = device.tfrecord_decode(image, plan, [('bb', wide, 4, 6), ('a', wide, 4, 0), ('a', wide, 4, 13),
                                                ('a', view, 2, 1)])
  assert status.dtype == torch.int64 and status.cpu().tolist() == [-1]
  want = np.full((frames + 9, 17), sentinel, np.uint32)
  want[4:4 + frames, 6:11] = data['bb'].view(np.uint32)
  want[4:4 + frames, 0:3] = data['a'].view(np.uint32)
  want[4:4 + frames, 13:16] = data['a'].view(np.uint32)
  assert np.array_equal(wide.cpu().numpy().view(np.uint32), want)
  want = np.full((frames + 9, 17), sentinel, np.uint32)
  want[2:2 + frames, 3:6] = data['a'].view(np.uint32)
  assert np.array_equal(other.cpu().numpy().view(np.uint32), want)
  # no output at all: only the checks
  assert device.tfrecord_decode(image, plan, []).cpu().tolist() == [-1]


def test_argument_checks(torch, device, tmp_path):
  path = str(tmp_path / 'args.tfrecords')
  tfrecord.write_file(path, {'a': hi.fill_bits((5, 3), np.float32, 1)})
  plan = tfrecord.decode_plan(path)
  image = upload(torch, path)
  dst = torch.zeros((5, 4), device='cuda')
  for outputs in ([('a', dst, 1, 0)], [('a', dst, 0, 2)], [('a', dst.double(), 0, 0)], [('a', dst.t(), 0, 0)]):
    with pytest.raises(ValueError):
      device.tfrecord_decode(image, plan, outputs)
  with pytest.raises(ValueError, match='outputs'):
    device.tfrecord_decode(image, plan, [('a', dst, 0, 0)] * 17)
  with pytest.raises(ValueError, match='aligned'):
    device.tfrecord_decode(torch.cat([image[:4], image])[4:], plan, [('a', dst, 0, 0)])
  wrong = dict(plan, template=bytes(8) + plan['template'][8:])
  with pytest.raises(ValueError, match='length field'):
    device.tfrecord_decode(image, wrong, [('a', dst, 0, 0)])
  outside = dict(plan, layout=[('a', plan['stride'] - 8, 3)])
  with pytest.raises(ValueError, match='outside'):
    device.tfrecord_decode(image, outside, [('a', dst, 0, 0)])
  assert torch.count_nonzero(dst).item() == 0


# ---------------------------------------------------------------- corruption
def flip(image, at, bit=0x04, fix_crc_of=None, stride=None):
  out = bytearray(image)
  out[at] ^= bit
  if fix_crc_of is not None:                        # the record's data CRC made valid again
    r0 = fix_crc_of * stride
    crc = tfrecord.masked_crc32c(bytes(out[r0 + 12:r0 + stride - 4]))
    out[r0 + stride - 4:r0 + stride] = int(crc).to_bytes(4, 'little')
  return out


def test_corrupt_files(device, tmp_path, fallbacks):
  widths = {'eeg': 5, 'wav': 2}
  stride = stride_of(widths)
  staged, group, _ = device.tfrecord_route(stride)
  assert staged
  frames = 2 * group + 3
  good = str(tmp_path / 'good.tfrecords')
  tfrecord.write_file(good, {k: hi.fill_bits((frames, w), np.float32, w) for k, w in widths.items()})
  image = read_bytes(good)
  plan = tfrecord.decode_plan(good)
  assert plan['stride'] == stride and plan['frames'] == frames
  payload = dict((k, o) for k, o, _ in plan['layout'])

  def case(tag, data, fields=None):
    return check_file(write_bytes(str(tmp_path / (tag + '.tfrecords')), data), fields)

  def crc_error(tag, record):
    return ('raised', ValueError, '%s: corrupt data CRC at byte %d' % (str(tmp_path / (tag + '.tfrecords')),
                                                                        record * stride))

  # one bit of a payload byte: the first record, the last of a full group, the first of the next group, the last of
  # the partial group -- asked for or not, the record's CRC covers it
  for record in (0, group - 1, group, frames - 1):
    for fields in (None, ['wav']):
      tag = 'payload_%d_%s' % (record, 'all' if fields is None else 'wav')
      assert case(tag, flip(image, record * stride + payload['eeg'] + 6), fields) == crc_error(tag, record)
  # the stored data CRC itself
  assert case('stored', flip(image, 3 * stride + stride - 2)) == crc_error('stored', 3)
  # two damaged records: the lower one is named, whichever workgroup finishes first
  twice = flip(flip(image, (group + 5) * stride + payload['wav']), 2 * stride + payload['eeg'] + 1)
  assert case('two', twice) == crc_error('two', 2)
  assert fallbacks == []

  # the skeleton: the host reader decides.  A protobuf tag and a feature name, with and without a valid data CRC
  tag_at = payload['eeg'] - 2                       # the FloatList's `value` tag, two bytes before the payload
  assert image[tag_at] == 0x0a
  name_at = image.index(b'eeg')
  assert 12 < name_at < stride
  r = group + 1
  n = 0
  for at, bit in ((tag_at, 0x10), (name_at, 0x02), (12, 0x08)):
    for fix in (None, r):
      got = case('skeleton_%d_%s' % (at, fix), flip(image, r * stride + at, bit, fix, stride))
      n += 1
      assert len(fallbacks) == n
      if fix is None:
        assert got[0] == 'raised' and 'corrupt data CRC at byte %d' % (r * stride) in got[2]
  renamed = case('renamed', flip(image, r * stride + name_at, 0x02, r, stride))
  assert renamed[0] == 'ok' and renamed[1]['eeg'].shape[0] == frames - 1          # (the flip still parses)
  # the length field and the length CRC of a middle record, and of the first
  for tag, at in (('length', r * stride + 1), ('lengthcrc', r * stride + 9), ('length0', 0), ('lengthcrc0', 10)):
    got = case(tag, flip(image, at))
    assert got[0] == 'raised' and got[1] is ValueError
  assert 'corrupt length CRC at byte %d' % (r * stride) in case('lengthcrc_again', flip(image, r * stride + 9))[2]
  # a file cut in the middle of a record
  got = case('cut', image[:5 * stride + 40])
  assert got[0] == 'raised' and 'truncated' in got[2]
  # a CRC failure below a skeleton failure is the CRC's; above it, the host's (which stops at the skeleton's record)
  both = flip(flip(image, 9 * stride + 1), 2 * stride + payload['eeg'])
  assert case('both', both) == crc_error('both', 2)
  both = flip(flip(image, 2 * stride + 9), 9 * stride + payload['eeg'])
  assert 'corrupt length CRC at byte %d' % (2 * stride) in case('both2', both)[2]


def test_corrupt_payload_on_the_large_route(device, tmp_path, fallbacks):
  width = next(w for w in range(12000, 13000) if not device.tfrecord_route(stride_of({'x': w}))[0])
  path = str(tmp_path / 'large.tfrecords')
  tfrecord.write_file(path, {'x': hi.fill_bits((3, width), np.float32, 4)})
  plan = tfrecord.decode_plan(path)
  image = read_bytes(path)
  for record in (0, 2):
    bad = write_bytes(str(tmp_path / ('large_%d.tfrecords' % record)),
                      flip(image, record * plan['stride'] + plan['layout'][0][1] + 4 * (width - 1) + 3, 0x80))
    assert check_file(bad) == ('raised', ValueError, '%s: corrupt data CRC at byte %d' % (bad, record * plan['stride']))
  assert fallbacks == []
  got = check_file(write_bytes(str(tmp_path / 'large_name.tfrecords'), flip(image, plan['stride'] + 20, 0x01)))
  assert got[0] == 'raised' and len(fallbacks) == 1


def test_irregular_files(device, tmp_path, fallbacks):
  rng = np.random.default_rng(5)
  eeg = rng.standard_normal((9, 4)).astype(np.float32)
  typed = str(tmp_path / 'typed.tfrecords')
  tfrecord.write_file_typed(typed, {'eeg': eeg, 'label': np.arange(9, dtype=np.int64).reshape(9, 1)})
  got = check_file(typed)
  assert got[0] == 'ok' and np.array_equal(got[1]['eeg'], eeg.view(np.uint32))
  assert check_file(typed, ['label'])[0] == 'ok'
  a, b = str(tmp_path / 'a.tfrecords'), str(tmp_path / 'b.tfrecords')
  tfrecord.write_file(a, {'eeg': eeg})
  tfrecord.write_file(b, {'eeg': eeg[:, :3]})
  changes = write_bytes(str(tmp_path / 'changes.tfrecords'), read_bytes(a) + read_bytes(b))
  got = check_file(changes)
  assert got[0] == 'raised' and 'changes width' in got[2]
  assert len(fallbacks) == 3


# ---------------------------------------------------------------- determinism
def test_same_bits_on_every_call_and_on_a_cu_masked_stream(torch, device, tmp_path):
  from telluride_decoding_amd import pipeline
  widths = {'eeg': 64, 'env': 2}
  stride = stride_of(widths)
  frames = 5 * device.tfrecord_route(stride)[1] + 7
  path = str(tmp_path / 'det.tfrecords')
  tfrecord.write_file(path, {k: hi.fill_bits((frames, w), np.float32, w) for k, w in widths.items()})
  good = read_bytes(path)
  plan = tfrecord.decode_plan(path)
  at = plan['layout'][0][1]
  assert frames > 200
  # payload bits in records 200 and 77, the length field of record 78: the status names record 77's CRC
  bad = write_bytes(str(tmp_path / 'det_bad.tfrecords'),
                    flip(flip(flip(good, 200 * stride + at + 9), 77 * stride + at + 19), 78 * stride + 3))
  h = device.default_handle()
  pipe = pipeline.FitPipeline(16, 0, 3, d=1)
  assert pipe._masked, 'the pipeline did not get its CU-masked streams'

  def run(image, handle):
    out = {k: torch.zeros((frames, w), device='cuda') for k, w in widths.items()}
    status = device.tfrecord_decode(image, plan, [(k, out[k], 0, 0) for k in widths], handle=handle)
    handle.synchronize()
    return status.cpu().tolist(), {k: v.cpu().numpy().view(np.uint32) for k, v in out.items()}

  for name, want_status in ((path, [-1]), (bad, [(77 << 2) | 2])):
    image = upload(torch, name)
    torch.cuda.synchronize()
    first = run(image, h)
    assert first[0] == want_status
    again = run(image, h)
    with torch.cuda.stream(pipe.s_solve):
      masked = run(image, pipe.h_solve)
    torch.cuda.synchronize()
    for other in (again, masked):
      assert other[0] == first[0]
      if want_status == [-1]:
        assert all(np.array_equal(other[1][k], first[1][k]) for k in widths)
  with torch.cuda.stream(pipe.s_solve):
    got = outcome(lambda: tfrecord.read_file_device(path, handle=pipe.h_solve))
  assert same_outcome(got, outcome(lambda: tfrecord.read_file(path, verify=True)))


# ---------------------------------------------------------------- datasets
@pytest.fixture(scope='module')
def three_files(tmp_path_factory):
  """Recordings of 1, 37 and 300 frames, and a '-bad-' file that must be skipped."""
  root = tmp_path_factory.mktemp('three')
  names = []
  for i, frames in enumerate((1, 37, 300)):
    rng = np.random.default_rng(20 + i)
    name = str(root / ('rec_%d.tfrecords' % i))
    tfrecord.write_file(name, {'eeg': rng.standard_normal((frames, 8)).astype(np.float32),
                               'aud': rng.standard_normal((frames, 3)).astype(np.float32),
                               'env': rng.standard_normal((frames, 2)).astype(np.float32),
                               'att': (rng.random((frames, 1)) > 0.5).astype(np.float32),
                               'unused': rng.standard_normal((frames, 5)).astype(np.float32)})
    names.append(name)
  names.insert(1, write_bytes(str(root / 'rec-bad-9.tfrecords'), b'not a TFRecord file'))
  return names


def same_files(a, b):
  return len(a.files) == len(b.files) and all(
      len(fa) == len(fb) == 4 and all(hi.same_bits(x, y) for x, y in zip(fa, fb)) for fa, fb in zip(a.files, b.files))


def check_dataset(torch, device, names, counted=True, **kw):
  h = device.default_handle()
  host = tfrecord.dataset_from_files(names, batch_size=16, **kw)
  dev = tfrecord.dataset_from_files(names, batch_size=16, device=h, **kw)
  assert same_files(dev, host)
  want = host.device_arrays(h)
  calls = []
  to_device, empty = h.to_device, h.empty
  h.to_device = lambda *a, **k: calls.append('to_device') or to_device(*a, **k)
  h.empty = lambda *a, **k: calls.append('empty') or empty(*a, **k)
  try:
    got = dev.device_arrays(h)
  finally:
    del h.to_device, h.empty
  assert calls == []                                  # nothing is uploaded again
  for g, w in zip(got[:3], want[:3]):
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == w.shape
    assert torch.equal(g.view(torch.int32), w.view(torch.int32))
  assert np.array_equal(got[3], want[3])
  assert (dev.c1, dev.c2, dev.d, dev.num_batches()) == (host.c1, host.c2, host.d, host.num_batches())
  return dev, host


@pytest.mark.parametrize('kw', [
    dict(in1_fields=['eeg', 'aud'], out_field='env'),
    dict(in1_fields=['eeg', 'aud'], out_field='ones', in2_fields=['env', 'eeg'], attended_field='att'),
    dict(in1_fields='eeg', out_field='env', in2_fields='aud', post_context=3, input_offset=1),
], ids=['plain', 'ones_in2_attended', 'strings'])
def test_dataset_from_files_on_the_device(torch, device, three_files, kw):
  dev, host = check_dataset(torch, device, three_files, **kw)
  assert [f[0].shape[0] for f in dev.files] == [1, 37, 300]
  for f in dev.files:
    assert all(a.flags['C_CONTIGUOUS'] and a.dtype == np.float32 for a in f)


def test_dataset_with_a_preprocessed_field(torch, device, three_files):
  """Both routes run the same kernels on the same float32 values (the device route asks the Preprocessor for the
  float64 result the host route gets, and rounds it to float32 as np.asarray does): equal bitwise, on the recordings
  of 1, 37 and 300 frames."""
  names = three_files
  spec = 'eeg(highpass_cutoff=0.5;highpass_order=2;channel_numbers=0-3,7)'
  dev, host = check_dataset(torch, device, names, in1_fields=['eeg', 'aud'], out_field='env', in2_fields='eeg',
                            preprocess={'eeg': spec}, frame_rate=128)
  assert dev.c1 == 5 + 3 and dev.c2 == 5


def test_dataset_with_a_file_the_host_reads(torch, device, tmp_path, three_files):
  """A file whose skeleton check fails (a renamed feature that nobody asks for, its CRC valid) is read on the host
  and uploaded into its rows; a damaged payload raises."""
  image = bytearray(read_bytes(three_files[2]))
  plan = tfrecord.decode_plan(three_files[2])
  at = image.index(b'unused')
  odd = write_bytes(str(tmp_path / 'odd.tfrecords'), flip(image, 5 * plan['stride'] + at, 0x02, 5, plan['stride']))
  names = [three_files[0], odd, three_files[3]]
  check_dataset(torch, device, names, in1_fields=['eeg', 'aud'], out_field='env')
  damaged = write_bytes(str(tmp_path / 'damaged.tfrecords'),
                        flip(image, 30 * plan['stride'] + dict((k, o) for k, o, _ in plan['layout'])['unused']))
  names = [three_files[0], damaged, three_files[3]]
  tfrecord.dataset_from_files(names, 'eeg', 'env')                    # (the host route never looks)
  with pytest.raises(ValueError) as e:
    tfrecord.dataset_from_files(names, 'eeg', 'env', device=device.default_handle())
  assert str(e.value) == '%s: corrupt data CRC at byte %d' % (damaged, 30 * plan['stride'])


def test_more_features_than_one_launch_takes(device, tmp_path, fallbacks):
  """Eighteen features: read_file_device decodes them in two launches, not on the host."""
  names = ['f%02d' % i for i in range(18)]
  assert len(names) > device.TFRECORD_MAX_OUTPUTS
  path = str(tmp_path / 'many.tfrecords')
  tfrecord.write_file(path, {k: hi.fill_bits((70, 1 + i % 3), np.float32, i) for i, k in enumerate(names)})
  assert set(check_file(path)[1]) == set(names)
  assert set(check_file(path, names[1:])[1]) == set(names[1:])
  bad = write_bytes(str(tmp_path / 'many_bad.tfrecords'),
                    flip(read_bytes(path), 69 * tfrecord.decode_plan(path)['stride'] + tfrecord.decode_plan(path)['layout'][17][1]))
  assert check_file(bad)[0] == 'raised'
  assert fallbacks == []


def test_dataset_with_a_renamed_requested_feature(device, tmp_path, three_files):
  """A record whose requested feature is renamed (its CRC valid) still parses, one row short: a worded error."""
  image = bytearray(read_bytes(three_files[2]))
  plan = tfrecord.decode_plan(three_files[2])
  at = image.index(b'eeg')
  short = write_bytes(str(tmp_path / 'short.tfrecords'), flip(image, 5 * plan['stride'] + at, 0x02, 5, plan['stride']))
  assert tfrecord.read_file(short, ['eeg', 'env'], verify=True)['eeg'].shape[0] == plan['frames'] - 1
  with pytest.raises(ValueError, match='its first record promises'):
    tfrecord.dataset_from_files([three_files[0], short], 'eeg', 'env', device=device.default_handle())


# ---------------------------------------------------------------- TFExampleData, end to end
@pytest.fixture(scope='module')
def recordings(tmp_path_factory):
  """The six-recording recipe of the decoding experiment (16 channels, 3000 frames)."""
  from telluride_decoding_amd import synth
  root = tmp_path_factory.mktemp('recordings')
  for i, (eeg, env, att) in enumerate(synth.make_trials(17, 6, 3000, 16)):
    label = (np.arange(3000) % 2).astype(np.float32).reshape(-1, 1)
    tfrecord.write_file(str(root / ('subj_trial_%d.tfrecords' % i)),
                        {'eeg': eeg, 'envelope': env[:, 0:1], 'attend': att, 'label': label})
  return str(root)


def brain_data_of(recordings, **kw):
  from telluride_decoding_amd import brain_data
  return brain_data.create_brain_dataset(
      'tfrecords', 'eeg', 'envelope', 100.0, pre_context=0, post_context=21, attended_field='attend',
      final_batch_size=512, data_dir=recordings, train_file_pattern='allbut', test_file_pattern='trial_0',
      validate_file_pattern='trial_1', **kw)


def test_create_dataset_default_is_the_device_route(torch, device, recordings, monkeypatch):
  calls = []
  inner = device.tfrecord_decode
  monkeypatch.setattr(device, 'tfrecord_decode', lambda *a, **k: calls.append(1) or inner(*a, **k))
  default, host = brain_data_of(recordings), brain_data_of(recordings, decode_on_device=False)
  for mode, files in (('train', 4), ('test', 1)):
    n = len(calls)
    a = default.create_dataset(mode)
    assert len(calls) == n + files
    b = host.create_dataset(mode)
    assert len(calls) == n + files
    assert same_files(a, b) and a.rows_used() == b.rows_used()
    assert a._device_cache is not None and b._device_cache is None


def test_run_decoding_experiment_same_results_on_both_routes(device, recordings, tmp_path, monkeypatch):
  from telluride_decoding_amd import brain_data, decoding

  def run(tag):
    flags = decoding.DecodingOptions().set_from_dict(dict(
        tfexample_dir=recordings, input_field='eeg', output_field='envelope', dnn_regressor='linear',
        pre_context=0, post_context=21, train_file_pattern='allbut', test_file_pattern='trial_0',
        validate_file_pattern='trial_1', correlation_frames=100, batch_size=512,
        summary_dir=str(tmp_path / tag)))
    return decoding.run_decoding_experiment(flags)

  calls = []
  inner = device.tfrecord_decode
  monkeypatch.setattr(device, 'tfrecord_decode', lambda *a, **k: calls.append(1) or inner(*a, **k))
  on_device = run('device')
  assert calls
  n = len(calls)
  monkeypatch.setattr(brain_data.TFExampleData, 'DECODE_ON_DEVICE', False)
  on_host = run('host')
  assert len(calls) == n
  assert on_device[0] == on_host[0] and on_device[1] == on_host[1] and on_device[2] == on_host[2]
  assert on_device[2] > 1.0


def test_a_damaged_test_file_raises_on_the_device_route_only(device, recordings, tmp_path):
  import shutil
  root = str(tmp_path / 'copy')
  shutil.copytree(recordings, root)
  name = os.path.join(root, 'subj_trial_0.tfrecords')
  plan = tfrecord.decode_plan(name)
  at = 1234 * plan['stride'] + dict((k, o) for k, o, _ in plan['layout'])['eeg'] + 17
  write_bytes(name, flip(read_bytes(name), at, 0x01))
  with pytest.raises(ValueError) as e:
    brain_data_of(root).create_dataset('test')
  assert str(e.value) == '%s: corrupt data CRC at byte %d' % (name, 1234 * plan['stride'])
  ds = brain_data_of(root, decode_on_device=False).create_dataset('test')
  assert ds.files[0][0].shape == (3000, 16)
  brain_data_of(root).create_dataset('train')         # (the other files are sound)
