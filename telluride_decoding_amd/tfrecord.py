"""Dependency-free TFRecord / tf.train.Example reader and writer.

The step before the hot path: the reference stores every recording as a TFRecord file of
tf.train.Example protos, ONE EXAMPLE PER FRAME, each feature a FloatList (writer
ingest.BrainTrial.write_data_as_tfrecords, ingest.py:612-651; reader
brain_data.TFExampleData, brain_data.py:733-839, discover_feature_shapes :887-927,
count_tfrecords :930-956).  TensorFlow is not a dependency of this package, so the two wire
formats are parsed here directly:

  TFRecord framing   uint64 length | uint32 masked-crc32c(length) | data | uint32 masked-crc32c(data)
  tf.train.Example   message Example  { Features features = 1; }
                     message Features { map<string, Feature> feature = 1; }
                     message Feature  { oneof kind { BytesList bytes_list = 1;
                                                     FloatList float_list = 2;
                                                     Int64List int64_list = 3; } }
                     FloatList / Int64List: repeated value = 1 (packed or not)

read_file() returns {feature name: float32 [frames, width]} -- the row-major time x channel
arrays the kernels take; dataset_from_files() applies the reference's field selection
(parse_and_select_from_tfrecord, brain_data.py:777-839: concatenated in1/in2 fields, the 'ones'
pseudo output, the placeholder input_2 / attended_speaker) and returns a brain_data.Dataset.
"""
import os
import struct

import numpy as np

_MASK_DELTA = 0xa282ead8


def _make_crc_table():
  poly = 0x82f63b78            # CRC-32C (Castagnoli), reflected
  table = []
  for i in range(256):
    c = i
    for _ in range(8):
      c = (c >> 1) ^ poly if c & 1 else c >> 1
    table.append(c)
  return table


_CRC_TABLE = _make_crc_table()


def crc32c(data):
  crc = 0xffffffff
  tab = _CRC_TABLE
  for b in data:
    crc = tab[(crc ^ b) & 0xff] ^ (crc >> 8)
  return crc ^ 0xffffffff


def masked_crc32c(data):
  crc = crc32c(data)
  return ((((crc >> 15) | (crc << 17)) & 0xffffffff) + _MASK_DELTA) & 0xffffffff


# ---------------------------------------------------------------- protobuf wire format
def _varint(buf, pos):
  result, shift = 0, 0
  while True:
    b = buf[pos]
    pos += 1
    result |= (b & 0x7f) << shift
    if not b & 0x80:
      return result, pos
    shift += 7


def _fields(buf):
  """Yields (field number, wire type, value) of one message; length-delimited values are
  memoryview slices."""
  pos, end = 0, len(buf)
  while pos < end:
    key, pos = _varint(buf, pos)
    num, wt = key >> 3, key & 7
    if wt == 0:
      val, pos = _varint(buf, pos)
    elif wt == 1:
      val, pos = buf[pos:pos + 8], pos + 8
    elif wt == 2:
      n, pos = _varint(buf, pos)
      val, pos = buf[pos:pos + n], pos + n
    elif wt == 5:
      val, pos = buf[pos:pos + 4], pos + 4
    else:
      raise ValueError('unsupported protobuf wire type %d' % wt)
    if pos > end:
      raise ValueError('truncated protobuf message')
    yield num, wt, val


def _parse_feature(buf):
  """Feature -> np.ndarray (float32 / int64) or list of bytes."""
  for num, wt, val in _fields(buf):
    if wt != 2:
      continue
    if num == 2:      # FloatList
      out = []
      for n2, w2, v2 in _fields(val):
        if n2 == 1 and w2 == 2:                      # packed
          out.append(np.frombuffer(v2, dtype='<f4'))
        elif n2 == 1 and w2 == 5:                    # one value
          out.append(np.frombuffer(v2, dtype='<f4'))
      return np.concatenate(out) if out else np.zeros((0,), np.float32)
    if num == 3:      # Int64List
      out = []
      for n2, w2, v2 in _fields(val):
        if n2 == 1 and w2 == 2:
          p, vals = 0, []
          while p < len(v2):
            x, p = _varint(v2, p)
            vals.append(x - (1 << 64) if x >= (1 << 63) else x)
          out.extend(vals)
        elif n2 == 1 and w2 == 0:
          out.append(v2 - (1 << 64) if v2 >= (1 << 63) else v2)
      return np.asarray(out, np.int64)
    if num == 1:      # BytesList
      return [bytes(v2) for n2, w2, v2 in _fields(val) if n2 == 1 and w2 == 2]
  return np.zeros((0,), np.float32)


def parse_example(record):
  """One serialized tf.train.Example -> {name: values}."""
  out = {}
  buf = memoryview(record)
  for num, wt, features in _fields(buf):
    if num != 1 or wt != 2:
      continue
    for n2, w2, entry in _fields(features):          # map<string, Feature> entries
      if n2 != 1 or w2 != 2:
        continue
      key, feat = None, None
      for n3, w3, v3 in _fields(entry):
        if n3 == 1 and w3 == 2:
          key = bytes(v3).decode('utf-8')
        elif n3 == 2 and w3 == 2:
          feat = v3
      if key is not None:
        out[key] = _parse_feature(feat) if feat is not None else np.zeros((0,), np.float32)
  return out


# ---------------------------------------------------------------- TFRecord framing
def iter_records(filename, verify=False):
  """Yields the raw records of a TFRecord file.  verify=True checks both CRCs."""
  with open(filename, 'rb') as f:
    data = f.read()
  pos, end = 0, len(data)
  view = memoryview(data)
  while pos < end:
    if pos + 12 > end:
      raise ValueError('%s: truncated record header at byte %d' % (filename, pos))
    (length,) = struct.unpack_from('<Q', data, pos)
    if verify and struct.unpack_from('<I', data, pos + 8)[0] != masked_crc32c(view[pos:pos + 8]):
      raise ValueError('%s: corrupt length CRC at byte %d' % (filename, pos))
    start = pos + 12
    if start + length + 4 > end:
      raise ValueError('%s: truncated record at byte %d' % (filename, pos))
    rec = view[start:start + length]
    if verify and struct.unpack_from('<I', data, start + length)[0] != masked_crc32c(rec):
      raise ValueError('%s: corrupt data CRC at byte %d' % (filename, pos))
    yield rec
    pos = start + length + 4


def count_tfrecords(tfrecord_file_name):
  """(valid records, error found) like brain_data.count_tfrecords (brain_data.py:930-956)."""
  if not isinstance(tfrecord_file_name, str):
    raise TypeError('tfrecord_file_name must be a string.')
  count = 0
  try:
    for rec in iter_records(tfrecord_file_name):
      parse_example(rec)
      count += 1
  except Exception:   # pylint: disable=broad-except
    return count, True
  return count, False


def discover_feature_shapes(tfrecord_file_name):
  """{feature name: (width, dtype)} of the first record (brain_data.py:887-927)."""
  if not isinstance(tfrecord_file_name, str):
    raise TypeError('discover_feature_shapes: input must be a string filename.')
  for rec in iter_records(tfrecord_file_name):
    ex = parse_example(rec)
    return {k: (len(v), 'bytes' if isinstance(v, list) else str(v.dtype)) for k, v in ex.items()}
  return {}


def _float_layout(record):
  """[(feature name, byte offset of its packed float payload in the record, float count)] when
  every feature of the Example is ONE packed FloatList (what the reference's ingest writes per
  frame), else None."""
  def fields_at(buf, base):
    pos, end = 0, len(buf)
    while pos < end:
      key, pos = _varint(buf, pos)
      num, wt = key >> 3, key & 7
      if wt != 2:
        raise ValueError('not a length-delimited field')
      n, pos = _varint(buf, pos)
      if pos + n > end:
        raise ValueError('truncated')
      yield num, buf[pos:pos + n], base + pos
      pos += n
  out = []
  try:
    buf = memoryview(record)
    for num, features, f0 in fields_at(buf, 0):
      if num != 1:
        return None
      for n2, entry, e0 in fields_at(features, f0):
        if n2 != 1:
          return None
        key, payload = None, None
        for n3, v3, v0 in fields_at(entry, e0):
          if n3 == 1:
            key = bytes(v3).decode('utf-8')
          elif n3 == 2:
            inner = list(fields_at(v3, v0))
            if len(inner) != 1 or inner[0][0] != 2:          # exactly one FloatList
              return None
            lists = list(fields_at(inner[0][1], inner[0][2]))
            if len(lists) != 1 or lists[0][0] != 1 or len(lists[0][1]) % 4:
              return None
            payload = (lists[0][2], len(lists[0][1]) // 4)
          else:
            return None
        if key is None or payload is None:
          return None
        out.append((key, payload[0], payload[1]))
  except (ValueError, IndexError, UnicodeDecodeError):
    return None
  return out or None


def _read_file_regular(filename, fields):
  """read_file for the regular case -- every record the same length and the same bytes outside
  its float payloads (one Example per frame, fixed feature widths) -- as array slicing of the whole
  file: no per-record Python (31 us a record through the generic parser: half a minute per 1e6
  frames).  None when the file is not of that shape."""
  size = os.path.getsize(filename)
  if size < 16:
    return None
  # the file is mapped, not read: the only copies are the feature blocks that are asked for (peak
  # host memory ~1x the payload instead of ~3x the file)
  data = np.memmap(filename, dtype=np.uint8, mode='r')
  (length,) = struct.unpack_from('<Q', bytes(data[:8]), 0)
  stride = length + 16
  if length == 0 or size % stride:
    return None
  layout = _float_layout(memoryview(bytes(data[12:12 + length])))
  if layout is None:
    return None
  arr = data.reshape(-1, stride)
  skeleton = np.ones(stride, bool)
  skeleton[8:12] = False                       # (CRC of the length: equal anyway)
  skeleton[12 + length:] = False               # CRC of the data
  for _, start, count in layout:
    skeleton[12 + start:12 + start + 4 * count] = False
  # every record's bytes outside its payloads against the first record's, in chunks of rows with an
  # early exit (a boolean copy of the whole file's skeleton was 1x the file again)
  cols = np.flatnonzero(skeleton)
  first = np.asarray(arr[0, cols])
  chunk = max(1, (8 << 20) // max(1, len(cols)))
  for r0 in range(0, arr.shape[0], chunk):
    if not np.array_equal(arr[r0:r0 + chunk][:, cols], np.broadcast_to(first, (min(chunk, arr.shape[0] - r0), len(cols)))):
      return None
  out = {}
  for key, start, count in layout:
    if fields is not None and key not in fields:
      continue
    if key in out:
      return None
    block = np.ascontiguousarray(arr[:, 12 + start:12 + start + 4 * count])
    if block.shape[0] == 1:
      block = block.copy()       # (one row counts as contiguous whatever its row stride: still the file's, not 4 * count)
    out[key] = block.view('<f4').astype(np.float32, copy=False)
  return out


def read_file(filename, fields=None, verify=False):
  """{feature: float32 [frames, width]} of the float / int features (one Example per frame)."""
  if not verify:
    out = _read_file_regular(filename, fields)
    if out is not None:
      if fields is not None:
        missing = set(fields) - set(out)
        if missing:
          raise ValueError('Could not find all desired features (%s) in data (%s)' %
                           (sorted(fields), sorted(out)))
      return out
  cols = {}
  for rec in iter_records(filename, verify=verify):
    ex = parse_example(rec)
    for k, v in ex.items():
      if isinstance(v, list) or (fields is not None and k not in fields):
        continue
      cols.setdefault(k, []).append(v)
  out = {}
  for k, rows in cols.items():
    widths = {len(r) for r in rows}
    if len(widths) != 1:
      raise ValueError('%s: feature %s changes width (%s)' % (filename, k, sorted(widths)))
    out[k] = np.stack(rows).astype(np.float32)
  if fields is not None:
    missing = set(fields) - set(out)
    if missing:
      raise ValueError('Could not find all desired features (%s) in data (%s)' %
                       (sorted(fields), sorted(out)))
  return out


# ---------------------------------------------------------------- device reader
def decode_plan(filename):
  """What device.tfrecord_decode needs to know about a regular file -- every record as long as the first and, outside
  its float payloads and its data CRC, the same bytes -- from its size and its first record; host only.
  {'stride': bytes per record, 'frames': records, 'template': the first record with payloads and data CRC zeroed,
  'mask': a byte per record byte, 1 where every record must equal the template (length, length CRC, protobuf tags,
  names and lengths), 0 on every float payload and the last 4 bytes, 'layout': [(feature name, byte offset of its
  payload in the record, floats)]}.  None when the file is not of that shape as far as the first record tells: too
  short, its size no multiple of the stride, a feature that is not one packed FloatList, a feature name twice, or a
  first record whose length CRC is wrong.  (Whether the other records keep to it is the device's skeleton check.)"""
  size = os.path.getsize(filename)
  if size < 16:
    return None
  with open(filename, 'rb') as f:
    head = f.read(12)
    (length,) = struct.unpack_from('<Q', head, 0)
    stride = length + 16
    if length == 0 or stride > (1 << 28) or size % stride:
      return None
    first = head + f.read(length + 4)
  if struct.unpack_from('<I', head, 8)[0] != masked_crc32c(head[:8]):
    return None
  layout = _float_layout(memoryview(first)[12:12 + length])
  if layout is None or len({k for k, _, _ in layout}) != len(layout):
    return None
  mask = np.ones(stride, np.uint8)
  mask[stride - 4:] = 0
  for _, start, count in layout:
    mask[12 + start:12 + start + 4 * count] = 0
  template = np.frombuffer(first, np.uint8) * mask
  return {'stride': stride, 'frames': size // stride, 'template': template.tobytes(), 'mask': mask.tobytes(),
          'layout': [(k, 12 + start, count) for k, start, count in layout]}


def _upload_image(filename, size, handle, pinned=None, image=None):
  """The file's bytes as a device uint8 tensor, through a pinned host buffer (both reused when given and large
  enough).  Queued on torch's current stream; returns (image, pinned buffer, event after the copy)."""
  import torch
  if pinned is None or pinned.numel() < size:
    pinned = torch.empty(size, dtype=torch.uint8, pin_memory=True)
  if image is None or image.numel() < size:
    image = handle.empty((size,), 'uint8')
  with open(filename, 'rb') as f:
    got = f.readinto(memoryview(pinned.numpy())[:size])
  if got != size:
    raise ValueError('%s: read %d of %d bytes' % (filename, got, size))
  image[:size].copy_(pinned[:size], non_blocking=True)
  done = torch.cuda.Event()
  done.record()
  return image, pinned, done


def _raise_missing(fields, found):
  missing = set(fields) - set(found)
  if missing:
    raise ValueError('Could not find all desired features (%s) in data (%s)' % (sorted(fields), sorted(found)))


def _device_fallback(filename, fields, handle):
  """read_file(verify=True) on the host -- the generic parser decides what is wrong with the file and words the
  error -- and its result uploaded."""
  return {k: handle.to_device(v) for k, v in read_file(filename, fields, verify=True).items()}


def read_file_device(filename, fields=None, handle=None):
  """read_file(filename, fields, verify=True) with the framing check, the CRC-32C of every record and the unpacking
  on the GPU (device.tfrecord_decode): {feature: device float32 [frames, width]}, the same values bit for bit, or
  the same exception.  A record r whose data CRC is wrong raises iter_records' ValueError('%s: corrupt data CRC at
  byte %d') with byte r * stride.  A file that is not regular (decode_plan None, or a record whose bytes outside the
  payloads differ from the first record's) is read by read_file(verify=True) on the host and uploaded."""
  import torch
  from telluride_decoding_amd import device
  h = handle or device.default_handle()
  plan = decode_plan(filename)
  if plan is None:
    return _device_fallback(filename, fields, h)
  wanted = [(k, count) for k, _, count in plan['layout'] if fields is None or k in fields]
  with torch.cuda.stream(h._stream):
    image, _, _ = _upload_image(filename, plan['frames'] * plan['stride'], h)
    out = {k: h.empty((plan['frames'], count), 'float32') for k, count in wanted}
    # (more features than one launch takes: several launches, each with all the checks, the lowest status counts)
    n = device.TFRECORD_MAX_OUTPUTS
    chunks = [wanted[c:c + n] for c in range(0, len(wanted), n)] or [[]]
    status = torch.full((len(chunks),), -1, dtype=torch.int64, device=h.device)
    for c, chunk in enumerate(chunks):
      device.tfrecord_decode(image, plan, [(k, out[k], 0, 0) for k, _ in chunk], handle=h, status=status[c:c + 1])
    code = int(status.cpu().numpy().view(np.uint64).min().astype(np.int64))
  if code != -1:
    if code & 3 == 2:
      raise ValueError('%s: corrupt data CRC at byte %d' % (filename, (code >> 2) * plan['stride']))
    return _device_fallback(filename, fields, h)
  if fields is not None:
    _raise_missing(fields, out)
  return out


# ---------------------------------------------------------------- writer
def _enc_varint(x):
  out = bytearray()
  while True:
    b = x & 0x7f
    x >>= 7
    if x:
      out.append(b | 0x80)
    else:
      out.append(b)
      return bytes(out)


def _ld(num, payload):
  return _enc_varint((num << 3) | 2) + _enc_varint(len(payload)) + payload


def serialize_example(features):
  """{name: 1-D float array} -> serialized tf.train.Example with packed FloatLists."""
  entries = b''
  for name in sorted(features):
    vals = np.asarray(features[name], '<f4').reshape(-1)
    float_list = _ld(1, vals.tobytes())
    feature = _ld(2, float_list)
    entries += _ld(1, _ld(1, name.encode('utf-8')) + _ld(2, feature))
  return _ld(1, entries)


def write_file(filename, data):
  """data: {name: [frames, width]} -> TFRecord file, one Example per frame
  (ingest.BrainTrial.write_data_as_tfrecords, ingest.py:612-651)."""
  n = {np.asarray(v).shape[0] for v in data.values()}
  if len(n) != 1:
    raise ValueError('all features need the same number of frames, not %s' % sorted(n))
  arrays = {k: np.asarray(v, np.float32).reshape(np.asarray(v).shape[0], -1) for k, v in data.items()}
  with open(filename, 'wb') as f:
    for i in range(n.pop()):
      rec = serialize_example({k: a[i] for k, a in arrays.items()})
      head = struct.pack('<Q', len(rec))
      f.write(head + struct.pack('<I', masked_crc32c(head)) + rec +
              struct.pack('<I', masked_crc32c(rec)))


def record_template(widths):
  """({name: floats per frame}) -> (template, layout) of the file write_file gives such features: template is one
  whole record with zero payloads -- 8 bytes of length, the masked CRC of those, the serialized Example, 4 zero
  bytes where the data CRC goes -- and layout [(name, byte offset of the payload in the record, floats)] in the
  record's order.  Every record of the file is these bytes but for its payloads and its data CRC: what a
  device-side encoder (device.tfrecord_encode) needs."""
  rec = serialize_example({k: np.zeros(int(w), np.float32) for k, w in widths.items()})
  layout = _float_layout(rec)
  if layout is None:
    raise ValueError('no fixed record layout for feature widths %s' % dict(widths))
  head = struct.pack('<Q', len(rec))
  template = head + struct.pack('<I', masked_crc32c(head)) + rec + b'\0\0\0\0'
  return template, [(k, 12 + start, count) for k, start, count in layout]


def _enc_int64(x):
  return _enc_varint(int(x) & 0xffffffffffffffff)


def serialize_example_typed(features):
  """serialize_example for rows of mixed kinds: a float row becomes a packed FloatList, an integer row a packed
  Int64List (convert_data_to_tfrecords, ingest.py:1155-1169)."""
  entries = b''
  for name in sorted(features):
    vals = np.asarray(features[name]).reshape(-1)
    if vals.dtype.kind in 'iu':
      feature = _ld(3, _ld(1, b''.join(_enc_int64(v) for v in vals)))
    else:
      feature = _ld(2, _ld(1, vals.astype('<f4').tobytes()))
    entries += _ld(1, _ld(1, name.encode('utf-8')) + _ld(2, feature))
  return _ld(1, entries)


def write_file_typed(filename, data):
  """write_file that keeps integer features as Int64Lists ({name: [frames, width]} of float or integer arrays)."""
  arrays = {k: np.asarray(v) for k, v in data.items()}
  n = {a.shape[0] for a in arrays.values()}
  if len(n) != 1:
    raise ValueError('all features need the same number of frames, not %s' % sorted(n))
  arrays = {k: a.reshape(a.shape[0], -1) for k, a in arrays.items()}
  with open(filename, 'wb') as f:
    for i in range(n.pop()):
      rec = serialize_example_typed({k: a[i] for k, a in arrays.items()})
      head = struct.pack('<Q', len(rec))
      f.write(head + struct.pack('<I', masked_crc32c(head)) + rec +
              struct.pack('<I', masked_crc32c(rec)))


# ---------------------------------------------------------------- field selection
def select_streams(features, in1_fields, out_field, in2_fields=None, attended_field=None):
  """(input_1, input_2, output, attended_speaker) of one recording, as
  brain_data.TFExampleData.parse_and_select_from_tfrecord builds them per frame
  (brain_data.py:777-839): listed fields concatenated; out_field 'ones' = a column of ones;
  no input_2 fields -> the first column of input_1; no attended field -> zeros."""
  in1_fields = [in1_fields] if isinstance(in1_fields, str) else list(in1_fields)
  in2_fields = [] if not in2_fields else ([in2_fields] if isinstance(in2_fields, str)
                                          else list(in2_fields))
  missing = set(in1_fields) - set(features)
  if missing:
    raise ValueError('Could not find all desired features (%s) in data (%s)' %
                     (in1_fields, sorted(features)))
  x = np.concatenate([features[k] for k in in1_fields], axis=1)
  if out_field == 'ones':
    y = np.ones((x.shape[0], 1), np.float32)
  else:
    y = features[out_field]
  if in2_fields:
    for k in in2_fields:
      if k not in features:
        raise ValueError('Could not find %s in parsed_features[%s]' % (k, sorted(features)))
    x2 = np.concatenate([features[k] for k in in2_fields], axis=1)
  else:
    x2 = x[:, 0:1]
  att = features[attended_field] if attended_field else np.zeros((x.shape[0], 1), np.float32)
  return x, x2, y, att


def _dataset_on_device(names, in1_fields, out_field, in2_fields, attended_field, wanted, preprocessors, handle):
  """dataset_from_files' device route: (files, device cache) of the recordings `names`.  The concatenated input_1,
  input_2, output and attention streams are allocated once on the device; every regular file is uploaded through a
  pinned buffer and decoded (device.tfrecord_decode) straight into its rows and its columns of them -- the
  concatenations of select_streams and Dataset.device_arrays are the kernel's stores -- and the statuses of all files
  are fetched with one wait.  A file without a plan, or whose skeleton check failed, is read by
  read_file(verify=True) on the host and uploaded into its rows.  Preprocessed fields are decoded into tensors of
  their own, processed file by file as device tensors and placed on the device.  `files` are row slices of one host
  copy of each stream; cache = (handle, x, x2, y, offsets) is what Dataset.device_arrays would have uploaded."""
  import torch
  from telluride_decoding_amd import device as dev
  h = handle
  in1 = [in1_fields] if isinstance(in1_fields, str) else list(in1_fields)
  in2 = [] if not in2_fields else ([in2_fields] if isinstance(in2_fields, str) else list(in2_fields))
  for field in preprocessors:
    if field not in wanted:
      raise ValueError('Could not find preprocess field %s in data (%s)' % (field, sorted(wanted)))

  # what every file holds: a plan, or (irregular) the host's features
  plans, host, rows, widths = [], [], [], None
  for name in names:
    plan = decode_plan(name)
    if plan is not None and wanted - {k for k, _, _ in plan['layout']}:
      plan = None                                   # (read_file words the missing-feature error)
    feats = None if plan is not None else read_file(name, wanted, verify=True)
    w = ({k: c for k, _, c in plan['layout'] if k in wanted} if plan is not None
         else {k: v.shape[1] for k, v in feats.items()})
    if widths is None:
      widths = w
    elif w != widths:
      raise ValueError('%s: feature widths %s differ from those of %s: %s' % (name, w, names[0], widths))
    plans.append(plan); host.append(feats)
    rows.append(plan['frames'] if plan is not None else next(iter(feats.values())).shape[0])
  offs = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
  total = int(offs[-1])

  # streams 0 .. 3 = input_1, input_2, output, attention.  A stream without a preprocessed field is decoded into
  # directly: (field, tensor, column) per place.  The fields of a stream with one are decoded into tensors of their
  # own (`own`) and the stream is put together on the device once the preprocessors have run, because a
  # preprocessor may change the width of its field.
  stream_fields = [in1, in2, [] if out_field == 'ones' else [out_field], [attended_field] if attended_field else []]
  composed = [any(k in preprocessors for k in fields) for fields in stream_fields]
  with torch.cuda.stream(h._stream):
    streams, targets = [None] * 4, []
    for s, fields in enumerate(stream_fields):
      if composed[s]:
        continue
      streams[s] = h.empty((total, sum(widths[k] for k in fields) if fields else 1), 'float32')
      col = 0
      for k in fields:
        targets.append((k, streams[s], col))
        col += widths[k]
    own = {k: h.empty((total, widths[k]), 'float32') for s in range(4) if composed[s] for k in stream_fields[s]}
    targets += [(k, t, 0) for k, t in own.items()]
    if out_field == 'ones':
      streams[2].fill_(1.0)
    if not attended_field:
      streams[3].zero_()

    def upload_host(i, feats):
      r0, r1 = int(offs[i]), int(offs[i + 1])
      for k in {k for k, _, _ in targets}:
        if feats[k].shape != (r1 - r0, widths[k]):
          raise ValueError('%s: feature %s is %s, not the %s its first record promises' %
                           (names[i], k, feats[k].shape, (r1 - r0, widths[k])))
      for k, dst, col in targets:
        dst[r0:r1, col:col + widths[k]].copy_(torch.from_numpy(np.ascontiguousarray(feats[k], np.float32)))

    chunks = [targets[c:c + dev.TFRECORD_MAX_OUTPUTS] for c in range(0, len(targets), dev.TFRECORD_MAX_OUTPUTS)]
    regular = [i for i, plan in enumerate(plans) if plan is not None]
    status = torch.full((max(1, len(regular) * len(chunks)),), -1, dtype=torch.int64, device=h.device)
    biggest = max([plans[i]['frames'] * plans[i]['stride'] for i in regular] or [0])
    image = h.empty((biggest,), 'uint8') if regular else None
    pinned = [None, None]                           # two host buffers: the next file is read while one is copied up
    copied = [None, None]
    for n, i in enumerate(regular):
      plan, b = plans[i], n & 1
      if copied[b] is not None:
        copied[b].synchronize()
      if pinned[b] is None:
        pinned[b] = torch.empty(biggest, dtype=torch.uint8, pin_memory=True)
      image, pinned[b], copied[b] = _upload_image(names[i], plan['frames'] * plan['stride'], h, pinned[b], image)
      for c, chunk in enumerate(chunks):
        slot = n * len(chunks) + c
        dev.tfrecord_decode(image, plan, [(k, dst, int(offs[i]), col) for k, dst, col in chunk], handle=h,
                            status=status[slot:slot + 1])
    for i, feats in enumerate(host):
      if feats is not None:
        upload_host(i, feats)
    codes = status.cpu().numpy().reshape(-1, len(chunks)) if regular else []        # the one wait for all files
    for n, i in enumerate(regular):
      code = int(codes[n].view(np.uint64).min().astype(np.int64))                    # (-1, all clear, sorts last)
      if code == -1:
        continue
      if code & 3 == 2:
        raise ValueError('%s: corrupt data CRC at byte %d' % (names[i], (code >> 2) * plans[i]['stride']))
      upload_host(i, read_file(names[i], wanted, verify=True))

  # The preprocessors queue on torch's current stream, which need not be the handle's: each stream waits for the
  # other where the work changes hands.
  done = {}
  if preprocessors:
    current = torch.cuda.current_stream(h.device)
    current.wait_stream(h._stream)
    for field, p in preprocessors.items():
      for i in range(len(names)):
        r0, r1 = int(offs[i]), int(offs[i + 1])
        out, _ = p.process_files(own[field][r0:r1], [0, r1 - r0], dtype='float64')
        if int(out.shape[0]) != r1 - r0:
          raise ValueError('%s: the preprocessing of %s changes the number of frames (%d -> %d)' %
                           (names[i], field, r1 - r0, int(out.shape[0])))
        if field not in done:
          done[field] = h.empty((total, int(out.shape[1])), 'float32')
        done[field][r0:r1].copy_(out)                       # (float64 -> float32: as np.asarray(out, np.float32))
    h._stream.wait_stream(current)
  with torch.cuda.stream(h._stream):
    for s, fields in enumerate(stream_fields):
      if composed[s]:
        streams[s] = torch.cat([done.get(k, own[k]) for k in fields], dim=1)
    if not in2:
      streams[1].copy_(streams[0][:, 0:1])
    hosts = [t.cpu().numpy() for t in streams]         # (waits for the handle's stream: `done` may be freed after it)
  files = [tuple(a[int(offs[i]):int(offs[i + 1])] for a in hosts) for i in range(len(names))]
  return files, (h, streams[0], streams[1], streams[2], offs)


def dataset_from_files(filenames, in1_fields, out_field, in2_fields=None, attended_field=None,
                       batch_size=512, pre_context=0, post_context=0, in2_pre_context=0,
                       in2_post_context=0, input_offset=0, preprocess=None, frame_rate=None, device=None):
  """TFRecord files -> brain_data.Dataset (one file = one recording; context never crosses
  files, brain_data.py:722-724).  Files whose name contains '-bad-' are skipped (:677).

  device (opt-in): a device.Handle.  The files are then checked and unpacked on the GPU (_dataset_on_device): the
  same Dataset bit for bit, already resident for device_arrays(device) -- but a file with a damaged record raises
  (a data CRC: iter_records' ValueError), as the reference's tf.data.TFRecordDataset does, where the host route,
  which never looks at a data CRC, reads on.

  preprocess (opt-in): {field: preprocess.Preprocessor or 'name(key=val;...)' string} applied to that
  field of every recording on the GPU before the fields are selected, its state reset at each file
  (Preprocessor.process_files).  A string builds a Preprocessor at frame_rate in and out, as the
  reference's brain_data.preprocess_list does (brain_data.py:766-774).  The steps must leave every field of
  a recording with the same number of frames."""
  from telluride_decoding_amd import brain_data
  wanted = set([in1_fields] if isinstance(in1_fields, str) else in1_fields)
  wanted |= set([] if not in2_fields else ([in2_fields] if isinstance(in2_fields, str) else in2_fields))
  if out_field != 'ones':
    wanted.add(out_field)
  if attended_field:
    wanted.add(attended_field)
  preprocessors = {}
  for field, spec in (preprocess or {}).items():
    if isinstance(spec, str):
      if frame_rate is None:
        raise ValueError('a preprocess string for %s needs frame_rate' % field)
      from telluride_decoding_amd import preprocess as pp
      spec = pp.Preprocessor(spec, frame_rate, frame_rate)
    preprocessors[field] = spec
  if device is not None and any('-bad-' not in name for name in filenames):
    files, cache = _dataset_on_device([name for name in filenames if '-bad-' not in name], in1_fields, out_field,
                                      in2_fields, attended_field, wanted, preprocessors, device)
    ds = brain_data.Dataset(files, batch_size, pre_context=pre_context, post_context=post_context,
                            in2_pre_context=in2_pre_context, in2_post_context=in2_post_context,
                            input_offset=input_offset)
    ds._device_cache = cache          # the first device_arrays(device) uploads nothing
    return ds
  files = []
  for name in filenames:
    if '-bad-' in name:
      continue
    features = read_file(name, fields=wanted)
    for field, p in preprocessors.items():
      if field not in features:
        raise ValueError('Could not find preprocess field %s in data (%s)' % (field, sorted(features)))
      data = features[field]
      out, _ = p.process_files(data, [0, data.shape[0]])
      features[field] = np.asarray(out, np.float32)
    files.append(select_streams(features, in1_fields, out_field, in2_fields, attended_field))
  return brain_data.Dataset(files, batch_size, pre_context=pre_context, post_context=post_context,
                            in2_pre_context=in2_pre_context, in2_post_context=in2_post_context,
                            input_offset=input_offset)
