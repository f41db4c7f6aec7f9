"""Raw recordings for tests/test_cpu_raw_ingest.py, tests/test_gpu_raw_ingest.py and tools/time_raw_ingest.py: a
seeded synthesiser of BrainVision and EDF files, an EDF writer, and NumPy readers of both formats that share no
code with the package (the oracle the device route is compared with, bit for bit)."""
import os
import re

import numpy as np

SPECIAL_F32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff, 0xff7fffff,
                        0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x3f800000], np.uint32)


def float_patterns(rng, count):
  """`count` float32 bit patterns: random bits with +-0, subnormals, the largest finite value, +-inf and NaN mixed
  in (about one in eight)."""
  bits = rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
  special = rng.random(count) < 0.125
  bits[special] = SPECIAL_F32[rng.integers(0, len(SPECIAL_F32), size=int(special.sum()))]
  return bits


def int16_patterns(rng, count):
  values = rng.integers(-32768, 32768, size=count).astype(np.int16)
  if count >= 2:
    values[0], values[-1] = -32768, 32767
  return values


def resolutions(channels):
  """Per-channel factors, none a power of two."""
  return [0.0488281 + 0.0137 * c for c in range(channels)]


def channel_names(channels):
  names = ['E%03d' % c for c in range(channels)]
  if channels >= 2:
    names[-2] = 'TRIG'
  return names


def write_brainvision(directory, stem, samples, factors, binary_format='IEEE_FLOAT_32', orientation='MULTIPLEXED',
                      data_format='BINARY', names=None, interval=2000):
  """Writes <stem>.vhdr and <stem>.eeg.  samples: [frames, channels] uint32 float bit patterns or int16, written
  little-endian frame by frame (MULTIPLEXED) or channel by channel (VECTORIZED).  Returns the header's path."""
  frames, channels = samples.shape
  names = names or channel_names(channels)
  lines = ['Brain Vision Data Exchange Header File Version 1.0', '; written by tests/host_raw.py', '',
           '[Common Infos]', 'Codepage=UTF-8', 'DataFile=%s.eeg' % stem, 'DataFormat=%s' % data_format,
           '; Data orientation', 'DataOrientation=%s' % orientation, 'NumberOfChannels=%d' % channels,
           'SamplingInterval=%d' % interval, '', '[Binary Infos]', 'BinaryFormat=%s' % binary_format, '',
           '[Channel Infos]', '; Ch<n>=<name>,<reference>,<resolution>,<unit>']
  lines += ['Ch%d=%s,,%r,µV' % (c + 1, names[c], factors[c]) for c in range(channels)]
  lines += ['', '[Comment]', 'synthetic', '']
  with open(os.path.join(directory, stem + '.vhdr'), 'w', encoding='utf-8') as f:
    f.write('\n'.join(lines))
  ordered = samples if orientation == 'MULTIPLEXED' else samples.T
  little = '<u4' if samples.dtype == np.uint32 else '<i2'
  with open(os.path.join(directory, stem + '.eeg'), 'wb') as f:
    f.write(np.ascontiguousarray(ordered).astype(little).tobytes())
  return os.path.join(directory, stem + '.vhdr')


def synth_brainvision(directory, stem, channels, frames, binary_format='IEEE_FLOAT_32', orientation='MULTIPLEXED',
                      seed=0):
  """A seeded recording; returns (header path, samples [frames, channels], factors)."""
  rng = np.random.default_rng([seed, channels, frames])
  if binary_format == 'INT_16':
    samples = int16_patterns(rng, frames * channels).reshape(frames, channels)
  else:
    samples = float_patterns(rng, frames * channels).reshape(frames, channels)
  factors = resolutions(channels)
  return write_brainvision(directory, stem, samples, factors, binary_format, orientation), samples, factors


def scaled_channels(samples, factors):
  """The oracle: float32 [channels, frames] = float32(sample) * float32(factor), one float32 multiply each."""
  data = samples.view(np.float32) if samples.dtype == np.uint32 else samples.astype(np.float32)
  with np.errstate(all='ignore'):
    return np.stack([data[:, c] * np.float32(factors[c]) for c in range(data.shape[1])])


def read_brainvision_numpy(header_path):
  """(names, sampling rate, float32 [channels, frames] scaled) of a BrainVision recording, by a reader of its
  own: regular expressions over the header, np.fromfile on the data."""
  with open(header_path, encoding='utf-8') as f:
    text = f.read()
  key = lambda name: re.search(r'^%s=(.*)$' % name, text, re.MULTILINE).group(1).strip()
  channels = int(key('NumberOfChannels'))
  entries = re.findall(r'^Ch(\d+)=([^,\n]*),([^,\n]*),([^,\n]*),?([^,\n]*)$', text, re.MULTILINE)
  entries.sort(key=lambda e: int(e[0]))
  assert len(entries) == channels
  dtype = {'IEEE_FLOAT_32': '<f4', 'INT_16': '<i2'}[key('BinaryFormat')]
  raw = np.fromfile(os.path.join(os.path.dirname(header_path), key('DataFile')), dtype=dtype)
  frames = raw.size // channels
  data = raw.reshape(frames, channels) if key('DataOrientation') == 'MULTIPLEXED' else raw.reshape(channels, frames).T
  data = data.astype(np.float32)
  with np.errstate(all='ignore'):
    scaled = np.stack([data[:, c] * np.float32(float(entries[c][3])) for c in range(channels)])
  return [e[1] for e in entries], 1e6 / float(key('SamplingInterval')), scaled


# ---------------------------------------------------------------- EDF
def _field(value, width):
  text = value if isinstance(value, str) else ('%d' % value if float(value) == int(value) else repr(float(value)))
  assert len(text) <= width, (text, width)
  return text.ljust(width).encode('latin-1')


def write_edf(path, signals, records_field=None, duration=1.0, reserved='', version='0', drop_tail_bytes=0):
  """Writes an EDF file.  signals: [{'label', 'digital' int16 [records, n], 'physical_min', 'physical_max',
  'digital_min', 'digital_max'}] in file order (an 'EDF Annotations' signal too: its 'digital' is its bytes as
  int16).  records_field: what the header says (default: the truth); version '\\xffBIOSEMI' makes a BDF header."""
  records = signals[0]['digital'].shape[0]
  head = _field(version, 8) if isinstance(version, str) else version.ljust(8)
  head += _field('X X X X', 80) + _field('Startdate X X X X', 80) + _field('01.01.01', 8) + _field('00.00.00', 8)
  head += _field(256 * (len(signals) + 1), 8) + _field(reserved, 44)
  head += _field(records if records_field is None else records_field, 8) + _field(duration, 8)
  head += _field(len(signals), 4)
  columns = (('label', 16, None), ('transducer', 80, 'electrode'), ('dimension', 8, 'uV'), ('physical_min', 8, None),
             ('physical_max', 8, None), ('digital_min', 8, None), ('digital_max', 8, None), ('prefilter', 80, 'none'),
             ('n', 8, None), ('reserved', 32, ''))
  for name, width, default in columns:
    for s in signals:
      value = s['digital'].shape[1] if name == 'n' else s.get(name, default)
      head += _field(value, width)
  body = np.concatenate([s['digital'].astype('<i2') for s in signals], axis=1).tobytes()
  if drop_tail_bytes:
    body = body[:-drop_tail_bytes]
  with open(path, 'wb') as f:
    f.write(head + body)
  return path


def synth_edf(path, channels, records, n, seed=0, annotations_at=None, annotation_n=7):
  """A seeded EDF file of `channels` ordinary signals (ranges that differ per signal, none a power of two apart)
  and, at position annotations_at, an 'EDF Annotations' signal of annotation_n samples."""
  rng = np.random.default_rng([seed, channels, records, n])
  signals = []
  for c in range(channels):
    signals.append({'label': 'TRIG' if (channels >= 2 and c == channels - 2) else 'E%03d' % c,
                    'digital': int16_patterns(rng, records * n).reshape(records, n),
                    'physical_min': round(-3276.8 - 1.5 * c, 2), 'physical_max': round(3276.7 + 0.25 * c, 2),
                    'digital_min': -32768, 'digital_max': 32767})
  if annotations_at is not None:
    signals.insert(annotations_at, {'label': 'EDF Annotations', 'digital': int16_patterns(rng, records * annotation_n)
                                    .reshape(records, annotation_n), 'physical_min': -1, 'physical_max': 1,
                                    'digital_min': -32768, 'digital_max': 32767})
  return write_edf(path, signals), signals


def read_edf_numpy(path):
  """(labels, rates, float64 [signals, samples]) of an EDF file's ordinary signals by a reader of its own: fixed
  slices of the header, one strided gather per signal, value = bitvalue * (offset + digital) in float64."""
  with open(path, 'rb') as f:
    blob = f.read()
  count = int(blob[252:256])
  records, duration = int(blob[236:244]), float(blob[244:252])
  starts = np.cumsum([0, 16, 80, 8, 8, 8, 8, 8, 80, 8]) * count + 256
  cell = lambda field, s, width: blob[starts[field] + s * width:starts[field] + (s + 1) * width].decode('latin-1').strip()
  labels = [cell(0, s, 16) for s in range(count)]
  n = [int(cell(8, s, 8)) for s in range(count)]
  per_record = sum(n)
  data = np.frombuffer(blob, '<i2', offset=256 * (count + 1))
  whole = data.size // per_record
  records = whole if records < 0 or records > whole else records
  data = data[:records * per_record].reshape(records, per_record)
  out_labels, values = [], []
  for s in range(count):
    if labels[s] == 'EDF Annotations':
      continue
    pmin, pmax, dmin, dmax = (np.float64(cell(f, s, 8)) for f in (3, 4, 5, 6))
    bitvalue = (pmax - pmin) / (dmax - dmin)
    offset = pmax / bitvalue - dmax
    first = sum(n[:s])
    digital = data[:, first:first + n[s]].reshape(-1).astype(np.float64)
    values.append(bitvalue * (offset + digital))
    out_labels.append(labels[s])
  rates = [n[s] / duration for s in range(count) if labels[s] != 'EDF Annotations']
  return out_labels, rates, np.stack(values)


def same_bits(got, want):
  """Bitwise equality of two float arrays, NaNs compared by position only."""
  got, want = np.asarray(got), np.asarray(want)
  if got.shape != want.shape or got.dtype != want.dtype:
    return False
  nan = np.isnan(want)
  if not np.array_equal(np.isnan(got), nan):
    return False
  as_int = np.uint32 if got.dtype == np.float32 else np.uint64
  return np.array_equal(np.where(nan, 0, got).view(as_int), np.where(nan, 0, want).view(as_int))
