"""BioSemi BDF recordings for tests/test_cpu_bdf.py, tests/test_gpu_bdf.py and tools/time_raw_ingest.py: a BDF
writer, a seeded synthesiser, and a NumPy reader that shares no code with the package (fixed slices of the header,
np.frombuffer(..., np.uint8) on the data): the oracle both routes are compared with, bit for bit."""
import numpy as np

STATUS = 'Status'
ANNOTATIONS = ('BDF Annotations', 'EDF Annotations')
EDGES_24 = np.array([0x7fffff, -0x800000, -1, 0, 1, -2, 0x800000 - 2, 0x123456], np.int32)   # (as signed numbers)


def int24_patterns(rng, count):
  """`count` signed 24-bit numbers as int32: random, with the bit patterns 0x7fffff, 0x800000, 0xffffff first."""
  values = rng.integers(-0x800000, 0x800000, size=count).astype(np.int32)
  values[:min(count, len(EDGES_24))] = EDGES_24[:count]
  return values


def pack24(values):
  """int32 [...] -> the little-endian 24-bit two's-complement bytes, uint8 [..., 3]."""
  u = np.asarray(values).astype(np.int64) & 0xffffff
  return np.stack([u & 0xff, (u >> 8) & 0xff, (u >> 16) & 0xff], axis=-1).astype(np.uint8)


def _field(value, width):
  text = value if isinstance(value, str) else ('%d' % value if float(value) == int(value) else repr(float(value)))
  assert len(text) <= width, (text, width)
  return text.ljust(width).encode('latin-1')


def write_bdf(path, signals, records_field=None, duration=1.0, reserved='24BIT', version=b'\xffBIOSEMI',
              extra_tail=b'', drop_tail_bytes=0):
  """Writes a BDF file.  signals: [{'label', 'digital' int32 [records, n] within 24 bits, 'physical_min',
  'physical_max', 'digital_min', 'digital_max'}] in file order (an annotations signal too: its 'digital' is its
  bytes, three to a number).  records_field: what the header says (default: the truth); version '0' makes an EDF
  header in front of the same data; extra_tail: bytes after the last record (part of a record that was cut off)."""
  records = signals[0]['digital'].shape[0]
  head = version.ljust(8) if isinstance(version, bytes) else _field(version, 8)
  head += _field('X X X X', 80) + _field('Startdate X X X X', 80) + _field('01.01.01', 8) + _field('00.00.00', 8)
  head += _field(256 * (len(signals) + 1), 8) + _field(reserved, 44)
  head += _field(records if records_field is None else records_field, 8) + _field(duration, 8)
  head += _field(len(signals), 4)
  columns = (('label', 16, None), ('transducer', 80, 'Active Electrode'), ('dimension', 8, 'uV'),
             ('physical_min', 8, None), ('physical_max', 8, None), ('digital_min', 8, None), ('digital_max', 8, None),
             ('prefilter', 80, 'HP: DC; LP: 417 Hz'), ('n', 8, None), ('reserved', 32, ''))
  for name, width, default in columns:
    for s in signals:
      head += _field(s['digital'].shape[1] if name == 'n' else s.get(name, default), width)
  body = np.concatenate([pack24(s['digital']).reshape(records, -1) for s in signals], axis=1).tobytes()
  if drop_tail_bytes:
    body = body[:-drop_tail_bytes]
  with open(path, 'wb') as f:
    f.write(head + body + extra_tail)
  return path


def status_codes(rng, count, every=37):
  """A Status channel as BioSemi writes it: a 16-bit trigger code that changes every `every` samples or so (back to
  0 now and then), under status bits 16 .. 23 that are set throughout (bit 23 makes every number negative)."""
  steps = rng.integers(0, 4, size=count // every + 2)
  codes = np.where(steps == 0, 0, rng.integers(1, 1 << 16, size=steps.size))
  low = np.repeat(codes, every)[:count].astype(np.int64)
  value = low | 0xd10000
  return (value - ((value & 0x800000) << 1)).astype(np.int32)


def synth_bdf(path, channels, records, n, seed=0, annotations_at=None, annotation_n=7, status=True, **kwds):
  """A seeded BDF file of `channels` ordinary signals 'A001' ... (ranges that differ per signal, none a power of two
  apart), then a 'Status' signal whose header ranges are not trivial, and at position annotations_at a
  'BDF Annotations' signal of annotation_n samples.  Returns (path, signals)."""
  rng = np.random.default_rng([seed, channels, records, n])
  signals = []
  for c in range(channels):
    signals.append({'label': 'A%03d' % (c + 1), 'digital': int24_patterns(rng, records * n).reshape(records, n),
                    'physical_min': -262144 - 3 * c, 'physical_max': 262143 + 5 * c,
                    'digital_min': -8388608, 'digital_max': 8388607})
  if status:
    signals.append({'label': STATUS, 'digital': status_codes(rng, records * n).reshape(records, n),
                    'physical_min': -262144, 'physical_max': 262143, 'digital_min': -8388608, 'digital_max': 8388607,
                    'dimension': 'Boolean', 'transducer': 'Triggers and Status'})
  if annotations_at is not None:
    signals.insert(annotations_at, {'label': ANNOTATIONS[0], 'digital': int24_patterns(rng, records * annotation_n)
                                    .reshape(records, annotation_n), 'physical_min': -1, 'physical_max': 1,
                                    'digital_min': -8388608, 'digital_max': 8388607})
  return write_bdf(path, signals, **kwds), signals


def read_bdf_numpy(path):
  """(labels, rates, float64 [signals, samples]) of a BDF file's ordinary signals by a reader of its own: fixed
  slices of the header, the data as uint8, value = bitvalue * (offset + digital) in float64 -- the 'Status' signal
  as stored."""
  with open(path, 'rb') as f:
    blob = f.read()
  assert blob[:8] == b'\xffBIOSEMI'
  count = int(blob[252:256])
  records, duration = int(blob[236:244]), float(blob[244:252])
  starts = np.cumsum([0, 16, 80, 8, 8, 8, 8, 8, 80, 8]) * count + 256
  cell = lambda field, s, width: blob[starts[field] + s * width:starts[field] + (s + 1) * width].decode('latin-1').strip()
  labels = [cell(0, s, 16) for s in range(count)]
  n = [int(cell(8, s, 8)) for s in range(count)]
  record_bytes = 3 * sum(n)
  data = np.frombuffer(blob, np.uint8, offset=256 * (count + 1))
  whole = data.size // record_bytes
  records = whole if records < 0 or records > whole else records
  data = data[:records * record_bytes].reshape(records, record_bytes).astype(np.int64)
  out_labels, rates, values = [], [], []
  for s in range(count):
    if labels[s] in ANNOTATIONS:
      continue
    first = 3 * sum(n[:s])
    run = data[:, first:first + 3 * n[s]].reshape(-1, 3)
    unsigned = run[:, 0] + 256 * run[:, 1] + 65536 * run[:, 2]
    digital = np.where(unsigned >= 1 << 23, unsigned - (1 << 24), unsigned).astype(np.float64)
    if labels[s] == STATUS:
      values.append(digital)
    else:
      pmin, pmax, dmin, dmax = (np.float64(cell(f, s, 8)) for f in (3, 4, 5, 6))
      bitvalue = (pmax - pmin) / (dmax - dmin)
      values.append(bitvalue * ((pmax / bitvalue - dmax) + digital))
    out_labels.append(labels[s])
    rates.append(n[s] / duration)
  return out_labels, rates, np.stack(values)


def code_onsets_numpy(signal, mask):
  """The contract of device.code_onsets / BrainTrial.find_status_trigger_times: (indices int64, codes int32)."""
  code = np.asarray(signal).astype(np.int64) & mask
  prev = np.concatenate(([0], code[:-1]))
  at = np.flatnonzero((code != prev) & (code != 0))
  return at.astype(np.int64), code[at].astype(np.int32)
