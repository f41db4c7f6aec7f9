"""BioSemi BDF recordings: the header parsed here, the 24-bit data records decoded on the GPU.

A BDF file is an EDF file (ingest_edf) with two differences: its first eight bytes are 0xff 'BIOSEMI' instead of a
version number, and every sample is a 24-bit little-endian two's-complement number, so a signal's run in a data
record is 3 * `samples per record` bytes and nothing in the file is aligned to anything.  The physical value of a
stored number is ingest_edf's,

  bitvalue = (physical_max - physical_min) / (digital_max - digital_min)
  offset   = physical_max / bitvalue - digital_max
  value    = bitvalue * (offset + digital)                     all in float64

with one exception: the signal labelled exactly 'Status' holds BioSemi's trigger codes and status bits, not
microvolts, and is served as stored (bitvalue 1, offset 0) whatever its header ranges say; every 24-bit number is
exact in float64.  This NumPy expression, bit for bit on either route, is the module's contract: it is the format as
BioSemi and the EDF specification publish it, and has not been compared with BioSemi's software, pyedflib or MNE.

  read_bdf_header   (main header, per-signal headers, file size)
  parse_bdf_file    the dictionary ingest.EdfBrainDataFile works from, as ingest_edf.parse_edf_file returns it
  BdfBrainDataFile  ingest.EdfBrainDataFile with a load_all_data that reads '<name>.bdf'

With a GPU (device.gpu_available()) the file is uploaded once and one launch (device.raw24_decode) makes the float64
[signals, samples] device matrix; without one the same values are NumPy's.  The events of the 'Status' signal are
BrainTrial.find_status_trigger_times's, which on a device signal copies back the events only.

Read: plain BDF and continuous BDF+ ('BDF+C'); signals labelled 'BDF Annotations' or 'EDF Annotations' are left out.
A ValueError that names the reason: a file that is not BDF (EDF files: ingest_edf), BDF+D (discontinuous), ordinary
signals that differ in samples per record, an empty range, a header that does not hold together.  A record count of
-1 or one larger than the file holds is replaced by the number of whole records in the file.
"""
import os

import numpy as np

from telluride_decoding_amd import device
from telluride_decoding_amd import ingest
from telluride_decoding_amd import ingest_edf

ANNOTATIONS = ('BDF Annotations', ingest_edf.ANNOTATIONS)
STATUS = 'Status'


def read_bdf_header(path):
  """(main header, [per-signal header], file size) of a BDF file, as ingest_edf.read_edf_header gives them for an
  EDF file; 'version' holds the byte 0xff, read as latin-1, in front of 'BIOSEMI'."""
  return ingest_edf._read_header(path, 'BDF')


def _digital(raw):
  """uint8 [..., 3 m] -> int32 [..., m]: little-endian 24-bit two's-complement numbers."""
  b = raw.reshape(raw.shape[:-1] + (-1, 3)).astype(np.int32)
  value = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
  return value - ((value & 0x800000) << 1)


def parse_bdf_file(sample_bdf_file):
  """{'labels', 'signals' float64 [signal, samples], 'sample_rates', 'header', 'signal_headers'} of a BDF file, as
  ingest_edf.parse_edf_file returns them for an EDF file.  'signals' is a device tensor with a GPU and a NumPy array
  without one."""
  path = sample_bdf_file
  main, kept, offsets, n, record_bytes, records, scale, add = ingest_edf._layout(
      path, kind='BDF', width=3, annotations=ANNOTATIONS, unscaled=(STATUS,))
  data_offset = main['header_bytes']
  if device.gpu_available():
    import torch
    from telluride_decoding_amd import tfrecord
    h = device.default_handle()
    if records == 0:
      values = h.empty((len(kept), 0), 'float64')
    else:
      with torch.cuda.stream(h._stream):
        image, _, _ = tfrecord._upload_image(path, data_offset + records * record_bytes, h)
        values = device.raw24_decode(image, data_offset, records, record_bytes, n, offsets, scale, add, handle=h)
  else:
    with open(path, 'rb') as f:
      f.seek(data_offset)
      raw = np.frombuffer(f.read(records * record_bytes), dtype=np.uint8).reshape(records, record_bytes)
    values = np.empty((len(kept), records * n), np.float64)
    for i, off in enumerate(offsets):
      digital = _digital(raw[:, off:off + 3 * n]).reshape(-1).astype(np.float64)
      values[i] = scale[i] * (add[i] + digital)
  return ingest_edf._parsed(main, kept, n, records, values)


class BdfBrainDataFile(ingest.EdfBrainDataFile):
  """ingest.EdfBrainDataFile read by this module's parse_bdf_file: names, values, rates and find_channel_index are
  inherited."""

  def load_all_data(self, data_dir):
    if not os.path.exists(data_dir):
      raise IOError('Data_dir does not exist:', data_dir)
    path = os.path.join(data_dir, self._data_filename)
    if not path.endswith('.bdf'):
      path += '.bdf'
    if not os.path.exists(path):
      raise IOError('Can not open %s for reading' % path)
    self._edf_dict = parse_bdf_file(path)
