"""BrainVision recordings: drop-in for the reference's ingest_brainvision.py (same names, parameters, defaults,
error types).

A recording is three files: the .vhdr header (text: [sections] of key=value lines), the .vmrk marker file (not
read here) and the binary .eeg data file the header names.

  parse_bv_keywords   one section -> its keys and values
  parse_bv_header     the header text -> {'Common Infos', 'Binary Infos', 'Channel Infos', 'Comment'}
  read_bv_file        (header, float32 [frames, channels]) on the host, unscaled
  BvBrainDataFile     an ingest.BrainDataFile: a channel's values are its samples times its resolution

What differs from the reference:
  * With a GPU (device.gpu_available()) BvBrainDataFile.load_all_data uploads the .eeg file once and one launch
    (device.raw_decode) turns it into a [channels, frames] float32 device matrix, already multiplied by every
    channel's resolution; signal_values(name) is that channel's row, a contiguous 1-D device tensor.  Without one
    the values are NumPy's, the same bits: float32(sample) * float32(resolution).
  * BinaryFormat=INT_16 and DataOrientation=VECTORIZED are read as well (the reference reads multiplexed
    IEEE_FLOAT_32 only).  Any other format or orientation and DataFormat=ASCII are the reference's ValueError,
    and so is a data file that is not a whole number of frames.
  * The header is read as UTF-8 (the units are 'µV') from the local file system; tf.io.gfile is not used.
"""
import collections
import os
import re

import numpy as np

from telluride_decoding_amd import device
from telluride_decoding_amd import ingest

_SAMPLE_TYPES = {'IEEE_FLOAT_32': '<f4', 'INT_16': '<i2'}
_ORIENTATIONS = ('MULTIPLEXED', 'VECTORIZED')


def _number_or_text(text):
  if text.isdigit():
    return int(text)
  try:
    return float(text)
  except ValueError:
    return text


def parse_bv_keywords(section):
  """The key=value lines of one section (its text from the section name on) as an ordered dictionary.  Lines that
  start with ';' are comments; a value that reads as a number becomes an int or a float."""
  body = section.split(']', 1)[1]
  found = collections.OrderedDict()
  for line in body.split('\n'):
    if not line or line[0] == ';' or '=' not in line:
      continue
    key, value = line.split('=', 1)
    found[key.strip()] = _number_or_text(value.strip())
  return found


def parse_bv_header(hdr):
  """{section name: contents} of a .vhdr text.  'Common Infos' and 'Binary Infos' are keyword dictionaries,
  'Channel Infos' maps Ch<n> to {'channel_name', 'reference_channel_name', 'resolution', 'unit'} (a TypeError when
  an entry is not text), 'Comment' is the section's lines."""
  sections = {}
  for text in re.split(r'^\[', hdr, flags=re.MULTILINE):
    if text.startswith('Common Infos'):
      sections['Common Infos'] = parse_bv_keywords(text)
    elif text.startswith('Binary Infos'):
      sections['Binary Infos'] = parse_bv_keywords(text)
    elif text.startswith('Channel Infos'):
      channels = parse_bv_keywords(text)
      for key, entry in channels.items():
        if not isinstance(entry, str):
          raise TypeError('Expected a string of key-vals, not a %s.' % type(entry))
        name, reference, resolution, unit = entry.split(',')
        channels[key] = {'channel_name': name, 'reference_channel_name': reference,
                         'resolution': float(resolution), 'unit': unit}
      sections['Channel Infos'] = channels
    elif text.startswith('Comment'):
      sections['Comment'] = text.split(']', 1)[1].split('\n')
  return sections


def _read_header(header_filename):
  """(header, data file name, sample dtype, orientation) of a .vhdr file; the ValueErrors for what is not read."""
  if not header_filename.endswith('.vhdr'):
    header_filename += '.vhdr'
  with open(header_filename, 'r', encoding='utf-8') as fp:
    header = parse_bv_header(fp.read())
  common, binary = header['Common Infos'], header['Binary Infos']
  data_filename = common['DataFile']
  if '$b' in data_filename:
    data_filename = data_filename.replace('$b', header_filename.rsplit('.', 1)[0])
  if '/' in header_filename and '/' not in data_filename:       # (the header only knows the data file's own name)
    data_filename = os.path.join(os.path.dirname(header_filename), data_filename)
  if common.get('DataFormat', 'BINARY') != 'BINARY':
    raise ValueError('Can\'t read BrainVision data that has format %s' % common['DataFormat'])
  if binary['BinaryFormat'] not in _SAMPLE_TYPES:
    raise ValueError('Can\'t read BrainVision data that has format %s' % binary['BinaryFormat'])
  orientation = common.get('DataOrientation', 'MULTIPLEXED')
  if orientation not in _ORIENTATIONS:
    raise ValueError('Can\'t read BrainVision data that has orientation %s' % orientation)
  return header, data_filename, np.dtype(_SAMPLE_TYPES[binary['BinaryFormat']]), orientation


def _frames_of(data_filename, size, channels, sample_bytes):
  if channels < 1 or size % (channels * sample_bytes):
    raise ValueError('%s: %d bytes are not a whole number of frames of %d channels x %d bytes' %
                     (data_filename, size, channels, sample_bytes))
  return size // (channels * sample_bytes)


def read_bv_file(header_filename):
  """(header, data): the header's sections (parse_bv_header) and the recording as float32 [frames, channels], not
  yet multiplied by the channels' resolutions.  `header_filename` may lack its '.vhdr'; the data file is the one
  the header names, beside it.  Little-endian, as every BrainVision recorder writes."""
  header, data_filename, dtype, orientation = _read_header(header_filename)
  with open(data_filename, 'rb') as f:
    raw = f.read()
  channels = header['Common Infos']['NumberOfChannels']
  frames = _frames_of(data_filename, len(raw), channels, dtype.itemsize)
  data = np.frombuffer(raw, dtype=dtype)
  data = data.reshape(frames, channels) if orientation == 'MULTIPLEXED' else data.reshape(channels, frames).T
  return header, data.astype(np.float32, copy=False)


class BvBrainDataFile(ingest.BrainDataFile):
  """The signals of one BrainVision recording, by channel name."""

  def __init__(self, filename, data_type=None, **kwds):
    self._header = {}
    super(BvBrainDataFile, self).__init__(filename, data_type=data_type, **kwds)

  def load_all_data(self, data_dir):
    if not os.path.exists(data_dir):
      raise IOError('Data_dir does not exist:', data_dir)
    data_filename = os.path.join(data_dir, self._data_filename)
    self._scaled = None
    if device.gpu_available():
      self._header, self._scaled = _read_bv_device(data_filename)
    else:
      self._header, self._data = read_bv_file(data_filename)

  @property
  def signal_names(self):
    return [entry['channel_name'] for entry in self._header['Channel Infos'].values()]

  def signal_values(self, name):
    if not isinstance(name, str):
      raise ValueError('Must search for values with a string name.')
    channel_index = self.find_channel_index(name)
    channel_resolution = self.find_channel_resolution(name)
    if channel_index is None:
      return None
    if self._scaled is not None:
      return self._scaled[channel_index]
    return self._data[:, channel_index] * channel_resolution

  def signal_fs(self, name):
    del name
    return 1e6 / float(self._header['Common Infos']['SamplingInterval'])

  def find_channel_index(self, desired_label='TRIG'):
    """The column of the channel with that name, None when there is none."""
    assert 'Channel Infos' in self._header
    for index, entry in enumerate(self._header['Channel Infos'].values()):
      if entry['channel_name'] == desired_label:
        return index
    return None

  def find_channel_resolution(self, desired_label='TRIG'):
    """The resolution (units per count) of the channel with that name, None when there is none."""
    assert 'Channel Infos' in self._header
    for entry in self._header['Channel Infos'].values():
      if entry['channel_name'] == desired_label:
        return entry['resolution']
    return None


def _read_bv_device(header_filename):
  """(header, float32 device [channels, frames]): the data file uploaded once and decoded, transposed and scaled by
  one device.raw_decode launch.  Column c of the file is the c-th entry of 'Channel Infos', as on the host."""
  import torch
  from telluride_decoding_amd import tfrecord
  header, data_filename, dtype, orientation = _read_header(header_filename)
  channels = header['Common Infos']['NumberOfChannels']
  w = dtype.itemsize
  size = os.path.getsize(data_filename)
  frames = _frames_of(data_filename, size, channels, w)
  resolutions = [entry['resolution'] for entry in header['Channel Infos'].values()]
  resolutions = (resolutions + [1.0] * channels)[:channels]     # (channels the header does not describe: counts)
  h = device.default_handle()
  if frames == 0:
    return header, h.empty((channels, 0), 'float32')
  kind = device.RAW_FLOAT32 if w == 4 else device.RAW_INT16
  with torch.cuda.stream(h._stream):
    image, _, _ = tfrecord._upload_image(data_filename, size, h)
    if orientation == 'MULTIPLEXED':
      records, record_bytes, n, offsets = frames, channels * w, 1, [c * w for c in range(channels)]
    else:
      records, record_bytes, n, offsets = 1, size, frames, [c * frames * w for c in range(channels)]
    scaled = device.raw_decode(image, 0, records, record_bytes, n, kind, offsets, resolutions, handle=h)
  return header, scaled
