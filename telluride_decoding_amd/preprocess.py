"""Drop-in for the reference's preprocess.Preprocessor (preprocess.py:54-587): high-pass and low-pass
Butterworth filtering, nearest-neighbour resampling, re-referencing, channel selection, normalisation and
temporal context, in the reference's order, on the MI355X.

The arithmetic runs in libtd_hotpath.so (csrc/preprocess.hip): the two filters as ONE cascade of
second-order sections (float64, state carried on the device between calls) with the resample fused into
its store, re-referencing + selection in one pass, normalisation + context in one pass.  The filters are
designed on the host by telluride_decoding_amd.iir (NumPy; no scipy at run time).

Return types follow the reference: a NumPy (or list) input gives a float64 NumPy array.  A torch tensor
on the GPU stays there: process() returns a device tensor (float32 by default, `device_dtype`), the route
into the fits without a host round trip.

AudioFeatures (preprocess.py:589-755): the intensity envelope and the spectrogram of
audio, on the device (csrc/audio.hip); its quirks and its one difference are in its docstring.

Differences of the Preprocessor from the reference:
  - The caller's array is never written: the reference's reref_data subtracts in place into its input
    when no filter ran before it (preprocess.py:428).
  - A name with parameters, 'eeg(highpass_cutoff=1;highpass_order=2;channel_numbers=0-31)', names the
    stream 'eeg' and its parameters take effect (they override the keyword arguments).  The reference's
    constructor parses them and then overwrites them with its keyword defaults (preprocess.py:102-107).
  - A streaming resample whose previous batch did not end on an output frame raises before anything
    runs; the reference has advanced its filter states by then (preprocess.py:572-574).
  - The properties of a disabled filter read 0 (and its order); the reference raises AttributeError.
"""
import re

import numpy as np

from telluride_decoding_amd import device, iir


def _torch():
  import torch
  return torch


def _is_device_tensor(data):
  try:
    torch = _torch()
  except ImportError:
    return False
  return isinstance(data, torch.Tensor) and data.is_cuda


def parse_channel_numbers(spec):
  """'0-3,7' -> [0, 1, 2, 3, 7] (inclusive ranges, sorted, unique: preprocess.py:153-175)."""
  pieces = spec.split(',') if ',' in spec else [spec]

  def expand(piece):
    if '-' in piece:
      ends = piece.split('-')
      assert len(ends) == 2
      return list(range(int(ends[0]), int(ends[1]) + 1))
    return [int(piece)]

  return np.unique(np.concatenate([expand(p) for p in pieces])).tolist()


def parse_name_params(param_string):
  """'name(key=val;key=val)' -> (name, {key: int | float | str}) (preprocess.py:563-582)."""
  pieces = re.compile(r'(\w*)\((.*)\)$').match(param_string)
  if not pieces:
    raise ValueError('preprocess parameter string %r is not of the form name(key=val;...)' % param_string)
  params = {}
  for param in pieces.group(2).split(';'):
    if '=' not in param:
      raise ValueError('preprocess param %s missing a value.' % param)
    k, v = param.split('=', 1)
    if v.isdigit():
      v = int(v)
    else:
      try:
        v = float(v)
      except ValueError:
        pass
    params[k] = v
  if isinstance(params.get('channel_numbers'), (int, float)):    # 'channel_numbers=5': one channel
    params['channel_numbers'] = str(int(params['channel_numbers']))
  return pieces.group(1), params


def resample_indices(frames_in, fs_in, fs_out):
  """(input row of every output frame, frames the next batch should skip): the reference's own float64
  products in its order (preprocess.py:376-390), so the indices are bit-exact."""
  len_data = float(frames_in) / fs_in
  frames_out = int(np.round(len_data * fs_out))
  delta_out = 1.0 / fs_out
  next_frame_idx = int(np.round(frames_out * delta_out * fs_in)) - frames_in
  idx_out = np.round(np.arange(frames_out) * delta_out * fs_in)
  idx = np.minimum(frames_in - 1, idx_out).astype(np.int64)
  return idx, next_frame_idx


_PARAM_KEYS = ('fs_in', 'fs_out', 'highpass_cutoff', 'highpass_order', 'lowpass_cutoff', 'lowpass_order',
               'ref_channels', 'channels_to_ref', 'channel_numbers', 'data_mean', 'data_std', 'pre_context',
               'post_context')


class Preprocessor(object):
  """Routines to implement data preprocessing (the reference's class, same constructor and defaults).

  Steps, each optional, in this order: high-pass filter, low-pass filter (added automatically at 0.75 x the
  output Nyquist, order 10, when downsampling without a usable cutoff), resampling, re-referencing, channel
  selection, normalisation, temporal context.  Enter 0 or None to disable a step.
  """
  device_dtype = 'float32'     # what process() returns for a device tensor ('float32' or 'float64')

  def __init__(self,
               name,
               fs_in,
               fs_out,
               highpass_cutoff=0,
               highpass_order=4,
               lowpass_cutoff=0,
               lowpass_order=4,
               ref_channels=None,
               channels_to_ref=None,
               channel_numbers=None,
               data_mean=0,
               data_std=1,
               pre_context=0,
               post_context=0):
    """Specifies desired parameters up front.  Enter 0 or None to disable."""
    values = dict(fs_in=fs_in, fs_out=fs_out, highpass_cutoff=highpass_cutoff, highpass_order=highpass_order,
                  lowpass_cutoff=lowpass_cutoff, lowpass_order=lowpass_order, ref_channels=ref_channels,
                  channels_to_ref=channels_to_ref, channel_numbers=channel_numbers, data_mean=data_mean,
                  data_std=data_std, pre_context=pre_context, post_context=post_context)
    if isinstance(name, str) and '(' in name:
      name, params = parse_name_params(name)
      unknown = set(params) - set(_PARAM_KEYS)
      if unknown:
        raise ValueError('Unknown preprocess parameters %s' % sorted(unknown))
      values.update(params)
    self.check_params(name, values['fs_in'], values['fs_out'], values['highpass_cutoff'],
                      values['highpass_order'], values['lowpass_cutoff'], values['lowpass_order'],
                      values['ref_channels'], values['channels_to_ref'], values['channel_numbers'],
                      values['data_std'], values['pre_context'], values['post_context'])
    self._name = name
    self._fs_in = values['fs_in']
    self._fs_out = values['fs_out']
    self._highpass_sos = self._lowpass_sos = None
    self.init_highpass(values['highpass_cutoff'], values['highpass_order'])
    self.init_lowpass(values['lowpass_cutoff'], values['lowpass_order'])
    self._ref_channels = values['ref_channels']
    self._channels_to_ref = values['channels_to_ref']
    self.init_channel_numbers(values['channel_numbers'])
    self._data_mean = values['data_mean']
    self._data_std = values['data_std']
    self._pre_context = values['pre_context']
    self._post_context = values['post_context']
    self._filter_state = None          # [S_hp + S_lp, 2, C] float64 on the device (scipy's zi layout)
    self._hp_ready = self._lp_ready = False
    self.context_reset()
    self._next_frame_idx = 0

  # ---------------------------------------------------------------- set-up
  def init_highpass(self, highpass_cutoff, highpass_order):
    """Initializes the high-pass filter coefficients."""
    self._highpass_cutoff = highpass_cutoff
    self._highpass_order = highpass_order
    if highpass_cutoff > 0:
      self._highpass_sos = iir.butter_sos(highpass_order, highpass_cutoff, 'hp', self.fs_in)
      self._highpass_zi = iir.sosfilt_zi(self._highpass_sos)
    else:
      self._highpass_sos = self._highpass_zi = None
    self._filter_state = None
    self._hp_ready = self._lp_ready = False

  def init_lowpass(self, lowpass_cutoff, lowpass_order):
    """Initializes the low-pass filter coefficients (with the anti-aliasing default when downsampling)."""
    if lowpass_cutoff > 0 or self._fs_out < self._fs_in:
      nyquist = self._fs_out / 2
      if lowpass_cutoff > nyquist or (self._fs_out < self._fs_in and lowpass_cutoff == 0):
        lowpass_cutoff = 0.75 * nyquist
        lowpass_order = 10
        print('Using %gHz low-pass filter to prevent aliasing' % lowpass_cutoff)
      self._lowpass_sos = iir.butter_sos(lowpass_order, lowpass_cutoff, 'lp', self.fs_in)
      self._lowpass_zi = iir.sosfilt_zi(self._lowpass_sos)
    else:
      self._lowpass_sos = self._lowpass_zi = None
    self._lowpass_cutoff = lowpass_cutoff
    self._lowpass_order = lowpass_order
    self._filter_state = None
    self._hp_ready = self._lp_ready = False

  def init_channel_numbers(self, channel_numbers):
    """Parses the channel specification (an int, a list, or a string like '0-3,7')."""
    if isinstance(channel_numbers, int):
      self._channel_numbers = [channel_numbers]
    elif isinstance(channel_numbers, list):
      self._channel_numbers = channel_numbers
    elif isinstance(channel_numbers, str):
      self._channel_numbers = parse_channel_numbers(channel_numbers)
    else:
      self._channel_numbers = None

  @property
  def name(self):
    return self._name

  @property
  def fs_in(self):
    return self._fs_in

  @property
  def fs_out(self):
    return self._fs_out

  @property
  def highpass_cutoff(self):
    return self._highpass_cutoff

  @property
  def highpass_order(self):
    return self._highpass_order

  @property
  def lowpass_cutoff(self):
    return self._lowpass_cutoff

  @property
  def lowpass_order(self):
    return self._lowpass_order

  @property
  def ref_channels(self):
    return self._ref_channels

  @property
  def channels_to_ref(self):
    return self._channels_to_ref

  @property
  def channel_numbers(self):
    return self._channel_numbers

  @property
  def data_mean(self):
    return self._data_mean

  @property
  def data_std(self):
    return self._data_std

  @property
  def pre_context(self):
    return self._pre_context

  @property
  def post_context(self):
    return self._post_context

  @property
  def sos(self):
    """The cascade the device runs: high-pass sections, then low-pass ones ([S, 6] float64, or None)."""
    parts = [s for s in (self._highpass_sos, self._lowpass_sos) if s is not None]
    return np.concatenate(parts) if parts else None

  @property
  def filter_state(self):
    """The carried filter state [S, 2, C] (float64 device tensor; None before the first call)."""
    return self._filter_state

  def __repr__(self):
    return ('Preprocessor(name={}, fs_in={}, fs_out={}, highpass_cutoff={}, highpass_order={}, '
            'lowpass_cutoff={}, lowpass_order={}, ref_channels={}, channels_to_ref={}, channel_numbers={} '
            'data_mean={}, data_std={}, pre_context={}, post_context={})').format(
                self.name, self.fs_in, self.fs_out, self.highpass_cutoff, self.highpass_order,
                self.lowpass_cutoff, self.lowpass_order, self._ref_channels, self.channels_to_ref,
                self.channel_numbers, self.data_mean, self.data_std, self.pre_context, self.post_context)

  def check_params(self, name, fs_in, fs_out, highpass_cutoff, highpass_order, lowpass_cutoff, lowpass_order,
                   ref_channels, channels_to_ref, channel_numbers, data_std, pre_context, post_context):
    """Checks correctness of parameters passed as input (the reference's errors, preprocess.py:248-281)."""
    if not isinstance(name, str):
      raise TypeError('name must be a string, not %s' % name)
    if fs_in <= 0:
      raise ValueError('fs_in should not be less than 0.')
    if fs_out <= 0:
      raise ValueError('fs_out should not be less than 0.')
    if highpass_cutoff < 0:
      raise ValueError('highpass_cutoff should not be less than 0.')
    if highpass_order < 0:
      raise ValueError('highpass_order should not be less than 0.')
    if lowpass_cutoff < 0:
      raise ValueError('lowpass_cutoff should not be less than 0.')
    if lowpass_order < 0:
      raise ValueError('lowpass_order should not be less than 0.')
    if not isinstance(ref_channels, list) and ref_channels is not None:
      raise ValueError('ref_channels must be a list.')
    if not isinstance(channels_to_ref, list) and channels_to_ref is not None:
      raise ValueError('channels_to_ref must be a list.')
    if not isinstance(channel_numbers, (list, str)) and channel_numbers is not None:
      raise ValueError('channel_numbers must be a list.')
    if data_std <= 0:          # (None: TypeError, as the reference -- data_std=None cannot be used)
      raise ValueError('data_std must be greater than 0.')
    if pre_context < 0:
      raise ValueError('pre_context should not be less than 0.')
    if post_context < 0:
      raise ValueError('post_context should not be less than 0.')

  def check_dims(self, data):
    """Checks that the data is two dimensional."""
    if len(data.shape) != 2:
      raise ValueError('Input data must be a two dimensional array. Data received has shape %s.'
                       % (tuple(data.shape),))

  def init_from_string(self, fs_in, param_string):
    """(Re)initialises from 'name(key=val;...)': the name and every parameter the string gives."""
    if '(' not in param_string:
      self.__init__(param_string, fs_in, self._fs_out)
      return
    name, params = parse_name_params(param_string)
    kwargs = dict(fs_out=self._fs_out, highpass_cutoff=self._highpass_cutoff,
                  highpass_order=self._highpass_order, lowpass_cutoff=self._lowpass_cutoff,
                  lowpass_order=self._lowpass_order, ref_channels=self._ref_channels,
                  channels_to_ref=self._channels_to_ref, channel_numbers=self._channel_numbers,
                  data_mean=self._data_mean, data_std=self._data_std, pre_context=self._pre_context,
                  post_context=self._post_context)
    kwargs.update(params)
    kwargs['fs_in'] = params.get('fs_in', fs_in)
    self.__init__(name, **kwargs)

  # ---------------------------------------------------------------- plumbing
  @staticmethod
  def _to_device(data):
    """(device tensor float32 / float64, was it a device tensor)"""
    if _is_device_tensor(data):
      t = data if data.dtype in (_torch().float32, _torch().float64) else data.to(_torch().float32)
      return t.contiguous(), True
    arr = np.asarray(data)
    if arr.dtype not in (np.float32, np.float64):
      arr = arr.astype(np.float64)
    h = device.default_handle()
    return _torch().from_numpy(np.ascontiguousarray(arr)).to(h.device), False

  @staticmethod
  def _back(t, on_device):
    return t if on_device else t.cpu().numpy().astype(np.float64, copy=False)

  def _state_for(self, c):
    s = self.sos
    if self._filter_state is None or self._filter_state.shape[2] != c:
      h = device.default_handle()
      self._filter_state = h.zeros((s.shape[0], 2, c), 'float64')
      self._hp_ready = self._lp_ready = False
    return self._filter_state

  def _n_hp(self):
    return 0 if self._highpass_sos is None else self._highpass_sos.shape[0]

  def _filter_stage(self, x, which, reset, file_offsets=None, rows=None, out_offsets=None):
    """One stage (or both: which = 'both') of the cascade on the device."""
    n_hp = self._n_hp()
    state = self._state_for(int(x.shape[1]))
    if which == 'hp':
      sos, zi, st, split = self._highpass_sos, self._highpass_zi, state[:n_hp], n_hp
    elif which == 'lp':
      sos, zi, st, split = self._lowpass_sos, self._lowpass_zi, state[n_hp:], self._lowpass_sos.shape[0]
    else:
      sos = self.sos
      zi = np.concatenate([z for z in (self._highpass_zi, self._lowpass_zi) if z is not None])
      st, split = state, n_hp if self._lowpass_sos is not None else sos.shape[0]
    if file_offsets is None:
      file_offsets = [0, int(x.shape[0])]
    y = device.sos_filter(x, file_offsets, sos, zi, split, st, reset, out_rows=rows, out_offsets=out_offsets)
    if which in ('hp', 'both') and self._highpass_sos is not None:
      self._hp_ready = True
    if which in ('lp', 'both') and self._lowpass_sos is not None:
      self._lp_ready = True
    return y

  # ---------------------------------------------------------------- the steps
  def highpass_filter_reset(self, data):
    """Resets the high-pass state to sosfilt_zi x the first row of data."""
    if self._highpass_sos is not None:
      x, _ = self._to_device(data[:1])
      self._filter_stage(x, 'hp', True)

  def highpass_filter(self, data, reset=False):
    """High-pass filters the data along each channel (float64)."""
    if self._highpass_sos is None:
      return data
    x, on_dev = self._to_device(data)
    self.check_dims(x)
    return self._back(self._filter_stage(x, 'hp', reset or not self._hp_ready), on_dev)

  def lowpass_filter_reset(self, data):
    """Resets the low-pass state to sosfilt_zi x the first row of data."""
    if self._lowpass_sos is not None:
      x, _ = self._to_device(data[:1])
      self._filter_stage(x, 'lp', True)

  def lowpass_filter(self, data, reset=False):
    """Low-pass filters the data along each channel (float64)."""
    if self._lowpass_sos is None:
      return data
    x, on_dev = self._to_device(data)
    self.check_dims(x)
    return self._back(self._filter_stage(x, 'lp', reset or not self._lp_ready), on_dev)

  def _resample_plan(self, frames_in):
    """Output rows of this batch (None: no resampling); raises on a misaligned streaming batch."""
    if self._fs_out == self._fs_in:
      return None, 0
    if self._next_frame_idx != 0:
      raise ValueError('New sample rate incompatable with batch size.')
    return resample_indices(frames_in, self._fs_in, self._fs_out)

  def resample(self, data):
    """Nearest-neighbour resampling by a (possibly non-integer) factor (preprocess.py:354-396)."""
    if self._fs_out == self._fs_in:
      return data
    x, on_dev = self._to_device(data)
    idx, nxt = self._resample_plan(int(x.shape[0]))
    self._next_frame_idx = nxt
    rows = _torch().from_numpy(idx).to(x.device)
    return self._back(device.reref_select(x, rows=rows), on_dev)

  def _groups(self, c):
    if self._ref_channels is None and self._channels_to_ref is None:
      return []
    if self._ref_channels is None:       # re-reference to the global average (the reference keeps this)
      self._ref_channels = [range(c)]
    if self._channels_to_ref is None:
      self._channels_to_ref = [range(c)]
    return [(list(r), list(ch)) for r, ch in zip(self._ref_channels, self._channels_to_ref)]

  def reref_data(self, data):
    """Re-references channel groups to the mean of their reference channels (means of the data before any
    group is subtracted).  The input is not modified."""
    x, on_dev = self._to_device(data)
    groups = self._groups(int(x.shape[1]))
    if not groups:
      return data
    return self._back(device.reref_select(x, groups=groups), on_dev)

  def select_channels(self, data):
    """Retains the desired channels."""
    if not self._channel_numbers:
      return data
    x, on_dev = self._to_device(data)
    return self._back(device.reref_select(x, select=self._channel_numbers), on_dev)

  def find_mean_std(self, data):
    """Freezes the mean of the data (over all frames and channels) if data_mean is None."""
    if self._data_std is None:
      raise TypeError('data_std=None is not supported (the reference rejects it in check_params)')
    if self._data_mean is None:
      z, _ = self._to_device(data)
      if z.dtype != _torch().float64:
        z = z.to(_torch().float64)
      self._data_mean = float(device.mean_f64(z).item())

  def normalize_data(self, data):
    """(data - mean) / std."""
    self.find_mean_std(data)
    z, on_dev = self._to_device(data)
    if z.dtype != _torch().float64:
      z = z.to(_torch().float64)
    out, _ = device.context_out(z, None, 0, 0, self._data_mean, self._data_std, dtype='float64')
    return self._back(out, on_dev)

  def shift(self, arr, shift_amt, pre_context, post_context):
    """Rows [pre - shift, N - post - shift) of arr (the reference's helper of add_context)."""
    return arr[pre_context - shift_amt:arr.shape[0] - post_context - shift_amt, :]

  def _context(self, z, mean, std, dtype):
    pre, post = self._pre_context, self._post_context
    if pre == 0 and post == 0:
      out, _ = device.context_out(z, None, 0, 0, mean, std, dtype=dtype)
      return out
    if self._context_state is None:
      self._context_state = device.default_handle().zeros((pre, int(z.shape[1])), 'float64')
    out, self._context_state = device.context_out(z, self._context_state, pre, post, mean, std, dtype=dtype)
    return out

  def add_context(self, data):
    """Pre and post temporal context: block b of output row r is row r + b of [carried rows ; data]; the
    last pre + post rows carry into the next call (the first call returns N - post rows)."""
    if self._pre_context == 0 and self._post_context == 0:
      return data
    z, on_dev = self._to_device(data)
    if z.dtype != _torch().float64:
      z = z.to(_torch().float64)
    return self._back(self._context(z, 0.0, 1.0, 'float64'), on_dev)

  def context_reset(self):
    """Resets the saved state of the context."""
    self._context_state = None

  # ---------------------------------------------------------------- the whole chain
  def _run(self, x, file_offsets, reset, dtype):
    """Every step over the files of x (device tensor); returns (output, output file offsets)."""
    offs = [int(v) for v in file_offsets]
    many = len(offs) > 2
    plans = [self._resample_plan(offs[f + 1] - offs[f]) if not many or self._fs_out == self._fs_in
             else resample_indices(offs[f + 1] - offs[f], self._fs_in, self._fs_out)
             for f in range(len(offs) - 1)]
    rows, out_offs = None, offs
    if plans[0][0] is not None:
      out_offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in plans])]).astype(np.int64).tolist()
      rows = _torch().from_numpy(np.concatenate([p[0] for p in plans])).to(x.device)
    next_idx = plans[-1][1]
    c = int(x.shape[1])
    gather = None
    if self.sos is not None:
      both = self._highpass_sos is not None and self._lowpass_sos is not None
      if not both or self._hp_ready == self._lp_ready:
        y = self._filter_stage(x, 'both', reset or many or not (self._hp_ready or self._lp_ready), offs, rows,
                               out_offs)
      else:       # one stage carried from a stand-alone call, the other still unset: two passes
        y = self._filter_stage(x, 'hp', reset or many or not self._hp_ready, offs)
        y = self._filter_stage(y, 'lp', reset or many or not self._lp_ready, offs, rows, out_offs)
    else:
      y = x
      if rows is not None:    # (no filter: upsampling, or a rate change with a cutoff of its own)
        gather = (rows + _torch().from_numpy(np.repeat(np.asarray(offs[:-1], np.int64), np.diff(out_offs)))
                  .to(x.device))
    self._next_frame_idx = next_idx
    groups = self._groups(c)
    select = self._channel_numbers or None
    m = out_offs[-1]
    if groups or select is not None or gather is not None or y.dtype != _torch().float64:
      z = device.reref_select(y, rows=gather, groups=groups, select=select) if m else \
          device.default_handle().zeros((0, len(select) if select else c), 'float64')
    else:
      z = y
    if self._data_std is None:
      raise TypeError('data_std=None is not supported (the reference rejects it in check_params)')
    if self._data_mean is None:
      self._data_mean = float(device.mean_f64(z[:out_offs[1]]).item())
    if not many:
      return self._context(z, self._data_mean, self._data_std, dtype), [0, None]
    outs, new_offs = [], [0]
    for f in range(len(out_offs) - 1):
      self.context_reset()
      o = self._context(z[out_offs[f]:out_offs[f + 1]], self._data_mean, self._data_std, dtype)
      outs.append(o)
      new_offs.append(new_offs[-1] + int(o.shape[0]))
    return _torch().cat(outs), new_offs

  def process(self, data, reset=False):
    """All steps for one batch of data [num_frames, num_channels]; reset restarts the filter states."""
    x, on_dev = self._to_device(data)
    self.check_dims(x)
    out, offs = self._run(x, [0, int(x.shape[0])], reset, self.device_dtype if on_dev else 'float64')
    return self._back(out, on_dev)

  def process_files(self, data, file_offsets, dtype=None):
    """Several recordings concatenated along time (rows file_offsets[f]:file_offsets[f+1]) in one call: each
    file as a fresh recording (filter states reset at its first row, resample phase and context restarted),
    as process(file, reset=True) after context_reset() would treat it.  Returns (output, output file
    offsets).  A frozen data_mean=None comes from the first file."""
    offs = [int(v) for v in file_offsets]
    if self.sos is not None and any(b == a for a, b in zip(offs, offs[1:])):
      raise ValueError('process_files: an empty file with a filter on (its reset reads the first row, as '
                       'the reference\'s highpass_filter_reset does)')
    x, on_dev = self._to_device(data)
    self.check_dims(x)
    if offs[0] != 0 or offs[-1] != int(x.shape[0]) or any(b < a for a, b in zip(offs, offs[1:])):
      raise ValueError('file_offsets must run from 0 to %d, nondecreasing' % int(x.shape[0]))
    self._next_frame_idx = 0
    dtype = dtype or (self.device_dtype if on_dev else 'float64')
    if len(offs) == 2:
      self.context_reset()
      out, _ = self._run(x, offs, True, dtype)
      return self._back(out, on_dev), [0, int(out.shape[0])]
    out, new_offs = self._run(x, offs, True, dtype)
    return self._back(out, on_dev), new_offs


# ------------------------------------------------------------------------------------------------ audio
# The device kernel's limits on compute_spectrogram (csrc/audio.hip); the reference has none.
SPECTROGRAM_MAX_SEGMENT = 1024
SPECTROGRAM_MAX_NFFT = 4096
SPECTROGRAM_MAX_TAPS = 16


def _np_dtype(torch_dtype):
  return _torch().empty(0, dtype=torch_dtype).numpy().dtype


def _torch_dtype(np_dtype):
  return _torch().from_numpy(np.empty(0, np_dtype)).dtype


class AudioFeatures(object):
  """Drop-in for the reference's preprocess.AudioFeatures (preprocess.py:589-755): the RMS intensity
  envelope of audio resampled by windowed means (audio_resample, compute_intensity) and an auditory
  spectrogram (compute_spectrogram), on the MI355X (csrc/audio.hip).

  A NumPy (or list) input returns NumPy in the reference's dtype; a torch tensor on the GPU stays there.
  The reference's quirks are kept: every call transposes an input with more columns
  than rows, the carried buffer holds the last int(fs_in * window / (2 fs_out)) rows of [buffer ; data]
  (all of them when that is 0), each call's window centres restart at t = 0 and stop at its end, an empty
  window gives NaN, and fs_out >= fs_in with window <= 1 passes the data through.  Means are summed in
  float64 (the reference's float32 means sit up to ~2.3e-7 from that).

  Difference: compute_spectrogram supports segment_size <= 1024, nfft <= 4096 and up to 16 smoothing taps
  and raises ValueError beyond them.
  """

  def __init__(self, name, fs_in, fs_out, window=1, exponent=1, buff=None):
    """Specifies desired parameters up front."""
    self.check_params(name, fs_in, fs_out, window)
    self._name = name
    self._fs_in = fs_in
    self._fs_out = fs_out
    self._window = window
    self._exponent = exponent
    self._buff = buff            # the caller's until the first call, then a device float64 tensor
    self._buff_dtype = None      # the dtype numpy's concatenation would give the buffer

  def check_params(self, name, fs_in, fs_out, window):
    """Checks correctness of parameters passed as input."""
    if not isinstance(name, str):
      raise TypeError('name must be a string, not %s' % name)
    if fs_in <= 0:
      raise ValueError('fs_in should not be less than 0.')
    if fs_out <= 0:
      raise ValueError('fs_out should not be less than 0.')
    if window <= 0:
      raise ValueError('window must be greater than than 0.')

  # ---------------------------------------------------------------- plumbing
  @staticmethod
  def _frames(data, square):
    """(x [N, C] float32 / float64 device tensor, was it a device tensor, the dtype numpy would see):
    1-D becomes a column, more columns than rows is transposed (preprocess.py:637-646)."""
    torch = _torch()
    if _is_device_tensor(data):
      x = data
      if square and x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
      dtype = np.dtype(np.float32) if square else _np_dtype(x.dtype)
      if x.dim() <= 1:
        x = x.reshape(-1, 1)
      elif x.dim() > 2:
        raise ValueError('audio data must be 1-D or 2-D, not %s' % (tuple(x.shape),))
      if x.shape[1] > x.shape[0]:
        x = x.t()
      if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float64)
      return x.contiguous(), True, dtype
    arr = np.asarray(data)
    if square:
      arr = arr.astype(np.float32)
    if arr.ndim <= 1:
      arr = np.reshape(arr, (-1, 1))
    elif arr.ndim > 2:
      raise ValueError('audio data must be 1-D or 2-D, not %s' % (arr.shape,))
    if arr.shape[1] > arr.shape[0]:
      arr = np.transpose(arr)
    dtype = arr.dtype
    if dtype not in (np.float32, np.float64):
      arr = arr.astype(np.float64)
    h = device.default_handle()
    return torch.from_numpy(np.ascontiguousarray(arr)).to(h.device), False, dtype

  def _buffer(self, c):
    """The carried buffer as a device float64 [B, c] tensor (None before any), checked against c channels
    as np.concatenate would."""
    if self._buff is None:
      return None
    if self._buff_dtype is None:       # the caller's buffer, first use
      b = self._buff
      if _is_device_tensor(b):
        dtype, t = _np_dtype(b.dtype), b.to(_torch().float64)
      else:
        arr = np.asarray(b)
        dtype = arr.dtype
        t = _torch().from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(device.default_handle().device)
      if t.dim() != 2:
        raise ValueError('all the input arrays must have same number of dimensions, but the buffer has %d '
                         'dimension(s) and the data 2' % t.dim())
      self._buff, self._buff_dtype = t.contiguous(), dtype
    if int(self._buff.shape[1]) != c:
      raise ValueError('all the input array dimensions except for the concatenation axis must match exactly, '
                       'but along dimension 1, the buffer has size %d and the data %d' %
                       (int(self._buff.shape[1]), c))
    return self._buff

  @staticmethod
  def _back(t, on_device, dtype):
    if on_device:
      want = _torch_dtype(dtype)
      return t if t.dtype == want else t.to(want)
    return t.cpu().numpy().astype(dtype, copy=False)

  def _resample(self, data, square):
    """audio_resample of data (square=False) or of float32(data)^2 followed by sqrt and ** exponent
    (square=True, compute_intensity)."""
    x, on_dev, dtype = self._frames(data, square)
    n, c = int(x.shape[0]), int(x.shape[1])
    half_window_size = 0.5 * self._window / self._fs_out
    buf = self._buffer(c)
    tau = int(buf.shape[0]) if buf is not None else 0
    cat_dtype = np.result_type(self._buff_dtype, dtype) if buf is not None else np.dtype(dtype)
    frames_in = tau + n
    frames_out = int(round((frames_in - tau) / self._fs_in * self._fs_out))
    keep = int(self._fs_in * half_window_size)
    begin = max(0, frames_in - keep) if keep > 0 else 0     # data[-keep:], data[-0:] being all of it
    h = device.default_handle()
    windowed = self._fs_out < self._fs_in or self._window > 1
    post = 1 if square else 0
    if windowed:
      out_dtype = np.dtype(np.float64)
    elif square:                   # numpy's dtypes of (data ** 0.5) ** exponent
      sq = np.ones(1, cat_dtype) ** 0.5
      out_dtype = (sq ** self._exponent).dtype
      post = 2 if (sq.dtype == np.float32 and out_dtype == np.float64) else 1
    else:
      out_dtype = cat_dtype
    if c == 0:                     # (an empty 1-D input, transposed to 1 x 0)
      out = h.zeros((frames_out if windowed else frames_in, 0), 'float64')
      new_buff = h.zeros((frames_in - begin, 0), 'float64')
    else:
      if windowed:
        out = device.audio_intensity(x, buf, frames_out, self._fs_in, self._fs_out, half_window_size, square,
                                     post, self._exponent)
      else:
        out = device.audio_passthrough(x, buf, 0, frames_in, square, post, self._exponent,
                                       'float32' if out_dtype == np.float32 else 'float64')
      new_buff = device.audio_passthrough(x, buf, begin, frames_in, square, 0, 1.0, 'float64')
    self._buff, self._buff_dtype = new_buff, cat_dtype
    return self._back(out, on_dev, out_dtype)

  # ---------------------------------------------------------------- the reference's methods
  def audio_resample(self, data):
    """Resamples audio [frames_in, channels] from fs_in to fs_out by (overlapping, window > 1) windowed
    means (preprocess.py:619-686): float64 [round(frames / fs_in * fs_out), channels], or the buffered rows
    plus the data unchanged when fs_out >= fs_in and window <= 1."""
    return self._resample(data, square=False)

  def compute_intensity(self, data):
    """The RMS intensity (the windowed mean of float32(data)^2, then sqrt) raised to `exponent`
    (preprocess.py:688-708)."""
    return self._resample(data, square=True)

  def compute_spectrogram(self, wave, segment_size=128, n_overlap=8, n_trans=4,
                          smoothing_filter=(.2, 1, .2)):
    """An auditory spectrogram (preprocess.py:712-755): scipy's STFT of the pre-emphasised wave (Hamming
    window, nfft = segment_size * n_trans), power smoothed by the causal FIR `smoothing_filter` along
    frequency then time, fourth root with a 1e-4 x max offset, scaled to 0..255.  Returns (spectrogram
    [nfft // 2 + 1, frames] float64, the bin frequencies numpy.fft.rfftfreq(nfft, 1.0))."""
    torch = _torch()
    on_dev = _is_device_tensor(wave)
    if on_dev:
      w = wave.squeeze().to(torch.float32)
    else:
      w = np.squeeze(np.asarray(wave)).astype(np.float32)
    if len(w.shape) != 1:
      raise ValueError('Wave.shape wrong:' + str(tuple(w.shape)))
    n = int(w.shape[0])
    if n == 0:
      raise ValueError('compute_spectrogram: an empty wave')
    seg = int(segment_size)
    if seg < 1:
      raise ValueError('nperseg must be a positive integer')
    seg = min(seg, n)              # scipy's _triage_segments: a wave shorter than a segment is one segment
    nfft = int(segment_size * n_trans)
    if nfft < seg:
      raise ValueError('nfft must be greater than or equal to nperseg.')
    noverlap = int(segment_size - segment_size / n_overlap)
    if noverlap >= seg:
      raise ValueError('noverlap must be less than nperseg.')
    taps = np.asarray(smoothing_filter, np.float64).ravel()
    if seg > SPECTROGRAM_MAX_SEGMENT:
      raise ValueError('compute_spectrogram: segment_size %d exceeds the device limit of %d' %
                       (seg, SPECTROGRAM_MAX_SEGMENT))
    if nfft > SPECTROGRAM_MAX_NFFT:
      raise ValueError('compute_spectrogram: nfft = segment_size * n_trans = %d exceeds the device limit of %d' %
                       (nfft, SPECTROGRAM_MAX_NFFT))
    if not 1 <= taps.shape[0] <= SPECTROGRAM_MAX_TAPS:
      raise ValueError('compute_spectrogram: %d smoothing taps, the device limit is 1 to %d' %
                       (taps.shape[0], SPECTROGRAM_MAX_TAPS))
    hop = seg - noverlap
    padded = n + 2 * (seg // 2)
    padded += (-(padded - seg) % hop) % seg
    frames = (padded - seg) // hop + 1
    if on_dev:
      wd = w.contiguous()
    else:
      wd = torch.from_numpy(np.ascontiguousarray(w)).to(device.default_handle().device)
    spec = device.audio_spectrogram(wd, seg, hop, nfft, taps, frames)
    f = np.fft.rfftfreq(nfft, 1.0)
    return (spec if on_dev else spec.cpu().numpy()), f
