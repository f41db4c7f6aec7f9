"""GPU parity of the Preprocessor drop-in (csrc/preprocess.hip through telluride_decoding_amd.preprocess)
against the reference's own outputs (G16, G17) and the host float64 restatement (tests/host_preprocess.py).
Bounds: float64 output within 1e-9 x max|x|; float32 output within that plus 2^-23 x max|ref|; resample
indices, channel selection and context layout exact; the frozen mean within 1e-12 of the data's scale.
The observed distances go to tests/parity_log."""
import json

import numpy as np
import pytest

from tests import host_preprocess as hp
from tests import parity_log

pytestmark = pytest.mark.gpu

CASES = ('a', 'b', 'c', 'd')


@pytest.fixture(scope='module')
def g16(load_golden):
  return load_golden('g16_preprocess')


@pytest.fixture(scope='module')
def pp():
  from telluride_decoding_amd import preprocess
  return preprocess


def make(pp, kw):
  kw = dict(json.loads(kw) if isinstance(kw, str) else kw)
  return pp.Preprocessor('g', kw.pop('fs_in'), kw.pop('fs_out'), **kw)


def dist(got, want, x_scale):
  got = np.asarray(got, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  return float(np.max(np.abs(got - want))) / x_scale if want.size else 0.0


@pytest.mark.parametrize('name', CASES)
def test_g16_whole(g16, pp, name):
  x = g16[name + '_x']
  scale = float(np.max(np.abs(x)))
  p = make(pp, str(g16[name + '_kwargs']))
  got = p.process(x)
  assert isinstance(got, np.ndarray) and got.dtype == np.float64
  d = dist(got, g16[name + '_whole'], scale)
  ds = dist(p.filter_state.cpu().numpy(), g16[name + '_whole_state'], scale) if p.sos is not None else 0.0
  parity_log.record('preprocess_g16_whole_' + name, out=d, state=ds)
  assert d <= 1e-9 and ds <= 1e-9
  assert p._next_frame_idx == int(g16[name + '_whole_next'])
  if name == 'a':
    assert abs(p.data_mean - float(g16['a_data_mean'])) <= 1e-12 * scale


@pytest.mark.parametrize('name', CASES)
def test_g16_streamed(g16, pp, name):
  x = g16[name + '_x']
  scale = float(np.max(np.abs(x)))
  p = make(pp, str(g16[name + '_kwargs']))
  s, worst = 0, 0.0
  for i, m in enumerate(g16[name + '_calls']):
    got = p.process(x[s:s + m], reset=(i == int(g16[name + '_reset_at'])))
    worst = max(worst, dist(got, g16['%s_call%d' % (name, i)], scale))
    s += m
  ds = dist(p.filter_state.cpu().numpy(), g16[name + '_stream_state'], scale) if p.sos is not None else 0.0
  parity_log.record('preprocess_g16_streamed_' + name, out=worst, state=ds)
  assert worst <= 1e-9 and ds <= 1e-9
  assert p._next_frame_idx == int(g16[name + '_stream_next'])


def test_misaligned_resample_raises(g16, pp):
  assert int(g16['c_second_raises']) == 1
  p = make(pp, str(g16['c_kwargs']))
  p.process(g16['c_x'])
  with pytest.raises(ValueError):
    p.process(g16['c_x'][:100])


def test_context_layout_and_selection_exact(g16, pp):
  """Filters off: channel selection, re-referencing and the context gather reproduce the reference exactly
  up to the float64 means (pure copies where no group subtracts)."""
  kw = json.loads(str(g16['b_kwargs']))
  kw.update(highpass_cutoff=0, lowpass_cutoff=0, ref_channels=None, channels_to_ref=None)
  x = g16['b_x'].astype(np.float64)
  p = make(pp, kw)
  h = hp.HostPreprocessor(kw)
  for s, m in ((0, 1000), (1000, 333), (1333, 1667)):
    np.testing.assert_array_equal(p.process(x[s:s + m]), h.process(x[s:s + m]))


def test_input_not_mutated(g16, pp):
  x = g16['b_x'].astype(np.float64)
  keep = x.copy()
  kw = dict(fs_in=128, fs_out=128, ref_channels=[[0]], channels_to_ref=[[1, 2]])
  p = make(pp, kw)
  p.process(x)
  p.reref_data(x)
  np.testing.assert_array_equal(x, keep)


def test_multi_file_call(g16, pp):
  x = g16['multi_x']
  offs = g16['multi_offsets']
  scale = float(np.max(np.abs(x)))
  p = make(pp, str(g16['a_kwargs']))
  got, out_offs = p.process_files(x, offs)
  want = [g16['multi_out0'], g16['multi_out1']]
  assert out_offs == [0, want[0].shape[0], want[0].shape[0] + want[1].shape[0]]
  d = max(dist(got[out_offs[f]:out_offs[f + 1]], want[f], scale) for f in range(2))
  parity_log.record('preprocess_multi_file', out=d)
  assert d <= 1e-9


def _host_case(c, n, fs_in=1000, fs_out=100, hpc=0.5, seed=0, calls=None):
  rng = np.random.default_rng(seed)
  x = (1.5 + rng.standard_normal((n, c))).astype(np.float32)
  kw = dict(fs_in=fs_in, fs_out=fs_out, highpass_cutoff=hpc, highpass_order=4, channels_to_ref=[list(range(c))],
            data_mean=None, data_std=1.5)
  return x, kw


@pytest.mark.parametrize('c', [1, 8, 63, 64, 128])
def test_channel_counts(pp, c):
  x, kw = _host_case(c, 3000, seed=c)
  want = hp.HostPreprocessor(kw).process(x)
  p = make(pp, kw)
  d = dist(p.process(x), want, float(np.max(np.abs(x))))
  parity_log.record('preprocess_channels_%d' % c, out=d)
  assert d <= 1e-9


@pytest.mark.parametrize('n', [4097, 16 * 64 * 64 + 13, 5, 1])
def test_frame_counts(pp, n):
  """N not a multiple of the chunk, N past one scan block of chunks (two scan levels), N shorter than a
  chunk, a single frame."""
  x, kw = _host_case(3, n, fs_in=100, fs_out=100, hpc=1.0, seed=n)
  kw['data_mean'] = 0.25
  want = hp.HostPreprocessor(kw).process(x)
  p = make(pp, kw)
  got = p.process(x)
  d = dist(got, want, float(np.max(np.abs(x))))
  parity_log.record('preprocess_frames_%d' % n, out=d)
  assert d <= 1e-9


def test_device_tensor_in_out(g16, pp):
  import torch
  from telluride_decoding_amd import device
  h = device.default_handle()
  x = g16['b_x']
  scale = float(np.max(np.abs(x)))
  p = make(pp, str(g16['b_kwargs']))
  t = torch.from_numpy(x).to(h.device)
  got = p.process(t)
  assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32
  want = g16['b_whole']
  err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want)))
  assert err <= 1e-9 * scale + 2.0 ** -23 * float(np.max(np.abs(want)))
  q = make(pp, str(g16['b_kwargs']))
  q.device_dtype = 'float64'
  got64 = q.process(t)
  assert got64.dtype == torch.float64 and dist(got64.cpu().numpy(), want, scale) <= 1e-9


def test_p1_against_g17(load_golden, pp):
  g17 = load_golden('g17_preprocess_long')
  x = hp.p1_input()
  np.testing.assert_array_equal(x[:4, :4], g17['x_head'])
  assert abs(float(x.astype(np.float64).sum()) - float(g17['x_sum'])) <= 1e-6 * abs(float(g17['x_sum']))
  scale = float(np.max(np.abs(x)))
  p = make(pp, hp.P1)
  import torch
  from telluride_decoding_amd import device
  t = torch.from_numpy(x).to(device.default_handle().device)
  p.device_dtype = 'float64'
  y = p.process(t)
  assert y.shape[0] == int(g17['n_out'])
  rows = g17['rows']
  d = dist(y[torch.from_numpy(rows).to(y.device)].cpu().numpy(), g17['y_rows'], scale)
  ds = dist(p.filter_state.cpu().numpy(), g17['state'], scale)
  dm = abs(p.data_mean - float(g17['data_mean'])) / scale
  parity_log.record('preprocess_p1', out=d, state=ds, mean=dm)
  # (the state was held to 2e-9 while the chunk scan ran in plain float64 -- observed 1.2e-9; with the
  # compensated scan it is 4e-12)
  assert d <= 1e-9 and ds <= 1e-9 and dm <= 1e-12


def test_dataset_from_files_feeds_fit(g16, pp, tmp_path):
  from telluride_decoding_amd import brain_data, brain_model, tfrecord
  kw = json.loads(str(g16['fit_kwargs']))
  names, ref_files = [], []
  for f in range(2):
    name = str(tmp_path / ('rec%d.tfrecords' % f))
    tfrecord.write_file(name, {'eeg': g16['fit_eeg%d' % f], 'env': g16['fit_env%d' % f]})
    names.append(name)
    pre = g16['fit_pre%d' % f].astype(np.float32)
    ref_files.append((pre, pre[:, 0:1], g16['fit_env%d' % f], np.zeros((pre.shape[0], 1), np.float32)))
  ds = tfrecord.dataset_from_files(names, 'eeg', 'env', batch_size=100, post_context=4,
                                   preprocess={'eeg': make(pp, kw)})
  model = brain_model.BrainModelLinearRegression(ds, regularization_lambda=0.1)
  model.fit(ds)
  ref_ds = brain_data.Dataset(ref_files, 100, post_context=4)
  ref_model = brain_model.BrainModelLinearRegression(ref_ds, regularization_lambda=0.1)
  ref_model.fit(ref_ds)
  w, w_ref = np.asarray(model.w_estimate), np.asarray(ref_model.w_estimate)
  err = float(np.max(np.abs(w - w_ref)) / np.max(np.abs(w_ref)))
  parity_log.record('preprocess_fit_weights', rel=err)
  assert err <= 1e-5
  # the string form builds the same preprocessor
  spec = 'eeg(highpass_cutoff=0.5;highpass_order=4;lowpass_cutoff=30;lowpass_order=4;channel_numbers=0-3,7)'
  ds2 = tfrecord.dataset_from_files(names[:1], 'eeg', 'env', batch_size=100, preprocess={'eeg': spec},
                                    frame_rate=128)
  assert ds2.files[0][0].shape == (g16['fit_eeg0'].shape[0], 5)


@pytest.mark.timeout(600)
def test_p1_every_row_against_float64(pp):
  """P1 on every output row and the final state against the float64 sequential filter of p1_input()
  (tests/host_preprocess.sosfilt_ref), at the general bound: the scan must not leave any chunk position of
  its blocks outside it."""
  x = hp.p1_input()
  n = hp.ref_rows(x.shape[0])
  x = x[:n]
  scale = float(np.max(np.abs(x)))
  h = hp.HostPreprocessor(hp.P1)
  want = h.process(x)
  p = make(pp, hp.P1)
  import torch
  from telluride_decoding_amd import device
  p.device_dtype = 'float64'
  got = p.process(torch.from_numpy(x).to(device.default_handle().device)).cpu().numpy()
  d = dist(got, want, scale)
  ds = dist(p.filter_state.cpu().numpy(), h.state(), scale)
  worst_row = int(np.argmax(np.max(np.abs(got - want), axis=1)))
  parity_log.record('preprocess_p1_every_row', out=d, state=ds, worst_row=worst_row, frames=n, ref=hp.REF_PATH)
  assert d <= 1e-9 and ds <= 1e-9, (d, ds, worst_row)
