"""GPU tests of the decoding driver: the windowed class-moments kernel against float64
NumPy with derived allowances, its repeatability, Decoder.train's windowed device route against the host
route on the golden G10 batches, the reference's own train_and_test / train_lda_model recipes
(test/decoding_test.py:219-309, thresholds unchanged, 2e4 frames), and run_decoding_experiment end to
end on TFRecord files."""
import json
import os

import numpy as np
import pytest

from tests import parity_log
from tests.conftest import golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
# the kernel's shares at up to 16384 windows (windows.hip: kWcmMinWinPerWave, four waves a workgroup)
WAVE_SHARE, GROUP_SHARE = 4, 16


# ---------------------------------------------------------------- 1. kernel sweep
def _stats(rng, cols, offset=0.0):
  return (offset + 0.5 * rng.standard_normal(cols), offset - 0.5 * rng.standard_normal(cols),
          rng.uniform(0.5, 2.0, cols))


def _reference(a, b, width, ma, mb, pw):
  """(window means, moments) in long double, and their allowances: a float64 sum of n terms in any order
  stays within n 2^-52 sum |terms|, so a window mean gets (width + 4) 2^-52 mean_w |v| and moment (i, j)
  (n_win + 2 width + 8) 2^-52 sum_w m~_i m~_j with m~ the window means of |v| (1 for the count's column)."""
  rows, cols = a.shape
  v = (a.astype(np.float64) - ma) * (b.astype(np.float64) - mb) / pw
  n_win = rows // width
  vw = v[:n_win * width].reshape(n_win, width, cols)
  means = vw.astype(LD).sum(axis=1) / LD(width)
  abs_means = np.abs(vw).mean(axis=1) if n_win else np.zeros((0, cols))
  aug = np.concatenate([means, np.ones((n_win, 1), LD)], axis=1)
  aug_abs = np.concatenate([abs_means, np.ones((n_win, 1))], axis=1)
  moments = aug.T @ aug
  return (means, moments, (width + 4) * EPS * abs_means,
          (n_win + 2 * width + 8) * EPS * (aug_abs.T @ aug_abs))


def _check_case(h, rng, rows, cols, width, stats=None, data_offset=0.0, tag=''):
  """One (rows, cols, width) on dense tensors and on strided views (lda = cols + 3, a column offset into a
  wider tensor).  Returns the worst observed error as a fraction of its allowance."""
  import torch
  from telluride_decoding_amd import device
  a = (data_offset + rng.standard_normal((rows, cols))).astype(np.float32)
  b = (data_offset + 0.5 * a - 0.5 * data_offset + rng.standard_normal((rows, cols))).astype(np.float32)
  ma, mb, pw = stats if stats is not None else _stats(rng, cols)
  means, moments, tol_means, tol_moments = _reference(a, b, width, ma, mb, pw)
  n_win = rows // width
  worst = 0.0
  for strided in (False, True):
    if strided:
      wide_a = h.to_device(rng.standard_normal((rows, cols + 3)).astype(np.float32))
      wide_b = h.to_device(rng.standard_normal((rows, cols + 3)).astype(np.float32))
      wide_a[:, 2:2 + cols] = torch.from_numpy(a).to(wide_a.device)
      wide_b[:, 1:1 + cols] = torch.from_numpy(b).to(wide_b.device)
      ad, bd = wide_a[:, 2:2 + cols], wide_b[:, 1:1 + cols]
      assert ad.stride(0) == cols + 3 and not (cols > 1 and ad.is_contiguous())
    else:
      ad, bd = h.to_device(a), h.to_device(b)
    got_moments, got_means = device.window_class_moments(ad, bd, width, ma, mb, pw, want_means=True, handle=h)
    only_moments = device.window_class_moments(ad, bd, width, ma, mb, pw, handle=h)
    assert torch.equal(only_moments, got_moments)
    got_moments, got_means = got_moments.cpu().numpy(), got_means.cpu().numpy()
    where = '%s rows=%d cols=%d width=%d strided=%s' % (tag, rows, cols, width, strided)
    assert got_means.shape == (n_win, cols) and got_moments.shape == (cols + 1, cols + 1), where
    assert got_moments[cols, cols] == n_win, where              # the count is exact
    if n_win == 0:
      assert not got_moments.any(), where
      continue
    err_means = np.abs(got_means.astype(LD) - means).astype(np.float64)
    err_moments = np.abs(got_moments.astype(LD) - moments).astype(np.float64)
    assert np.all(err_means <= tol_means), (where, float(np.max(err_means / tol_means)))
    assert np.all(err_moments <= tol_moments), (where, float(np.max(err_moments / tol_moments)))
    np.testing.assert_array_equal(got_moments, got_moments.T, err_msg=where)
    worst = max(worst, float(np.max(err_means / tol_means)), float(np.max(err_moments / tol_moments)))
  return worst


@pytest.mark.parametrize('cols', [1, 2, 5, 31, 32])
def test_window_class_moments_sweep(cols):
  """Window counts of one window, one less / exactly / one more than a wave's and a workgroup's share and
  three workgroups with a partial last one; rows % width of 0, 1 and width - 1; every width around the
  64-lane step; the window that is the whole stream and the one that is a frame too long."""
  from telluride_decoding_amd import device
  h = device.default_handle()
  rng = np.random.default_rng(100 + cols)
  worst = 0.0
  counts = (1, WAVE_SHARE - 1, WAVE_SHARE, WAVE_SHARE + 1, GROUP_SHARE - 1, GROUP_SHARE, GROUP_SHARE + 1,
            2 * GROUP_SHARE + 5)
  for wi, width in enumerate((2, 3, 63, 64, 65, 100, 257)):
    for ci, n_win in enumerate(counts):
      rest = (0, 1, width - 1)[(wi + ci) % 3]
      worst = max(worst, _check_case(h, rng, n_win * width + rest, cols, width))
    for rest in (0, 1, width - 1):            # every remainder at the largest count as well
      worst = max(worst, _check_case(h, rng, counts[-1] * width + rest, cols, width))
  for rows in (777, 1000):
    worst = max(worst, _check_case(h, rng, rows, cols, rows, tag='whole stream'))
    worst = max(worst, _check_case(h, rng, rows, cols, rows + 1, tag='no window'))
  parity_log.record('window_class_moments_sweep_cols%d' % cols, worst_fraction_of_allowance=worst)


def test_window_class_moments_large_shapes_and_offsets():
  """Means of about 100 against unit-variance data with power != 1 (the float64 centring), a window of 2e5
  frames (one wave walks it) and 1e5 windows (more than the minimum share per wave: 1000 workgroups)."""
  from telluride_decoding_amd import device
  h = device.default_handle()
  rng = np.random.default_rng(7)
  centred = _check_case(h, rng, 37 * 100 + 99, 5, 100, stats=_stats(rng, 5, offset=100.0), data_offset=100.0,
                        tag='means of 100')
  long_window = _check_case(h, rng, 200000, 5, 200000, tag='one long window')
  many = _check_case(h, rng, 200000, 2, 2, tag='1e5 windows')
  parity_log.record('window_class_moments_large', centred=centred, long_window=long_window, many_windows=many)


def test_window_class_moments_rejects_what_it_cannot_do():
  from telluride_decoding_amd import device
  h = device.default_handle()
  a = h.zeros((64, 33))
  with pytest.raises(ValueError, match='1 to 32 columns, not 33'):
    device.window_class_moments(a, a, 8, np.zeros(33), np.zeros(33), np.ones(33), handle=h)
  b = h.zeros((64, 4))
  with pytest.raises(ValueError, match='at least 2'):
    device.window_class_moments(b, b, 1, np.zeros(4), np.zeros(4), np.ones(4), handle=h)
  with pytest.raises(ValueError):
    device.window_class_moments(b, b[:, :3], 8, np.zeros(4), np.zeros(4), np.ones(4), handle=h)
  wide = h.zeros((64, 4), 'float64')
  with pytest.raises(TypeError, match='must be a float32 tensor'):
    device.window_class_moments(wide, wide, 8, np.zeros(4), np.zeros(4), np.ones(4), handle=h)
  with pytest.raises(TypeError, match='must be a float32 tensor'):
    device.window_class_moments(b, b.cpu(), 8, np.zeros(4), np.zeros(4), np.ones(4), handle=h)
  # no rows: no window, which is not an error
  none = h.zeros((0, 4))
  moments, means = device.window_class_moments(none, none, 8, np.zeros(4), np.zeros(4), np.ones(4),
                                               want_means=True, handle=h)
  assert tuple(moments.shape) == (5, 5) and not moments.cpu().numpy().any() and tuple(means.shape) == (0, 4)


# ---------------------------------------------------------------- 2. repeatability
def test_window_class_moments_is_bitwise_repeatable():
  import torch
  from telluride_decoding_amd import device
  h = device.default_handle()
  rng = np.random.default_rng(11)
  for rows, cols, width in ((53 * 100 + 17, 5, 100), (2000 * 3 + 2, 32, 3), (70000, 8, 7)):
    a, b = h.to_device(rng.standard_normal((rows, cols))), h.to_device(rng.standard_normal((rows, cols)))
    ma, mb, pw = _stats(rng, cols)
    first = device.window_class_moments(a, b, width, ma, mb, pw, want_means=True, handle=h)
    first = [t.clone() for t in first]
    device.window_class_moments(b, a, width + 1, mb, ma, pw, handle=h)      # another shape in between
    again = device.window_class_moments(a, b, width, ma, mb, pw, want_means=True, handle=h)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), (rows, cols, width)


def test_window_class_moments_same_bits_on_a_cu_masked_stream():
  """The grid follows from (rows, width) alone: a handle on a stream that owns 64 of the chip's CUs
  (pipeline.FitPipeline's solve stream) gives the bits of the default handle, moments and means."""
  import torch
  from telluride_decoding_amd import device, pipeline
  h = device.default_handle()
  pipe = pipeline.FitPipeline(16, 0, 3, d=1)
  assert pipe._masked, 'the pipeline did not get its CU-masked streams'
  rng = np.random.default_rng(12)
  for rows, cols, width in ((53 * 100 + 17, 5, 100), (2000 * 3 + 2, 32, 3), (70000, 8, 7), (30000, 1, 100)):
    a, b = h.to_device(rng.standard_normal((rows, cols))), h.to_device(rng.standard_normal((rows, cols)))
    ma, mb, pw = _stats(rng, cols)
    whole = device.window_class_moments(a, b, width, ma, mb, pw, want_means=True, handle=h)
    torch.cuda.synchronize()
    with torch.cuda.stream(pipe.s_solve):
      masked = device.window_class_moments(a, b, width, ma, mb, pw, want_means=True, handle=pipe.h_solve)
    pipe.h_solve.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(whole[0], masked[0]) and torch.equal(whole[1], masked[1]), (rows, cols, width)
    assert float(whole[0][cols, cols]) == rows // width


# ---------------------------------------------------------------- 3. / 4. Decoder.train
def _g10_batches():
  """The minibatches of golden G10 (the data of the reference's test/infer_decoder_test.py): matched
  training data, the same with input_2 and the output permuted inside every minibatch, and test data."""
  g = golden('g10_decoder_train')
  n, _, batch = (int(v) for v in g['cfg'])

  def batches(eeg, i1, flag, perms=None):
    out = []
    for k, s in enumerate(range(0, n, batch)):
      x2 = y = i1[s:s + batch]
      if perms is not None:
        x2, y = x2[perms[0][k]], y[perms[1][k]]
      out.append(({'input_1': eeg[s:s + batch], 'input_2': x2, 'attended_speaker': flag[s:s + batch]}, y))
    return out
  matched = batches(g['train_eeg'], g['train_i1'], g['train_flag'])
  mixed = batches(g['train_eeg'], g['train_i1'], g['train_flag'], (g['mix_perm_x2'], g['mix_perm_y']))
  return matched, mixed


def _g10_decoder(tag):
  from telluride_decoding_amd import infer_decoder
  if tag == 'linear':          # the models of test/infer_decoder_test.py:46-74
    return infer_decoder.LinearRegressionDecoder(lambda d: np.asarray(d['input_1']) / 2.0 + 0.5, reduction='lda')
  return infer_decoder.CCADecoder(
      lambda d: np.concatenate((np.asarray(d['input_1'])[:, 0:2], np.asarray(d['input_2'])[:, 0:2]), axis=1),
      reduction='lda')


def _host_route(dec, mixed, matched, window_size):
  """compute_lda_model(average_data(compute_correlation(...))) with the statistics of both classes: what
  Decoder.train does on the host for a window."""
  from telluride_decoding_amd import infer_decoder
  streams = []
  for data in (mixed, matched):
    pairs = [dec.decode_one(d, y) for d, y in data]
    r1 = np.concatenate([np.asarray(p[0]).reshape(len(p[0]), -1) for p in pairs])
    r2 = np.concatenate([np.asarray(p[1]).reshape(len(p[1]), -1) for p in pairs])
    dec.add_data_correlator(r1, r2)
    streams.append((r1, r2))
  classes = [infer_decoder.average_data(dec.compute_correlation(r1, r2), window_size) for r1, r2 in streams]
  return dec.compute_lda_model(classes[0], classes[1])


def _assert_same_model(dec, dprime, ref, ref_dprime, rtol=1e-5):
  got, want = dec.lda_params, ref.lda_params
  np.testing.assert_allclose(dprime, ref_dprime, rtol=rtol)
  scale = np.max(np.abs(want.slope * np.asarray(want.w_real)[:, 0]))
  np.testing.assert_allclose(got.slope * np.asarray(got.w_real)[:, 0],
                             want.slope * np.asarray(want.w_real)[:, 0], rtol=rtol, atol=rtol * scale)
  np.testing.assert_allclose(got.intercept, want.intercept, rtol=rtol, atol=rtol * scale)
  np.testing.assert_allclose(np.asarray(got.mean_vectors), np.asarray(want.mean_vectors), rtol=rtol,
                             atol=rtol * np.max(np.abs(np.asarray(want.mean_vectors))))
  return abs(dprime - ref_dprime) / abs(ref_dprime)


@pytest.mark.parametrize('tag', ['linear', 'cca'])
@pytest.mark.parametrize('window_size', [7, 100])
def test_train_windowed_device_route_matches_host_route(tag, window_size):
  matched, mixed = _g10_batches()
  dec = _g10_decoder(tag)
  dprime = dec.train(mixed, matched, window_size=window_size)
  ref = _g10_decoder(tag)
  ref_dprime = _host_route(ref, mixed, matched, window_size)
  err = _assert_same_model(dec, dprime, ref, ref_dprime)
  np.testing.assert_allclose(dec.correlation_params.power, ref.correlation_params.power, rtol=1e-12)
  parity_log.record('decoder_train_windowed_%s_w%d' % (tag, window_size), dprime=dprime, dprime_rel_err=err)


def _wide_batches(cols=33, n=2000, batch=500):
  rng = np.random.default_rng(41)
  x = rng.standard_normal((n, cols)).astype(np.float32)
  y = (x + rng.standard_normal((n, cols))).astype(np.float32)
  flag = np.zeros((n, 1), np.float32)
  matched = [({'input_1': x[s:s + batch], 'input_2': x[s:s + batch], 'attended_speaker': flag[s:s + batch]},
              y[s:s + batch]) for s in range(0, n, batch)]
  mixed = [(d, t[rng.permutation(len(t))]) for d, t in matched]
  return matched, mixed


def test_train_windowed_keeps_the_host_route_beyond_32_columns():
  from telluride_decoding_amd import infer_decoder
  matched, mixed = _wide_batches()
  make = lambda: infer_decoder.LinearRegressionDecoder(lambda d: np.asarray(d['input_1']), reduction='lda')
  dec, ref = make(), make()
  dprime = dec.train(mixed, matched, window_size=10)
  ref_dprime = _host_route(ref, mixed, matched, 10)
  assert np.isfinite(dprime) and dprime > 1.0
  _assert_same_model(dec, dprime, ref, ref_dprime)


def test_train_windowed_does_not_touch_the_host_helpers(monkeypatch):
  from telluride_decoding_amd import infer_decoder
  matched, mixed = _g10_batches()

  def forbidden(*args, **kwargs):
    raise AssertionError('the windowed route went through a host helper')
  monkeypatch.setattr(infer_decoder, 'average_data', forbidden)
  monkeypatch.setattr(infer_decoder.Decoder, 'compute_correlation', forbidden)
  for tag in ('linear', 'cca'):
    dprime = _g10_decoder(tag).train(mixed, matched, window_size=100)
    assert np.isfinite(dprime) and dprime > 0
  assert _g10_decoder('linear').train(mixed, matched, window_size=100.0) > 0     # a whole number as a float
  with pytest.raises(ValueError, match='must be a whole number of frames'):
    _g10_decoder('linear').train(mixed, matched, window_size=100.5)
  with pytest.raises(ValueError, match='No data for class 0'):       # no full window in class 0
    _g10_decoder('linear').train(mixed[:1], matched, window_size=len(mixed[0][1]) + 1)
  with pytest.raises(ValueError, match='No data for class 1'):
    _g10_decoder('linear').train(mixed, matched[:1], window_size=len(matched[0][1]) + 1)


# ---------------------------------------------------------------- 5. the reference's recipes
FRAMES = 20000


def _simulated_eeg(num_channels, frames, noise_level=0.3, unattended_gain=0.10, seed=0, fs=100):
  """The simulated recording of the reference's decoding_test.py:66-216: two "speakers" (5 Hz and 7 Hz
  sinusoids, the second attended), each through its own random 0.25 s impulse response per channel
  (shaped by 30 t exp(-30 t); the unattended one scaled by its gain), plus white noise.  Returns
  (response [frames, channels], attended audio [frames, 1])."""
  rng = np.random.RandomState(seed)
  t_imp = np.arange(int(0.25 * fs)) / float(fs)
  shape = (30 * t_imp * np.exp(-t_imp * 30)).reshape(-1, 1)
  h_att = rng.randn(len(t_imp), num_channels) * shape
  h_unatt = rng.randn(len(t_imp), num_channels) * shape * unattended_gain
  times = np.arange(frames) / float(fs)
  unattended = np.sin(times * 2 * np.pi * 5).astype(np.float32)
  attended = np.sin(times * 2 * np.pi * 7).astype(np.float32)
  response = np.zeros((frames, num_channels), np.float32)
  for c in range(num_channels):
    full = np.convolve(attended, h_att[:, c]) + np.convolve(unattended, h_unatt[:, c])
    response[:, c] = (full + noise_level * rng.randn(len(full)))[:frames]
  return response, attended.reshape(-1, 1)


def _recipe_flags(**values):
  from telluride_decoding_amd import decoding
  flags = decoding.DecodingOptions().set_from_dict({'attended_field': ''})   # the reference's flag defaults
  return flags.set_from_dict(values)


def test_train_and_test_linear_recipe():
  from telluride_decoding_amd import brain_data, decoding
  flags = _recipe_flags(dnn_regressor='linear', regularization_lambda=0.0)
  bd = brain_data.TestBrainData('input', 'output', flags.frame_rate, final_batch_size=flags.batch_size,
                                pre_context=flags.pre_context, post_context=flags.post_context, repeat_count=1)
  response, speech = _simulated_eeg(32, FRAMES)
  bd.preserve_test_data(response, speech)
  model = decoding.create_brain_model(flags, bd.create_dataset('train'))
  train_results, test_results = decoding.train_and_test(flags, bd, model)
  parity_log.record('decoding_recipe_linear', pearson=test_results['pearson_correlation_first'])
  assert train_results == {}
  assert test_results['pearson_correlation_first'] > 0.97


def test_train_and_test_dnn_recipe():
  from telluride_decoding_amd import brain_data, decoding
  flags = _recipe_flags(dnn_regressor='fullyconnected')
  assert (flags.learning_rate, flags.hidden_units) == (0.05, '20-20')
  bd = brain_data.TestBrainData('input', 'output', flags.frame_rate, final_batch_size=flags.batch_size,
                                pre_context=flags.pre_context, post_context=flags.post_context, repeat_count=1)
  response, speech = _simulated_eeg(32, FRAMES)
  bd.preserve_test_data(response, speech)
  model = decoding.create_brain_model(flags, bd.create_dataset('train'))
  train_results, test_results = decoding.train_and_test(flags, bd, model, epochs=10)
  parity_log.record('decoding_recipe_dnn', pearson=test_results['pearson_correlation_first'])
  assert len(train_results.history['loss']) == 10
  assert test_results['pearson_correlation_first'] > 0.97


def test_train_and_test_cca_recipe_and_lda_model():
  from telluride_decoding_amd import brain_data, decoding, infer_decoder
  flags = _recipe_flags(dnn_regressor='cca', pre_context=2, post_context=3, input2_field='speech',
                        cca_dimensions=4)
  bd = brain_data.TestBrainData('eeg', 'none', flags.frame_rate, final_batch_size=flags.batch_size,
                                pre_context=flags.pre_context, post_context=flags.post_context,
                                in2_fields=flags.input2_field, in2_pre_context=flags.pre_context,
                                in2_post_context=flags.post_context, repeat_count=1)
  response, speech = _simulated_eeg(32, FRAMES, noise_level=0.0, unattended_gain=0.0)
  bd.preserve_test_data(response, 0 * response[:, 0:1], speech)
  model = decoding.create_brain_model(flags, bd.create_dataset('train'))
  _, test_results = decoding.train_and_test(flags, bd, model)
  assert abs(test_results['cca_pearson_correlation_first']) > 0.75
  dprime, decoder = decoding.train_lda_model(bd, model, flags)
  parity_log.record('decoding_recipe_cca', pearson=test_results['cca_pearson_correlation_first'], dprime=dprime)
  assert dprime > 0.7
  assert isinstance(decoder, infer_decoder.Decoder)
  same, _ = decoding.train_lda_model(bd, model, flags.as_dict())          # a dict of options is accepted
  assert same == dprime


# ---------------------------------------------------------------- 6. end to end on files
@pytest.fixture(scope='module')
def recordings(tmp_path_factory):
  """Six synthetic recordings (16 channels, 3000 frames) as TFRecord files."""
  from telluride_decoding_amd import synth, tfrecord
  root = tmp_path_factory.mktemp('recordings')
  for i, (eeg, env, att) in enumerate(synth.make_trials(17, 6, 3000, 16)):
    label = (np.arange(3000) % 2).astype(np.float32).reshape(-1, 1)
    tfrecord.write_file(str(root / ('subj_trial_%d.tfrecords' % i)),
                        {'eeg': eeg, 'envelope': env[:, 0:1], 'attend': att, 'label': label})
  return str(root)


def _file_flags(recordings, tmp_path, **values):
  from telluride_decoding_amd import decoding
  flags = decoding.DecodingOptions().set_from_dict(dict(
      tfexample_dir=recordings, input_field='eeg', output_field='envelope', dnn_regressor='linear',
      pre_context=0, post_context=21, train_file_pattern='allbut', test_file_pattern='trial_0',
      validate_file_pattern='trial_1', correlation_frames=100, batch_size=512,
      summary_dir=str(tmp_path / 'summary')))
  return flags.set_from_dict(values)


def test_run_decoding_experiment_on_files(recordings, tmp_path):
  from telluride_decoding_amd import brain_data, brain_model, decoding, infer_decoder
  flags = _file_flags(recordings, tmp_path, saved_model_dir=str(tmp_path / 'saved'))
  train_results, test_results, dprime = decoding.run_decoding_experiment(flags)
  assert train_results == {} and flags.summary_dir.endswith('/')

  # the same steps by hand
  bd = brain_data.TFExampleData('eeg', 'envelope', 100.0, pre_context=0, post_context=21, attended_field='attend',
                                final_batch_size=512, data_dir=recordings, train_file_pattern='allbut',
                                test_file_pattern='trial_0', validate_file_pattern='trial_1')
  assert [os.path.basename(f) for f in bd.filter_file_names('train')] == [
      'subj_trial_%d.tfrecords' % i for i in (2, 3, 4, 5)]
  model = brain_model.BrainModelLinearRegression(bd.create_dataset('train'), 0.1)
  model.fit(bd.create_dataset('train'))
  want_results = model.evaluate(bd.create_dataset('test'))
  decoder = infer_decoder.create_decoder('linear', reduction='lda', model=model)
  want_dprime = decoder.train(bd.create_dataset('test', mixup_batch=True), bd.create_dataset('test'),
                              window_size=100)
  assert set(test_results) == set(want_results) == {'loss', 'pearson_correlation_first'}
  for k in want_results:
    np.testing.assert_allclose(test_results[k], want_results[k], rtol=1e-12)
  np.testing.assert_allclose(dprime, want_dprime, rtol=1e-12)
  assert test_results['pearson_correlation_first'] > 0.5 and dprime > 1.0
  parity_log.record('decoding_end_to_end', pearson=test_results['pearson_correlation_first'], dprime=dprime)

  with open(os.path.join(flags.summary_dir, 'results.txt')) as fp:
    lines = fp.read().splitlines()
  assert lines[0] == 'Parameters: %s' % flags.experiment_parameters(';')
  assert lines[1:] == ['Final_Testing/%s: %g' % (k, test_results[k]) for k in test_results] + [
      'Final_Testing/dprime: %g' % dprime]

  saved = os.path.join(flags.saved_model_dir, 'decoder_model.json')
  assert os.listdir(flags.saved_model_dir) == ['decoder_model.json']
  with open(saved) as fp:
    json.load(fp)
  restored = infer_decoder.create_decoder('linear', reduction='lda', model=model)
  restored.restore_parameters(saved)
  np.testing.assert_allclose(restored.correlation_params.power, decoder.correlation_params.power, rtol=1e-12)
  np.testing.assert_allclose(restored.lda_params.slope, decoder.lda_params.slope, rtol=1e-12)
  np.testing.assert_allclose(np.asarray(restored.lda_params.w_real), np.asarray(decoder.lda_params.w_real),
                             rtol=1e-12)


def test_run_decoding_experiment_classifier_has_no_lda_stage(recordings, tmp_path):
  from telluride_decoding_amd import decoding
  flags = _file_flags(recordings, tmp_path, dnn_regressor='classifier', input2_field='envelope',
                      output_field='label', hidden_units='8', epoch_count=2, post_context=3,
                      learning_rate=0.001)
  train_results, test_results, dprime = decoding.run_decoding_experiment(flags)
  assert dprime is None
  assert np.isfinite(test_results['loss']) and 0.0 <= test_results['accuracy'] <= 1.0
  assert len(train_results.history['loss']) == 2
  with open(os.path.join(flags.summary_dir, 'results.txt')) as fp:
    text = fp.read()
  assert 'Final_Testing/loss: %g\n' % test_results['loss'] in text and 'dprime' not in text
