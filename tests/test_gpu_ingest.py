"""GPU side of the ingest drop-in (csrc/ingest.hip through telluride_decoding_amd.ingest).

Encoder: byte for byte against the reference's own file (tests/golden/meg_subj01_400.tfrecords) and against
tfrecord.write_file of the NumPy-cast arrays, over the group edges, every payload alignment, both routes, both
input dtypes, strided and reversed inputs and the special bit patterns.  Moments: against a long double / fsum
two-pass truth (tests/host_ingest.py) within 1e-12 -- float64 tree sums of <= 1e5 terms err by about
log2(n) 2^-53 ~ 2e-15 of sum |x|, and the mean's error enters the centred sum only to second order, so 1e-12
leaves two to three orders of margin and is still 1e4 times tighter than a one-pass formula reaches on data with
this DC offset.  Normalise: the bits of NumPy's (a - mean) / std.  End to end: one ulp of float32."""
import os
import pickle

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
def ingest():
  from telluride_decoding_amd import ingest as module
  return module


@pytest.fixture(scope='module')
def device():
  from telluride_decoding_amd import device as module
  assert module.gpu_available()
  return module


@pytest.fixture(autouse=True)
def on_the_gpu(device):
  """ingest takes its device path whenever a GPU is visible: none of these tests may run without one."""
  assert device.gpu_available()


@pytest.fixture(scope='module')
def g19(load_golden):
  return load_golden('g19_ingest')


def read_bytes(path):
  with open(path, 'rb') as f:
    return f.read()


def host_file(path, data, flipped=()):
  """What the host writer makes of the same data, cast by NumPy."""
  with np.errstate(over='ignore', invalid='ignore'):
    cast = {k: (v[::-1] if k in flipped else v).astype(np.float32) for k, v in data.items()}
  tfrecord.write_file(path, cast)
  return read_bytes(path)


def strided(torch, a):
  """The array as a device view whose rows are further apart than its width."""
  big = torch.zeros((a.shape[0], a.shape[1] + 5), dtype=torch.from_numpy(a[:0]).dtype, device='cuda')
  big[:, 2:2 + a.shape[1]] = torch.from_numpy(a).cuda()
  view = big[:, 2:2 + a.shape[1]]
  assert view.shape[0] < 2 or view.stride(0) == a.shape[1] + 5
  return view


def check_encode(torch, ingest, tmp_path, data, as_device=(), as_strided=(), flipped=False):
  given = {}
  for k, v in data.items():
    given[k] = strided(torch, v) if k in as_strided else (torch.from_numpy(v).cuda() if k in as_device else v)
  out = str(tmp_path / 'device.tfrecords')
  from telluride_decoding_amd import device
  launches = []
  encode = device.tfrecord_encode
  device.tfrecord_encode = lambda *a, **k: launches.append(1) or encode(*a, **k)
  try:
    write(ingest, tmp_path, given, out, flipped)
  finally:
    device.tfrecord_encode = encode
  assert len(launches) == 1                      # the whole file image in one call
  want = host_file(str(tmp_path / 'host.tfrecords'), data, ('eeg',) if flipped else ())
  return compare(out, want, data)


def write(ingest, tmp_path, given, out, flipped):
  if flipped:
    trial = ingest.BrainTrial('device')
    for k, v in given.items():
      trial.add_model_feature(k, v)
    assert trial.write_data_as_tfrecords(str(tmp_path), reverse_data_for_test=True) == out
  else:
    ingest.convert_data_to_tfrecords(out, given)


def compare(out, want, data):
  assert len(want) < 3 << 20
  got = read_bytes(out)
  assert len(got) == len(want)
  if got != want:
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    bad = np.flatnonzero(g != w)
    stride = len(want) // next(iter(data.values())).shape[0]
    raise AssertionError('%d bytes differ, the first at record %d byte %d (stride %d)' %
                         (len(bad), bad[0] // stride, bad[0] % stride, stride))
  return out


# ---------------------------------------------------------------- encoder
def test_encoder_reproduces_the_reference_file(torch, ingest, device, tmp_path):
  data = tfrecord.read_file(GOLDEN_FILE)
  template, _ = ingest.device_record_plan(data)
  assert len(template) == 650 and device.tfrecord_route(650)[0]
  out = str(tmp_path / 'golden.tfrecords')
  ingest.convert_data_to_tfrecords(out, {k: torch.from_numpy(v).cuda() for k, v in data.items()})
  got, want = read_bytes(out), read_bytes(GOLDEN_FILE)
  assert len(want) == 260000 and got == want
  ingest.convert_data_to_tfrecords(out, data)            # NumPy in: the same path
  assert read_bytes(out) == want


@pytest.mark.parametrize('frames', [1, 2, 63, 64, 65, 257, 1000])
def test_encoder_group_edges(torch, ingest, tmp_path, frames):
  """Five features (names of 1 to 5 letters, widths 1 / 3 / 31 / 32 / 33, float32 and float64 by turns, one
  strided, three on the device) over the group edges and a last partial group, plain and reversed."""
  widths = (1, 3, 31, 32, 33)
  data = {name: hi.fill_bits((frames, w), np.float64 if i % 2 else np.float32, 100 * frames + i)
          for i, (name, w) in enumerate(zip(NAMES, widths))}
  check_encode(torch, ingest, tmp_path, data, as_device=('a', 'ccc'), as_strided=('dddd',))
  data['eeg'] = data.pop('eeeee')
  out = check_encode(torch, ingest, tmp_path, data, as_device=('bb', 'eeg'), as_strided=('ccc',), flipped=True)
  if frames == 257:
    back = tfrecord.read_file(out, verify=True)
    with np.errstate(over='ignore', invalid='ignore'):
      assert hi.same_bits(back['eeg'], data['eeg'][::-1].astype(np.float32))
      assert hi.same_bits(back['a'], data['a'])


@pytest.mark.parametrize('width', [1, 3, 31, 32, 33, 148])
def test_encoder_every_alignment(torch, ingest, device, tmp_path, width):
  """One feature, its name 1 to 5 letters long: the payload offset and the stride take every residue mod 4."""
  residues = set()
  for i, name in enumerate(NAMES):
    for dtype in (np.float32, np.float64):
      data = {name: hi.fill_bits((65, width), dtype, 7 * width + i)}
      template, layout = tfrecord.record_template({name: width})
      residues.add((layout[0][1] % 4, len(template) % 4))
      check_encode(torch, ingest, tmp_path, data, as_device=(name,) if i % 2 else ())
  assert {r[0] for r in residues} == {0, 1, 2, 3} and {r[1] for r in residues} == {0, 1, 2, 3}


def single_width_stride(width):
  return len(tfrecord.record_template({'x': width})[0])


def test_encoder_both_sides_of_the_large_record_predicate(torch, ingest, device, tmp_path):
  """The widest record that is staged, the first that is not (device.tfrecord_route), 4096 floats (record above
  16 KB, three-byte varints), and two features with a 20 000-float one; 3 frames each."""
  large = next(w for w in range(1, 13000) if not device.tfrecord_route(single_width_stride(w))[0])
  assert large > 1 and device.tfrecord_route(single_width_stride(large - 1))[0]
  for i, width in enumerate((large - 1, large, 4096)):
    for dtype in (np.float32, np.float64):
      data = {'x': hi.fill_bits((3, width), dtype, width + i)}
      check_encode(torch, ingest, tmp_path, data, as_device=('x',))
  # the largest record that is staged at all: one whose stride is a multiple of 16 fills the staging area alone
  stride, name, width = max((len(tfrecord.record_template({n: w})[0]), n, w) for n in NAMES
                            for w in range(12250, 12290)
                            if device.tfrecord_route(len(tfrecord.record_template({n: w})[0]))[0])
  assert stride % 16 == 0 and device.tfrecord_route(stride)[1] == 1
  check_encode(torch, ingest, tmp_path, {name: hi.fill_bits((3, width), np.float32, 9)}, as_device=(name,))
  assert single_width_stride(4096) > 16384
  data = {'eeg': hi.fill_bits((3, 20000), np.float64, 5), 'm': hi.fill_bits((3, 2), np.float32, 6)}
  assert not device.tfrecord_route(len(ingest.device_record_plan(data)[0]))[0]
  check_encode(torch, ingest, tmp_path, data, as_strided=('eeg',), flipped=True)


def test_encoder_two_features_and_integers(torch, ingest, tmp_path):
  data = {'eeg': hi.fill_bits((70, 64), np.float32, 1), 'intensity': hi.fill_bits((70, 1), np.float64, 2)}
  check_encode(torch, ingest, tmp_path, data, as_device=('eeg', 'intensity'))
  check_encode(torch, ingest, tmp_path, data, as_device=('eeg',), flipped=True)
  # an int32 feature has no fixed record layout: the host writes the trial, the integers as an Int64List
  ints = np.arange(-70, 140, 3, dtype=np.int32).reshape(70, 1)
  mixed = {'eeg': torch.from_numpy(data['eeg']).cuda(), 'label': ints}
  assert ingest.device_record_plan(mixed) is None
  out = str(tmp_path / 'mixed.tfrecords')
  ingest.convert_data_to_tfrecords(out, mixed)
  first = tfrecord.parse_example(next(tfrecord.iter_records(out, verify=True)))
  assert first['label'].dtype == np.int64
  back = tfrecord.read_file(out)
  assert np.array_equal(back['label'], ints.astype(np.float32)) and hi.same_bits(back['eeg'], data['eeg'])
  with pytest.raises(ValueError):
    ingest.convert_data_to_tfrecords(out, {'eeg': mixed['eeg'], 'c': np.zeros((70, 1), np.complex64)})


# ---------------------------------------------------------------- moments
SWEEP_MOMENT_CASES = (('one', (1,), 1, 'float64'), ('row', (1,), 3, 'float32'), ('w3', (63, 1025, 4097), 3, 'float64'),
                      ('w64', (4097, 1, 1025, 63), 64, 'float32'), ('w148', (1025, 4097), 148, 'float64'),
                      ('w1', (63, 1, 1025, 4097, 63), 1, 'float32'))
_truth = {}


def moment_case(case):
  """(the arrays, {columnwise: (mean, std)} truth), computed once."""
  name, rows, width, dtype = case
  if name not in _truth:
    arrays = hi.moments_data(name, rows, width, dtype)
    _truth[name] = (arrays, {cw: hi.moments_truth(arrays, cw) for cw in (False, True)})
  return _truth[name]


def check_moments(got, truth, arrays, columnwise, slack_mean=0.0, slack_std=0.0):
  mean, std = got
  t_mean, t_std = truth
  if columnwise:
    width = arrays[0].shape[1]
    assert mean.shape == (1, width) == std.shape and mean.dtype == np.float64 == std.dtype
  else:
    assert type(mean) is np.float64 and type(std) is np.float64
  scale = np.mean(np.abs(np.concatenate(arrays).astype(np.float64)), axis=0 if columnwise else None)
  err_mean, err_std = np.abs(mean - t_mean), np.abs(std - t_std)
  print('moments: mean off by %.3g of mean|x|, std by %.3g of std' %
        (np.max(err_mean / scale), np.max(err_std / np.maximum(t_std, 1e-300))))
  assert np.all(err_mean <= 1e-12 * scale + slack_mean)
  assert np.all(err_std <= 1e-12 * np.asarray(t_std) + slack_std)


@pytest.mark.parametrize('columnwise', [False, True], ids=['whole', 'columns'])
@pytest.mark.parametrize('case', SWEEP_MOMENT_CASES, ids=[c[0] for c in SWEEP_MOMENT_CASES])
def test_moments_sweep(torch, ingest, case, columnwise):
  arrays, truth = moment_case(case)
  check_moments(ingest.find_mean_std(arrays, columnwise=columnwise), truth[columnwise], arrays, columnwise)
  on_device = [torch.from_numpy(a).cuda() for a in arrays]
  check_moments(ingest.find_mean_std(on_device, columnwise=columnwise), truth[columnwise], arrays, columnwise)


@pytest.mark.parametrize('columnwise', [False, True], ids=['whole', 'columns'])
def test_moments_strided(torch, ingest, columnwise):
  arrays, truth = moment_case(SWEEP_MOMENT_CASES[3])
  views = [strided(torch, a) for a in arrays]
  check_moments(ingest.find_mean_std(views, columnwise=columnwise), truth[columnwise], arrays, columnwise)


@pytest.mark.parametrize('case', hi.G19_MOMENT_CASES, ids=[c[0] for c in hi.G19_MOMENT_CASES])
def test_moments_against_the_reference(torch, ingest, g19, case):
  """No further from the truth than the reference's own result is, plus the bound above."""
  name = case[0]
  arrays, truth = moment_case(case)
  assert np.allclose(hi.checksum(np.concatenate(arrays)), g19['moments_%s_xsum' % name], rtol=1e-12, atol=0)
  for columnwise in (False, True):
    if columnwise:
      r_mean, r_std = g19['moments_%s_mean' % name], g19['moments_%s_std' % name]
    else:
      r_mean, r_std = g19['moments_%s_all' % name]
    t_mean, t_std = truth[columnwise]
    check_moments(ingest.find_mean_std(arrays, columnwise=columnwise), truth[columnwise], arrays, columnwise,
                  slack_mean=np.abs(r_mean - t_mean), slack_std=np.abs(r_std - t_std))


# ---------------------------------------------------------------- normalise
@pytest.mark.parametrize('rows', [1, 65, 4097])
@pytest.mark.parametrize('width', [1, 148])
def test_normalize_bits(torch, ingest, rows, width):
  rng = np.random.default_rng(rows + width)
  a32 = (3e3 + 40 * rng.standard_normal((rows, width))).astype(np.float32)
  a64 = 3e3 + 40 * rng.standard_normal((rows, width))
  col_mean, col_std = 3e3 + rng.standard_normal((1, width)), 40 + rng.random((1, width))
  cases = [(a32, np.float32(3001.25), np.float32(39.7), np.float32),        # float32 scalars
           (a32, np.float64(3000.1), np.float64(40.3), None),               # float64 scalars
           (a32, 3000.1, 40.3, np.float32),                                 # Python floats
           (a64, np.float64(3000.1), np.float64(40.3), np.float64),
           (a32, col_mean, col_std, np.float64), (a64, col_mean, col_std, np.float64),
           (a32, col_mean.astype(np.float32), col_std.astype(np.float32), np.float32),
           (a32, np.float64(3000.1), 0.0, None), (a64, col_mean, np.zeros((1, width)), np.float64)]
  for a, mean, std, dtype in cases:
    want = (a - mean) / std if np.max(np.abs(std)) > 0 else a - mean
    if dtype is not None:
      assert want.dtype == dtype
    got = ingest.normalize_data(a, mean, std)
    assert isinstance(got, np.ndarray) and hi.same_bits(got, want)
    got = ingest.normalize_data(torch.from_numpy(a).cuda(), mean, std)
    assert isinstance(got, torch.Tensor) and got.is_cuda and hi.same_bits(got.cpu().numpy(), want)
  view = strided(torch, a32)
  assert hi.same_bits(ingest.normalize_data(view, 3000.1, 40.3).cpu().numpy(), (a32 - 3000.1) / 40.3)
  flat = a64[:, 0].copy()
  assert hi.same_bits(ingest.normalize_data(flat, 3000.1, 40.3), (flat - 3000.1) / 40.3)


# ---------------------------------------------------------------- end to end
def test_experiment_end_to_end(torch, ingest, tmp_path):
  """Two trials of device tensors, uneven lengths, one with an EEG offset: z_score_all_data,
  assemble_brain_data, write_all_data; every file against the float64 restatement of the same steps."""
  rng = np.random.default_rng(11)
  sr = 64
  spec = {'t1': (1000, 1003, None), 't2': (1037 + sr, 1030, 1.0)}
  raw, trials = {}, {}
  for name, (n_eeg, n_int, offset) in spec.items():
    c1 = (1e4 + 30 * rng.standard_normal(n_eeg)).astype(np.float32)
    c2 = -500 + 5 * rng.standard_normal((n_eeg + 3, 2))
    intensity = 7 + 2 * rng.standard_normal((n_int, 1))
    raw[name] = (c1, c2, intensity)
    df = ingest.MemoryBrainDataFile({'C1': torch.from_numpy(c1).cuda(), 'C2': torch.from_numpy(c2).cuda()}, sr)
    trials[name] = [{'intensity': torch.from_numpy(intensity).cuda()}, df]
  exp = ingest.BrainExperiment(trials, str(tmp_path), str(tmp_path), frame_rate=sr)
  exp.load_all_data()
  exp.trial_data('t2').fix_eeg_offset(1.0)
  exp.z_score_all_data()
  for trial in exp.iterate_trials():
    assert trial.model_features['intensity'].is_cuda
    trial.assemble_brain_data('C2, C1')
    eeg = trial.model_features['eeg']
    assert eeg.is_cuda and eeg.dtype == torch.float32
  files = exp.write_all_data(str(tmp_path))
  assert [os.path.basename(f) for f in files] == ['t1.tfrecords', 't2.tfrecords']

  both = np.concatenate([raw[n][2] for n in spec])
  mean, std = hi.moments_truth([both], False)
  for name, path in zip(spec, files):
    c1, c2, intensity = raw[name]
    drop = sr if spec[name][2] else 0
    eeg = np.concatenate((c1[drop:, None].astype(np.float64), c2[drop:len(c1)]), axis=1)    # brain_data's order
    frames = min(len(eeg), len(intensity))
    assert frames == {'t1': 1000, 't2': 1030}[name]
    assert ingest.count_tfrecords(path) == (frames, False)
    back = tfrecord.read_file(path, verify=True)
    assert back['eeg'].shape == (frames, 3) and back['intensity'].shape == (frames, 1)
    assert hi.ulp_distance32(back['eeg'], eeg[:frames].astype(np.float32)).max() <= 1
    want = ((intensity[:frames] - mean) / std).astype(np.float32)
    assert hi.ulp_distance32(back['intensity'], want).max() <= 1
  assert abs(exp._feature_mean['intensity'] - mean) <= 1e-12 * np.mean(np.abs(both))
  assert abs(exp._feature_std['intensity'] - std) <= 1e-12 * std
  exp.save_zscore_data(str(tmp_path / 'zscore.pkl'))
  with open(str(tmp_path / 'zscore.pkl'), 'rb') as f:
    saved = pickle.load(f)
  assert saved == {'mean': {'intensity': exp._feature_mean['intensity']},
                   'std': {'intensity': exp._feature_std['intensity']}}
  assert type(saved['mean']['intensity']) is np.float64
