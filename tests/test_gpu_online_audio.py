"""The online audio front end on the GPU (td_audio_online_push, online.OnlineAudioFeatures): recordings of 3000 rows
of seeded int16 draws cut into pushes every way -- float64 frames, float32 frames, the window read-back and the live
tail copy byte for byte --; the integer input making every window sum exact, the float64 frames against
tests/host_audio.window_means_exact after finish's arithmetic and against the batch AudioFeatures.compute_intensity
of the whole recording on the device, byte for byte; non-integer float32 input against the exactly summed
restatement within 1e-12 x max (float32 frames: that plus 2^-23 max|ref|); non-finite input; the workgroup edges, a
bank with strides, the plumbing, every invalid argument, and the hand-off through online.FrameJoin into an
OnlineDecoder."""
import numpy as np
import pytest

from tests import host_online
from tests import host_online_audio as hoa
from tests import host_online_pre
from tests import parity_log

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROWS = hoa.ROWS
FAST = (1, 2, 0.5, 0, -1)                       # numpy's scalar-power fast paths: no pow() in finish
# (fs_in, fs_out, window, exponent, channels, input dtype): spans of 63, 64 and 65 rows, 250 rows, empty and 1-row
# spans with NaNs, upsampling, overlapping spans with held frames; every channel count and input type at least once
CASES = [(6300, 100, 1, 1, 1, 'int16'), (6400, 100, 1, 1, 2, 'float32'), (6500, 100, 1, 0.5, 3, 'float64'),
         (16000, 64, 1, 1, 2, 'int16'), (100, 64, 0.1, 1, 8, 'float32'), (64, 100, 1.5, 2, 1, 'float64'),
         (16000, 64, 1.5, 1, 8, 'int16'), (16000, 64, 3, hoa.LOG10_2, 2, 'int16')]
IDS = ['%d_to_%d_w%g_e%.3g_c%d_%s' % case for case in CASES]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


class Bank(object):
  """S sessions of one configuration on the device, and a walk over a cut of the recording through
  device.audio_online_push."""

  def __init__(self, dev, params, x, x_pad=0, state_pad=0):
    import torch
    self.dev, self.h = dev, dev.default_handle()
    self.fs_in, self.fs_out, self.window, self.exponent = params
    x = np.asarray(x)
    x = x[None] if x.ndim == 2 else x
    self.s, self.n, self.c = x.shape
    # (x_pad: extra columns and rows between the sessions, so that neither stride is the packed one)
    full = torch.zeros((self.s, self.n + x_pad, self.c + x_pad), dtype=getattr(torch, x.dtype.name),
                       device=self.h.device)
    full[:, :self.n, :self.c] = torch.from_numpy(np.array(x)).to(self.h.device)
    self.x = full[:, :self.n, :self.c]
    self.k = dev.audio_online_plan(0, 0, self.fs_in, self.fs_out, self.window).tail_rows
    self.nbytes = dev.audio_online_state_bytes(self.c, self.k)
    self.state_pad = state_pad

  def run(self, sizes, flush_apart, fill=0):
    """Pushes of the given sizes, the last one flushing (or a flush of its own behind them): the outputs and the
    windows concatenated along the frames, the live tail copy and the plans."""
    import torch
    dev, h = self.dev, self.h
    block = torch.full((self.s, self.nbytes + self.state_pad), fill, dtype=torch.uint8, device=h.device)
    state = block[:, :self.nbytes]
    state.zero_()
    outs, at, live = [], 0, 0
    sizes = list(sizes) + ([0] if flush_apart else [])
    for i, n in enumerate(sizes):
      out = dev.audio_online_push(self.x[:, at:at + n] if n else None, self.fs_in, self.fs_out, self.window,
                                  self.exponent, state, live, at, c=self.c, flush=i == len(sizes) - 1, want64=True,
                                  windows=True, handle=h)
      assert out.plan.frames_before == sum(int(o.out32.shape[1]) for o in outs)
      assert out.live == (1 - live if n else live)
      live = out.live
      outs.append(out)
      at += n
    assert at == self.n
    if self.state_pad:
      assert bool((block[:, self.nbytes:] == fill).all())
    tail = state.contiguous().view(torch.float32).reshape(self.s, 2, self.k, self.c)[:, live]
    return dict(out32=torch.cat([o.out32 for o in outs], dim=1).cpu().numpy(),
                out64=torch.cat([o.out64 for o in outs], dim=1).cpu().numpy(),
                win=torch.cat([o.windows for o in outs], dim=0).cpu().numpy(),
                state=tail.cpu().numpy().copy(), plans=[o.plan for o in outs])


def _same(got, want, what):
  for key in ('out64', 'out32', 'win', 'state'):
    assert got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
    assert got[key].tobytes() == want[key].tobytes(), (what, key)


def _dist(got, want):
  """max |got - want| / max |want| over the finite entries; NaN and inf positions exact."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions differ'
  assert np.array_equal(np.isposinf(got), np.isposinf(want)), '+inf positions differ'
  ok = np.isfinite(want)
  if not ok.any():
    return 0.0
  return float(np.max(np.abs(got[ok] - want[ok]))) / float(np.max(np.abs(want[ok])))


_WHOLE = {}


def _case(dev, case):
  """(x, Bank, the whole recording in one push, the oracle's frames and windows): once per case, read-only."""
  if case not in _WHOLE:
    fs_in, fs_out, window, exponent, c, dtype = case
    x = hoa.recording(c, dtype)
    bank = Bank(dev, case[:4], x)
    _WHOLE[case] = (x, bank, bank.run([ROWS], False)) + hoa.oracle(x, fs_in, fs_out, window, exponent)
  return _WHOLE[case]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_any_cut_of_the_recording_gives_the_same_bits(dev, case):
  """float64 frames, float32 frames, the window read-back and the live tail copy, byte for byte: one push of
  everything; 3000 pushes of one row (every span straddles the seam between the tail and the push at every
  position); pushes of 1, 63, 64, 65, K - 1, K, K + 1 and the rest; a seeded random cut with empty pushes -- ended
  by a flushing last push and by a flush of its own."""
  x, bank, whole, want, _ = _case(dev, case)
  assert whole['out64'].shape == whole['out32'].shape == (1,) + want.shape
  assert whole['out32'].tobytes() == whole['out64'].astype(np.float32).tobytes()
  assert bank.k == hoa.tail_rows(*case[:3])
  cuts = hoa.cuts(ROWS, bank.k, seed=case[4])
  assert 0 in cuts['random'][0] and len(cuts) == 7
  for name, (sizes, flush_apart) in sorted(cuts.items()):
    _same(bank.run(sizes, flush_apart), whole, name)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_integer_input_gives_the_exact_envelope_of_the_whole_recording(dev, case):
  """Integer input: every float32 square is an integer and every window sum exact in float64, whatever its order.
  The windows are the whole recording's (HostAudioFeatures.windows), the tail copy holds the last K squares, and
  the float64 frames equal window_means_exact followed by finish's arithmetic -- byte for byte where the exponent
  is one of numpy's fast paths; with log10(2) the device's pow and the host's may differ in the last place, so that
  case is held to 1e-12 x max here and to the batch kernel's bytes in the next test."""
  x, bank, whole, want, want_win = _case(dev, case)
  fs_in, fs_out, window, exponent, c, _ = case
  np.testing.assert_array_equal(whole['win'], want_win)
  sq = np.asarray(x).astype(np.float32)
  np.testing.assert_array_equal(whole['state'][0], np.concatenate([np.zeros((bank.k, c), np.float32), sq * sq])[-bank.k:])
  if (fs_in, fs_out) == (100, 64):
    assert np.isnan(want).any() and not np.isnan(want).all()      # empty and 1-row spans
  if exponent in FAST:
    np.testing.assert_array_equal(whole['out64'][0], want)        # (NaN positions included)
  else:
    assert _dist(whole['out64'][0], want) <= TOL


@pytest.mark.parametrize('params,c,dtype', [((6400, 100, 1, 1), 2, 'float32'), ((6500, 100, 1.5, hoa.LOG10_2), 4, 'float64'),
                                            ((16000, 64, 3, hoa.LOG10_2), 2, 'float32')],
                         ids=['6400_c2_e1', '6500_w1.5_c4_elog', '16000_w3_c2_elog'])
def test_it_is_the_batch_kernels_envelope_of_the_whole_recording(dev, params, c, dtype):
  """AudioFeatures(...).compute_intensity(whole) on a fresh object, on the device: the same float64 bytes as the
  online frames of a cut (integer input: both sums are exact, and sqrt, the division and pow are the same code)."""
  import torch
  from telluride_decoding_amd import preprocess
  x = hoa.recording(c, dtype)
  got = Bank(dev, params, x).run(hoa.cuts(ROWS, hoa.tail_rows(*params[:3]), seed=5)['edges'][0], True)
  xd = torch.from_numpy(np.array(x)).to(dev.default_handle().device)
  want = preprocess.AudioFeatures('a', *params).compute_intensity(xd)
  assert want.is_cuda and want.dtype == torch.float64
  want = want.cpu().numpy()
  assert got['out64'].shape == (1,) + want.shape
  assert got['out64'][0].tobytes() == want.tobytes()


@pytest.mark.parametrize('params', [(16000, 64, 1, 1), (6500, 100, 1.5, hoa.LOG10_2), (6300, 100, 1, 0.5),
                                    (100, 64, 0.1, 1)], ids=['16000_64', '6500_w1.5_elog', '6300_e.5', '100_64_w.1'])
def test_noise_is_cut_invariant_and_within_1e_12_of_the_exact_restatement(dev, params):
  """Non-integer float32 input, 2 channels: the cuts byte for byte; the float64 frames within 1e-12 x max of the
  exactly summed restatement (math.fsum per window), the float32 frames within that plus 2^-23 max|ref|."""
  x = hoa.noise(2)
  bank = Bank(dev, params, x)
  whole = bank.run([ROWS], False)
  cuts = hoa.cuts(ROWS, bank.k, seed=11)
  for name in ('edges', 'random', 'whole_flush_apart'):
    _same(bank.run(*cuts[name]), whole, name)
  want, want_win = hoa.oracle(x, *params)
  np.testing.assert_array_equal(whole['win'], want_win)
  d64 = _dist(whole['out64'][0], want)
  d32 = _dist(whole['out32'][0], want)
  bound32 = TOL + 2.0 ** -23
  name = '%d_to_%d_w%g_e%.3g' % params
  parity_log.record('online_audio_noise_%s' % name, out64=d64, out32=d32, bound32=bound32)
  print('online audio %s: float64 %.3g, float32 %.3g (bound %.3g) of max|ref|' % (name, d64, d32, bound32))
  assert d64 <= TOL and d32 <= bound32, (d64, d32, bound32)


def test_non_finite_input_keeps_its_positions(dev):
  x = np.array(hoa.noise(2))
  x[700, 0], x[1500, 1], x[2200, 0] = np.inf, np.nan, -np.inf
  params = (6400, 100, 1.5, 1)
  want, _ = hoa.oracle(x, *params)
  bank = Bank(dev, params, x)
  got = bank.run([699, 2, 1, 1000, 1298], True)
  _same(got, bank.run([ROWS], False), 'non-finite')
  assert np.isinf(want).sum() >= 2 and np.isnan(want).sum() >= 1
  d = _dist(got['out64'][0], want)              # (asserts the NaN and inf positions)
  assert d <= TOL


def test_workgroup_edges_and_pushes_around_the_tail(dev):
  """6400 -> 100, window 1 (K = 66, 4 frames per workgroup); every run's frames are the first frames of the whole
  recording's.  A push that emits no frame; pushes that emit 3, 4 and 5 frames; a push longer than K behind a push
  shorter than K; pushes of K - 1, K and K + 1 rows behind one another."""
  case = CASES[1]
  x, bank, whole, _, _ = _case(dev, case)
  k = bank.k
  assert k == 66

  def run(sizes):
    got = Bank(dev, case[:4], x[:sum(sizes)]).run(sizes, True)
    m = got['out64'].shape[1]
    sure = sum(p.frames_after - p.frames_before for p in got['plans'][:-1])      # (the flush clamps at its own end)
    assert got['out64'][:, :sure].tobytes() == whole['out64'][:, :sure].tobytes(), sizes
    assert got['out32'][:, :sure].tobytes() == whole['out32'][:, :sure].tobytes(), sizes
    assert got['win'][:sure].tobytes() == whole['win'][:sure].tobytes(), sizes
    assert m == hoa.frames_of(sum(sizes), *case[:2])
    return [p.frames_after - p.frames_before for p in got['plans']]

  def rows_for(frames, before=0):
    n = 0
    while dev.audio_online_plan(before, n, *case[:3]).frames_after - dev.audio_online_plan(
        before, 0, *case[:3]).frames_before < frames:
      n += 1
    return n

  assert run([31, 1])[:2] == [0, 0]                            # u_0 = 32, F(32) = 0
  for frames in (3, 4, 5):
    n = rows_for(frames)
    assert run([n])[0] == frames and run([10, n - 10])[:2] == [0, frames]
  run([k - 20, 3 * k + 5, 7])
  run([k - 1, k, k + 1, 1, k + 1, k, k - 1])
  run([5, 4 * k, 5, 4 * k])


def test_a_bank_is_its_sessions(dev):
  """Three sessions with row and session strides that are not the packed ones and a padded state stride, in one
  call == three calls of one session; one shared AudioFeatures == three copies."""
  from telluride_decoding_amd import online
  params = (16000, 64, 1.5, 0.5)
  x = hoa.recording(2, 'int16', sessions=3)
  sizes = [37, 0, 250, 1, 2712]
  bank = Bank(dev, params, x, x_pad=3, state_pad=24)
  assert bank.x.stride(1) == 5 and bank.x.stride(0) == 5 * (ROWS + 3)
  got = bank.run(sizes, True, fill=7)
  for i in range(3):
    one = Bank(dev, params, x[i]).run(sizes, True)
    for key in ('out32', 'out64', 'state'):
      assert got[key][i].tobytes() == one[key][0].tobytes(), (i, key)
    assert got['win'].tobytes() == one['win'].tobytes()
  assert got['out64'][0].tobytes() != got['out64'][1].tobytes()
  f = hoa.features(*params)
  h = dev.default_handle()
  import torch
  xd = torch.from_numpy(np.array(x)).to(h.device)
  assert xd.dtype == torch.int16
  shared = hoa.run_audio(online.OnlineAudioFeatures(f, num_sessions=3), xd, sizes)
  copies = hoa.run_audio(online.OnlineAudioFeatures([f, hoa.features(*params), f]), xd, sizes)
  assert shared[1].tobytes() == copies[1].tobytes() == got['out64'].tobytes()
  assert shared[0].tobytes() == copies[0].tobytes() == got['out32'].tobytes()


def test_one_launch_per_push_reset_and_the_same_bits_twice(dev):
  """online.OnlineAudioFeatures: 1 launch per push, 0 for an empty one; two runs give the same bytes; a reset in the
  middle of a recording equals a fresh object; host arrays and device tensors give the same frames."""
  from telluride_decoding_amd import online
  params = (16000, 64, 1, 1)
  x = hoa.recording(2, 'int16')
  import torch
  h = dev.default_handle()
  xd = torch.from_numpy(np.array(x)).to(h.device)
  assert xd.dtype == torch.int16
  runs = []
  obj = online.OnlineAudioFeatures(hoa.features(*params))
  for attempt in range(2):
    out = []
    h.profile_enable(True)
    h.profile_read()
    at = 0
    for n in (5, 0, 1, 37, 250, 2707):
      out.append(obj.push(xd[at:at + n], want64=True))
      assert h.profile_read()[0] == (1 if n else 0), n
      at += n
    out.append(obj.flush(want64=True))
    assert h.profile_read()[0] <= 1
    h.profile_enable(False)
    assert all(o[0].is_cuda and o[1].is_cuda for o in out)
    runs.append((np.concatenate([o[0].cpu().numpy() for o in out], axis=1),
                 np.concatenate([o[1].cpu().numpy() for o in out], axis=1), obj.state.cpu().numpy()))
    assert (obj.rows_pushed, obj.frames_emitted) == (ROWS, runs[-1][0].shape[1]) == (ROWS, 12)
    with pytest.raises(ValueError, match='flushed'):
      obj.push(xd[:1])
    if attempt == 0:                    # a reset in the middle of the next recording, then the recording
      obj.reset()
      obj.push(xd[:777])
      obj.reset()
  for a, b in zip(*runs):
    assert a.tobytes() == b.tobytes()
  assert runs[0][2].shape == (1, 252, 2) and runs[0][2].dtype == np.float32
  host = hoa.run_audio(online.OnlineAudioFeatures(hoa.features(*params)), np.asarray(x), [1500, 1500])
  assert isinstance(host[0], np.ndarray) and host[0].tobytes() == runs[0][0].tobytes()
  assert host[1].tobytes() == runs[0][1].tobytes()


def test_invalid_arguments_queue_nothing(dev):
  """Every TD_ERR_INVALID of the header, through the C interface: nothing is launched and the state stays."""
  import ctypes
  import torch
  h = dev.default_handle()
  c, n = 2, 600
  k = dev.audio_online_plan(0, 0, 16000, 64, 1).tail_rows
  nbytes = dev.audio_online_state_bytes(c, k)
  x = h.zeros((2, n, c)) + 3.0
  state = torch.full((2, nbytes), 7, dtype=torch.uint8, device=h.device)
  out32, out64 = h.zeros((2 * n * c,)), h.zeros((2 * n * c,), 'float64')     # (room for the widest call below)
  win = torch.zeros((n, 2), dtype=torch.int64, device=h.device)
  p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
  good = dict(h=h.ptr, sessions=2, x=p(x), x_type=1, ldx=c, x_ss=n * c, n=n, c=c, before=0, flush=0, fs_in=16000.0,
              fs_out=64.0, window=1.0, exponent=1.0, state=p(state), state_ss=nbytes, live=0, out32=p(out32),
              out64=p(out64), ldout=c, out_ss=n * c, win=p(win))
  inf, nan = float('inf'), float('nan')
  bad = [dict(h=None), dict(sessions=0), dict(sessions=65536), dict(x=None), dict(state=None),
         dict(out32=None, out64=None), dict(c=0), dict(c=9), dict(x_type=-1), dict(x_type=3), dict(fs_in=0.0),
         dict(fs_out=-1.0), dict(fs_in=inf), dict(fs_out=nan), dict(window=0.0), dict(window=-1.0), dict(window=inf),
         dict(window=nan), dict(fs_in=64.0, fs_out=64.0), dict(fs_in=64.0, fs_out=100.0, window=0.5),
         dict(fs_in=48000.0, window=11.0), dict(n=-1), dict(n=(1 << 20) + 1), dict(fs_in=16000.0, fs_out=1e9, window=2.0),
         dict(before=-1), dict(live=-1), dict(live=2), dict(ldx=c - 1), dict(ldout=c - 1), dict(x_ss=c - 1),
         dict(out_ss=c - 1), dict(state_ss=nbytes - 8), dict(state_ss=nbytes + 4)]
  h.profile_enable(True)
  h.profile_read()
  for change in bad:
    args = dict(good, **change)
    assert h.lib.td_audio_online_push(*args.values()) == -1, change
  assert h.profile_read()[0] == 0
  assert bool((state == 7).all())
  # (and the call the changes were made to is a good one; either output alone and no read-back; an empty push queues
  # nothing)
  state.zero_()
  assert h.lib.td_audio_online_push(*good.values()) == 0
  assert h.lib.td_audio_online_push(*dict(good, out32=None, win=None, before=n, live=1).values()) == 0
  assert h.lib.td_audio_online_push(*dict(good, out64=None, before=2 * n, live=0, x_type=0, ldx=2 * c,
                                          x_ss=2 * n * c).values()) == 0
  assert h.profile_read()[0] == 3
  assert h.lib.td_audio_online_push(*dict(good, n=0, x=None, before=3 * n, live=1).values()) == 0
  assert h.profile_read()[0] == 0
  h.profile_enable(False)
  assert bool(state.any())


def test_the_hand_off_into_an_online_decoder(dev):
  """Raw EEG through OnlinePreprocessor, stereo int16 audio through OnlineAudioFeatures, the two cut by independent
  seeded chunk sizes, joined by FrameJoin into a linear OnlineDecoder: every tensor on the way is a device tensor,
  and the scores and decisions are those of ONE push of the whole-recording front-end output with the
  whole-recording envelopes (the batch AudioFeatures.compute_intensity on the device), byte for byte."""
  import torch
  from telluride_decoding_amd import online, preprocess
  c, pre, post = 5, 2, 9
  rec = host_online.recipe(c, pre, post)
  decoder = host_online.linear_decoder(c, pre, post, rec['w'], rec['b'], rec['corr'][0])
  h = dev.default_handle()
  frames = 300
  raw = np.repeat(rec['eeg'][:frames], 10, axis=0) + np.float32(2.0)            # 1 kHz -> 100 Hz: 3000 raw rows
  kw = dict(fs_in=1000, fs_out=100, highpass_cutoff=0.5, highpass_order=4, data_mean=0.0, data_std=1.0)
  params = (4000, 100, 1.5, 1)                                                  # 12000 audio rows -> 300 frames
  pcm = np.random.default_rng(9).integers(-20000, 20001, size=(40 * frames, 2)).astype(np.int16)
  rawd, pcmd = h.to_device(raw), torch.from_numpy(pcm).to(h.device)
  assert pcmd.dtype == torch.int16

  # the whole recording, each stream in one piece
  whole_front = online.OnlinePreprocessor(host_online_pre.make(kw))
  eeg_whole = torch.cat([whole_front.push(rawd), whole_front.flush()], dim=1)
  env_whole = preprocess.AudioFeatures('a', *params).compute_intensity(pcmd).to(torch.float32)
  assert tuple(eeg_whole.shape) == (1, frames, c) and tuple(env_whole.shape) == (frames, 2)
  once = online.OnlineDecoder(decoder, 37, 11)
  a = once.push(eeg_whole, env_whole[:, 0], env_whole[:, 1])
  b = once.flush()
  want_scores = np.concatenate([a.scores[0], b.scores[0]])
  want_decisions = np.concatenate([a.decisions[0], b.decisions[0]])
  assert want_scores.shape == ((frames - 37) // 11 + 1, 2)

  def chunks(total, most, seed):
    rng, sizes = np.random.default_rng(seed), []
    while sum(sizes) < total:
      sizes.append(int(min(rng.integers(0, most), total - sum(sizes))))
    return sizes

  raw_sizes, pcm_sizes = chunks(len(raw), 400, 1), chunks(len(pcm), 1500, 2)
  assert raw_sizes != pcm_sizes
  front = online.OnlinePreprocessor(host_online_pre.make(kw))
  audio = online.OnlineAudioFeatures(hoa.features(*params))
  join = online.FrameJoin(3)
  live = online.OnlineDecoder(decoder, 37, 11)
  scores, decisions, at_raw, at_pcm, joined = [], [], 0, 0, 0

  def decode(blocks):
    for t in blocks:
      assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    r = live.push(*blocks)
    scores.append(r.scores[0]); decisions.append(r.decisions[0])
    return int(blocks[0].shape[1])

  for i in range(max(len(raw_sizes), len(pcm_sizes))):
    n_raw = raw_sizes[i] if i < len(raw_sizes) else 0
    n_pcm = pcm_sizes[i] if i < len(pcm_sizes) else 0
    eeg = front.push(rawd[at_raw:at_raw + n_raw])
    env = audio.push(pcmd[at_pcm:at_pcm + n_pcm])
    assert eeg.is_cuda and env.is_cuda and env.dtype == torch.float32
    joined += decode(join.push(eeg, env[..., 0], env[..., 1]))
    at_raw, at_pcm = at_raw + n_raw, at_pcm + n_pcm
  assert (at_raw, at_pcm) == (len(raw), len(pcm))
  eeg, env = front.flush(), audio.flush()
  rest = join.flush(eeg, env[..., 0], env[..., 1])
  assert rest.beyond == [0, 0, 0]
  joined += decode(rest.blocks)
  assert joined == frames and join.frames_delivered == [frames] * 3
  r = live.flush()
  scores.append(r.scores[0]); decisions.append(r.decisions[0])
  assert np.concatenate(scores).tobytes() == want_scores.tobytes()
  assert np.concatenate(decisions).tobytes() == want_decisions.tobytes()
