"""The online front end on the GPU (td_frontend_push, online.OnlinePreprocessor): recordings of 3000 raw rows cut
into pushes every way -- float32 output, float64 output and the final state block byte for byte --, every output row
and the filter state against tests/host_preprocess.HostPreprocessor on the whole recording at the bounds of
tests/test_gpu_preprocess_sweep.py (float64 and the state within 1e-9 max|x|, float32 within that plus
2^-23 max|ref|; nothing set aside), the unfiltered chain against Preprocessor.process byte for byte, the pass edges
and the held frame, a bank with strides, and the plumbing up to the hand-off into an OnlineDecoder."""
import numpy as np
import pytest

from tests import host_online
from tests import host_online_pre as ho
from tests import parity_log

pytestmark = pytest.mark.gpu

TOL = 1e-9
ROWS = ho.ROWS
# (channels, sections, fs_in, fs_out, input dtype): every value of every axis at least once
CASES = [(64, 7, 1000, 64, 'float32'), (1, 0, 250, 250, 'float64'), (5, 1, 250, 250, 'float32'),
         (63, 2, 64, 100, 'float32'), (65, 16, 1000, 100, 'float64'), (128, 7, 1000, 100, 'float32')]
IDS = ['c%d_s%d_%d_to_%d_%s' % case for case in CASES]


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


class Bank(object):
  """S sessions of one configuration on the device, and a walk over a cut of the recording through
  device.frontend_push."""

  def __init__(self, dev, kw, x, stats=None, x_pad=0, state_pad=0):
    import torch
    from telluride_decoding_amd import online
    self.dev, self.h = dev, dev.default_handle()
    h = self.h
    x = np.asarray(x)
    x = x[None] if x.ndim == 2 else x
    self.s, self.n, self.c = x.shape
    self.cfg = online.frontend_parameters(ho.make(kw))
    self.groups = online.frontend_groups(self.cfg, self.c)
    self.sections = 0 if self.cfg['sos'] is None else int(self.cfg['sos'].shape[0])
    # (x_pad: extra columns and rows between the sessions, so that neither stride is the packed one)
    full = torch.zeros((self.s, self.n + x_pad, self.c + x_pad), dtype=getattr(torch, x.dtype.name), device=h.device)
    full[:, :self.n, :self.c] = torch.from_numpy(np.array(x)).to(h.device)      # (a copy: the recording is read-only)
    self.x = full[:, :self.n, :self.c]
    stats = [(self.cfg['mean'], self.cfg['std'])] if stats is None else stats
    self.mean = h.to_device(np.array([[m] for m, _ in stats], np.float64), np.float64).reshape(-1)
    self.std = h.to_device(np.array([[s] for _, s in stats], np.float64), np.float64).reshape(-1)
    self.nbytes = dev.frontend_state_bytes(self.c, self.sections)
    self.state_pad = state_pad

  def run(self, sizes, flush_apart, fill=0):
    """Pushes of the given sizes, the last one flushing (or a flush of its own behind them): both outputs
    concatenated along the frames, the final state blocks and the plans."""
    import torch
    dev, h, cfg = self.dev, self.h, self.cfg
    block = torch.full((self.s, self.nbytes + self.state_pad), fill, dtype=torch.uint8, device=h.device)
    state = block[:, :self.nbytes]
    state.zero_()
    outs, at = [], 0
    sizes = list(sizes) + ([0] if flush_apart else [])
    for i, n in enumerate(sizes):
      out = dev.frontend_push(self.x[:, at:at + n] if n else None, cfg['sos'], cfg['split'], cfg['zi'], cfg['fs_in'],
                              cfg['fs_out'], self.groups, cfg['select'], self.mean, self.std, state, at, c=self.c,
                              flush=i == len(sizes) - 1, want64=True, handle=h)
      assert out.plan.frames_before == sum(int(o.out32.shape[1]) for o in outs)
      outs.append(out)
      at += n
    assert at == self.n
    if self.state_pad:
      assert bool((block[:, self.nbytes:] == fill).all())
    return dict(out32=torch.cat([o.out32 for o in outs], dim=1).cpu().numpy(),
                out64=torch.cat([o.out64 for o in outs], dim=1).cpu().numpy(),
                state=state.cpu().numpy().copy(), plans=[o.plan for o in outs])


def _same(got, want, what):
  for key in ('out32', 'out64', 'state'):
    assert got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
    assert got[key].tobytes() == want[key].tobytes(), (what, key)


_WHOLE = {}


def _case(dev, case):
  """(kw, x, Bank, the whole recording in one push): computed once per case and shared, read-only."""
  if case not in _WHOLE:
    c, sections, fs_in, fs_out, dtype = case
    kw = ho.config(sections, fs_in, fs_out, c)
    assert ho.sections_of(kw) == sections
    x = ho.recording(c, fs_in, dtype)
    bank = Bank(dev, kw, x)
    _WHOLE[case] = (kw, x, bank, bank.run([ROWS], False))
  return _WHOLE[case]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_any_cut_of_the_recording_gives_the_same_bits(dev, case):
  """float32 output, float64 output and the final state block, byte for byte: one push of everything, pushes of 1,
  7, 9, 10, 11, 63, 64, 65, 500 and the rest, a seeded random cut with empty pushes -- ended by a flushing last
  push and by a flush of its own --; the 7-section 64-channel 1000 -> 64 case also takes 3000 pushes of one row."""
  from telluride_decoding_amd import preprocess
  kw, x, bank, whole = _case(dev, case)
  frames = len(preprocess.resample_indices(ROWS, case[2], case[3])[0]) if case[2] != case[3] else ROWS
  assert whole['out32'].shape == whole['out64'].shape == (1, frames, len(kw.get('channel_numbers') or range(case[0])))
  assert np.isfinite(whole['out64']).all() and whole['state'].any()
  assert whole['out32'].tobytes() == whole['out64'].astype(np.float32).tobytes()
  cuts = ho.cuts(ROWS, seed=case[0])
  assert 0 in cuts['random'][0]
  for name, (sizes, flush_apart) in sorted(cuts.items()):
    if name == 'ones' and case != CASES[0]:
      continue
    _same(bank.run(sizes, flush_apart), whole, name)


HARD_CASE = (4, 16, 1000, 1000, 'float32')


@pytest.mark.parametrize('case', CASES + [HARD_CASE], ids=IDS + ['s16_hard_0p01_1hz'])
def test_every_row_and_the_filter_state_against_the_oracle(dev, case):
  """HostPreprocessor(kw).process(whole, reset=True) and its .state(): the float64 output and the filter-state
  part of the state block within 1e-9 max|x|, the float32 output within that plus 2^-23 max|ref|, on every row."""
  if case == HARD_CASE:
    kw = dict(ho.HARD, data_mean=0.5, data_std=1)
    x = ho.recording(4, 1000, 'float32')
    got = Bank(dev, kw, x).run([1, 7, 9, 10, 11, 63, 64, 65, 500, ROWS - 730], True)
  else:
    kw, x, _, got = _case(dev, case)
  want, want_state = ho.oracle(kw, x)
  scale = float(np.max(np.abs(x)))
  assert got['out64'].shape == (1,) + want.shape
  d64 = float(np.max(np.abs(got['out64'][0] - want))) / scale
  d32 = float(np.max(np.abs(got['out32'][0].astype(np.float64) - want))) / scale
  bound32 = TOL + 2.0 ** -23 * float(np.max(np.abs(want))) / scale
  ds = 0.0
  if want_state is not None:
    state = got['state'].view(np.float64).reshape(-1, x.shape[1])[:-2].reshape(want_state.shape)
    ds = float(np.max(np.abs(state - want_state))) / scale
  name = 's16_hard_0p01_1hz' if case == HARD_CASE else IDS[CASES.index(case)]
  parity_log.record('online_pre_%s' % name, out64=d64, out32=d32, bound32=bound32, state=ds)
  print('online front end %s: float64 %.3g, float32 %.3g (bound %.3g), state %.3g of max|x|' %
        (name, d64, d32, bound32, ds))
  assert d64 <= TOL and d32 <= bound32 and ds <= TOL, (d64, d32, bound32, ds)


@pytest.mark.parametrize('fs_in,fs_out', [(1000, 64), (64, 100)])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_without_a_filter_it_is_preprocessor_process_byte_for_byte(dev, fs_in, fs_out, dtype):
  """Overlapping re-reference groups (one channel listed twice), a strided selection, no filter: the output over a
  cut is Preprocessor.process(whole) on the device, float32 and float64."""
  import torch
  c = 9
  kw = dict(fs_in=fs_in, fs_out=fs_out, data_mean=0.3, data_std=1.7, ref_channels=[[0, 1, 2], [2, 1, c - 1]],
            channels_to_ref=[[0, 1, c - 1], [1, 1, 2]], channel_numbers=list(range(0, c, 3)))
  if fs_out < fs_in:
    kw.update(lowpass_cutoff=0)               # (a Preprocessor adds its low-pass when downsampling: built, then removed)
  x = ho.recording(c, fs_in, dtype)
  prep = ho.make(kw)
  prep._lowpass_sos = prep._lowpass_zi = None
  assert prep.sos is None
  bank = Bank(dev, kw, x)
  bank.cfg['sos'], bank.cfg['zi'], bank.cfg['split'], bank.sections = None, None, 0, 0
  bank.nbytes = dev.frontend_state_bytes(c, 0)
  got = bank.run([1, 36, 0, 250, 713, 2000], True)
  xd = torch.from_numpy(np.array(x)).to(bank.h.device)
  for key, device_dtype in (('out32', 'float32'), ('out64', 'float64')):
    prep.device_dtype = device_dtype
    want = prep.process(xd, reset=True).cpu().numpy()
    assert got[key].shape == (1,) + want.shape and want.dtype == got[key].dtype
    assert got[key][0].tobytes() == want.tobytes(), key


def test_with_a_filter_against_process_on_one_chunk_of_its_plan(dev):
  """Reported, not required: on a recording that is ONE chunk of td_sos_filter's plan the batch route runs no scan,
  only the same recurrence with the compiler's choice of contractions.  The distance is held to the oracle's
  bound; whether the bytes are equal goes to the parity log."""
  import torch
  c = 4
  n, chunk = None, None
  for n in (256, 128, 64, 32, 16):
    chunk, _ = dev.sos_filter_plan(n, n, c)
    if chunk >= n:
      break
  assert chunk >= n
  kw = dict(fs_in=250, fs_out=250, highpass_cutoff=0.5, highpass_order=4, lowpass_cutoff=30, lowpass_order=6,
            data_mean=0.25, data_std=1.5)
  x = ho.recording(c, 250, 'float32')[:n]
  bank = Bank(dev, kw, x)
  got = bank.run([n], False)
  prep = ho.make(kw)
  prep.device_dtype = 'float64'
  want = prep.process(torch.from_numpy(np.array(x)).to(bank.h.device), reset=True).cpu().numpy()
  d = float(np.max(np.abs(got['out64'][0] - want))) / float(np.max(np.abs(x)))
  equal = got['out64'][0].tobytes() == want.tobytes()
  parity_log.record('online_pre_vs_process_one_chunk', rows=n, out64=d, bytes_equal=bool(equal))
  print('online front end vs Preprocessor.process on one chunk of %d rows: %.3g of max|x|, bytes equal: %s' %
        (n, d, equal))
  assert d <= TOL


def test_pass_edges_and_the_held_frame(dev):
  """1000 -> 100, 5 channels, 7 sections; every run's frames are the first frames of the whole recording's.  A
  push that emits exactly one pass (64 frames: 635 rows), then one that emits none (3 rows); one that emits a pass
  and one frame (646 rows); 14 rows hold frame 1 back (its row 10 is there, resample_indices(14) has 1 frame) and
  the next 2 rows emit it at the head of their push, from the state; a flush behind the 14 rows drops it."""
  kw = ho.config(7, 1000, 100, 5)
  x = ho.recording(5, 1000)
  whole = Bank(dev, kw, x).run([ROWS], False)
  assert dev.frontend_lds_bytes(5, 1, 64)[0] == 64

  def run(sizes, flush_apart):
    got = Bank(dev, kw, x[:sum(sizes)]).run(sizes, flush_apart)
    m = got['out32'].shape[1]
    assert got['out32'].tobytes() == whole['out32'][:, :m].tobytes(), sizes
    assert got['out64'].tobytes() == whole['out64'][:, :m].tobytes(), sizes
    return got, [p.frames_after - p.frames_before for p in got['plans']], [p.held for p in got['plans']]

  _, emitted, _ = run([635, 3, 2], False)
  assert emitted == [64, 0, 0]
  _, emitted, _ = run([646], False)
  assert emitted == [65]
  _, emitted, held = run([14, 2, 4], False)
  assert emitted == [1, 1, 0] and held == [1, 0, 0]
  got, emitted, held = run([14], True)
  assert emitted == [1, 0] and held == [1, 1] and got['out32'].shape[1] == 1
  # (and the state of 14 rows is the state of 14 rows, whatever held them)
  assert got['state'].tobytes() == Bank(dev, kw, x[:14]).run([1] * 14, False)['state'].tobytes()


def test_a_bank_is_its_sessions(dev):
  """Three sessions with their own mean / std, row and session strides that are not the packed ones and a padded
  state stride, in one call == three calls of one session; a shared mean / std (stride 0) == three copies."""
  kw = ho.config(7, 1000, 64, 5)
  x = np.stack([ho.recording(5, 1000) * np.float32(g) for g in (1.0, 2.0, -0.5)])
  stats = [(0.25, 1.5), (-1.0, 0.5), (0.0, 2.0)]
  sizes = [37, 0, 250, 1, 2712]
  bank = Bank(dev, kw, x, stats, x_pad=3, state_pad=24)
  assert bank.x.stride(1) == 8 and bank.x.stride(0) == 8 * (ROWS + 3)
  got = bank.run(sizes, True, fill=7)
  for i in range(3):
    one = Bank(dev, kw, x[i], stats[i:i + 1]).run(sizes, True)
    for key in ('out32', 'out64', 'state'):
      assert got[key][i].tobytes() == one[key][0].tobytes(), (i, key)
  assert got['out32'][0].tobytes() != got['out32'][1].tobytes()
  shared = Bank(dev, kw, x, stats[:1]).run(sizes, False)
  copies = Bank(dev, kw, x, stats[:1] * 3).run(sizes, False)
  _same(shared, copies, 'shared')


def test_one_launch_per_push_reset_and_the_same_bits_twice(dev):
  """online.OnlinePreprocessor: 1 launch per push, 0 for an empty one; two runs give the same bytes; a reset in the
  middle of a recording equals a fresh object; host arrays and device tensors give the same frames."""
  from telluride_decoding_amd import online
  kw = ho.config(7, 1000, 64, 64)
  x = ho.recording(64, 1000)
  h = dev.default_handle()
  xd = h.to_device(x)
  runs = []
  front = online.OnlinePreprocessor(ho.make(kw))
  for attempt in range(2):
    out = []
    h.profile_enable(True)
    h.profile_read()
    at = 0
    for n in (5, 0, 1, 37, 250, 2707):
      out.append(front.push(xd[at:at + n], want64=True))
      assert h.profile_read()[0] == (1 if n else 0), n
      at += n
    out.append(front.flush(want64=True))
    assert h.profile_read()[0] <= 1
    h.profile_enable(False)
    assert all(o[0].is_cuda and o[0].dtype.is_floating_point for o in out)
    runs.append((np.concatenate([o[0].cpu().numpy() for o in out], axis=1),
                 np.concatenate([o[1].cpu().numpy() for o in out], axis=1), front.state.cpu().numpy()))
    assert (front.rows_pushed, front.frames_emitted) == (ROWS, runs[-1][0].shape[1]) == (ROWS, 192)
    with pytest.raises(ValueError, match='flushed'):
      front.push(xd[:1])
    if attempt == 0:                    # a reset in the middle of the next recording, then the recording
      front.reset()
      front.push(xd[:777])
      front.reset()
  for a, b in zip(*runs):
    assert a.tobytes() == b.tobytes()
  assert runs[0][2].shape == (1, 2 * 7 + 2, 64)
  host = ho.run_front(online.OnlinePreprocessor(ho.make(kw)), x, [1500, 1500])
  assert isinstance(host[0], np.ndarray) and host[0].tobytes() == runs[0][0].tobytes()


def test_invalid_arguments_queue_nothing(dev):
  """Every TD_ERR_INVALID of the header, through the C interface: nothing is launched and the state stays."""
  import ctypes
  import torch
  h = dev.default_handle()
  c, cs, n, sections = 4, 2, 20, 2
  nbytes = dev.frontend_state_bytes(c, sections)
  x = h.zeros((2, n, c))
  mean, std = h.zeros((2,), 'float64'), h.zeros((2,), 'float64') + 1.0
  state = torch.full((2, nbytes), 7, dtype=torch.uint8, device=h.device)
  out32, out64 = h.zeros((2 * n * c,)), h.zeros((2 * n * c,), 'float64')     # (room for the widest call below)
  p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
  ints = lambda v: (ctypes.c_int * len(v))(*v)
  dbls = lambda v: (ctypes.c_double * len(v))(*v)
  sos = dbls([1, 2, 1, 1, -0.5, 0.1, 1, -2, 1, 1, -0.4, 0.2])
  good = dict(h=h.ptr, sessions=2, x=p(x), x_is_f64=0, ldx=c, x_ss=n * c, n=n, c=c, sos=sos, sections=sections,
              split=1, zi=dbls([0.1, 0.2, 0.3, 0.4]), fs_in=1000.0, fs_out=100.0, groups=1, ref_ptr=ints([0, 2]),
              ref_idx=ints([0, 3]), chan_ptr=ints([0, 2]), chan_idx=ints([1, 2]), sel=ints([3, 1]), cs=cs,
              mean=p(mean), std=p(std), stat_ss=1, before=0, flush=0, state=p(state), state_ss=nbytes, out32=p(out32),
              out64=p(out64), ldout=cs, out_ss=n * cs)
  bad_sos = dbls([1, 2, 1, 2, -0.5, 0.1, 1, -2, 1, 1, -0.4, 0.2])
  bad = [dict(h=None), dict(sessions=0), dict(x=None), dict(mean=None), dict(std=None), dict(state=None),
         dict(out32=None, out64=None), dict(sos=None), dict(zi=None), dict(ref_ptr=None), dict(ref_idx=None),
         dict(chan_ptr=None), dict(chan_idx=None), dict(c=0), dict(c=129), dict(cs=0), dict(cs=129),
         dict(sections=-1), dict(sections=17), dict(sos=bad_sos), dict(split=-1), dict(split=3), dict(fs_in=0.0),
         dict(fs_out=-1.0), dict(fs_in=float('inf')), dict(fs_out=float('nan')), dict(n=-1), dict(n=(1 << 20) + 1),
         dict(fs_in=1.0, fs_out=1e7), dict(before=-1), dict(groups=-1), dict(groups=33), dict(ref_ptr=ints([0, 0])),
         dict(ref_idx=ints([0, 4])), dict(ref_idx=ints([-1, 3])), dict(chan_idx=ints([1, 4])),
         dict(chan_ptr=ints([2, 0])), dict(sel=ints([3, 4])), dict(sel=ints([-1, 1])), dict(ldx=c - 1),
         dict(ldout=cs - 1), dict(x_ss=c - 1), dict(out_ss=cs - 1), dict(stat_ss=-1), dict(state_ss=nbytes - 8),
         dict(state_ss=nbytes + 4)]
  h.profile_enable(True)
  h.profile_read()
  for change in bad:
    args = dict(good, **change)
    assert h.lib.td_frontend_push(*args.values()) == -1, change
  assert h.profile_read()[0] == 0
  assert bool((state == 7).all())
  # (and the call the changes were made to is a good one; either output alone; no section takes NULL tables; an
  # empty push queues nothing)
  assert h.lib.td_frontend_push(*good.values()) == 0
  assert h.lib.td_frontend_push(*dict(good, out32=None, before=n).values()) == 0
  assert h.lib.td_frontend_push(*dict(good, out64=None, before=2 * n, sos=None, zi=None, sections=0, split=0,
                                      groups=0, ref_ptr=None, ref_idx=None, chan_ptr=None, chan_idx=None, sel=None,
                                      cs=c, ldout=c, out_ss=n * c, state_ss=nbytes).values()) == 0
  assert h.profile_read()[0] == 3
  assert h.lib.td_frontend_push(*dict(good, n=0, x=None, before=3 * n).values()) == 0
  assert h.profile_read()[0] == 0
  h.profile_enable(False)
  assert not bool((state == 7).all())


def test_the_frames_go_into_an_online_decoder_as_they_are(dev):
  """front.push(raw) -> decoder.push(eeg, env1, env2) with no host copy in between: the device tensor of every push
  goes in unchanged, and the decisions are those of ONE push of the concatenated front-end output."""
  import torch
  from telluride_decoding_amd import online
  c, pre, post = 5, 2, 9
  rec = host_online.recipe(c, pre, post)
  decoder = host_online.linear_decoder(c, pre, post, rec['w'], rec['b'], rec['corr'][0])
  h = dev.default_handle()
  # raw rows at 1 kHz whose 100 Hz frames carry the recipe's EEG: every frame held for 10 rows, plus an offset
  raw = np.repeat(rec['eeg'][:300], 10, axis=0) + np.float32(2.0)
  kw = dict(fs_in=1000, fs_out=100, highpass_cutoff=0.5, highpass_order=4, data_mean=0.0, data_std=1.0)
  rawd = h.to_device(raw)
  envd = h.to_device(rec['env'][:300])
  front = online.OnlinePreprocessor(ho.make(kw))
  live = online.OnlineDecoder(decoder, 37, 11)
  scores, decisions, frames, at = [], [], [], 0
  for n in (37, 250, 1, 999, 1713):
    eeg = front.push(rawd[at:at + n])
    assert isinstance(eeg, torch.Tensor) and eeg.is_cuda and eeg.dtype == torch.float32 and eeg.is_contiguous()
    m0, m = sum(int(f.shape[1]) for f in frames), int(eeg.shape[1])
    r = live.push(eeg, envd[m0:m0 + m, 0], envd[m0:m0 + m, 1])
    frames.append(eeg); scores.append(r.scores[0]); decisions.append(r.decisions[0])
    at += n
  eeg = front.flush()
  m0, m = sum(int(f.shape[1]) for f in frames), int(eeg.shape[1])
  r = live.push(eeg, envd[m0:m0 + m, 0], envd[m0:m0 + m, 1])
  frames.append(eeg); scores.append(r.scores[0]); decisions.append(r.decisions[0])
  r = live.flush()
  scores.append(r.scores[0]); decisions.append(r.decisions[0])
  whole = torch.cat(frames, dim=1)
  assert tuple(whole.shape) == (1, 300, c)
  once = online.OnlineDecoder(decoder, 37, 11)
  a = once.push(whole, envd[:, 0], envd[:, 1])
  b = once.flush()
  want_scores = np.concatenate([a.scores[0], b.scores[0]])
  want_decisions = np.concatenate([a.decisions[0], b.decisions[0]])
  assert want_scores.shape == ((300 - 37) // 11 + 1, 2)
  assert np.concatenate(scores).tobytes() == want_scores.tobytes()
  assert np.concatenate(decisions).tobytes() == want_decisions.tobytes()
