"""Python host layer over the C-ABI: device handle and sufficient statistics.

PyTorch is used ONLY as plumbing -- device memory (`torch.empty(..., device=
'cuda')`), the current HIP stream and `torch.distributed` (RCCL).  All hot-path
arithmetic runs in the hand-written HIP kernels of libtd_hotpath.so.
"""
import collections
import ctypes

import numpy as np

from telluride_decoding_amd import _lib

_handles = {}


def _torch():
  import torch  # deferred: `import telluride_decoding_amd` stays cheap on CPU
  return torch


def gpu_available():
  lib = _lib.load()
  n = ctypes.c_int(0)
  return lib.td_device_count(ctypes.byref(n)) == _lib.TD_OK and n.value > 0


class Handle(object):
  """One per (process, GPU).  Work is queued on torch's current stream."""

  def __init__(self, device_id=None):
    torch = _torch()
    self.lib = _lib.load()
    if device_id is None:
      device_id = torch.cuda.current_device() if torch.cuda.is_available() else 0
    ptr = ctypes.c_void_p()
    _lib.check(None, self.lib.td_create(int(device_id), ctypes.byref(ptr)))
    self.ptr = ptr
    self.device_id = int(device_id)
    self.device = torch.device('cuda', self.device_id)
    self.accumulate_mode = 'f16x2'
    self.use_torch_stream()

  def use_torch_stream(self):
    """Adopts torch's current stream: everything this handle queues goes there."""
    torch = _torch()
    stream = torch.cuda.current_stream(self.device)
    self.check(self.lib.td_set_stream(self.ptr, ctypes.c_void_p(stream.cuda_stream)))
    self._stream = stream

  def check(self, status):
    _lib.check(self.ptr, status)

  def synchronize(self):
    self.check(self.lib.td_synchronize(self.ptr))

  def record_event(self):
    """An event recorded on the stream this handle queues its work on (the one it adopted,
    which need not be torch's current stream any more); .synchronize() waits for everything
    the handle queued before it."""
    ev = _torch().cuda.Event()
    ev.record(self._stream)
    return ev

  ACCUMULATE_MODES = {'f16x2': 0, 'bf16x3': 1, 'f32': 2}

  def set_accumulate_mode(self, mode):
    """'f16x2' (default: two float16 pieces, 3 products), 'bf16x3' (6 products, exact to 2^-27)
    or 'f32' (the float32 matrix instruction): td_set_accumulate_mode."""
    self.check(self.lib.td_set_accumulate_mode(self.ptr, self.ACCUMULATE_MODES[mode]))
    self.accumulate_mode = mode

  SOLVERS = {'auto': 0, 'cholesky': 1, 'cg': 2}

  def set_solver(self, mode):
    """'auto' (default: a few large systems on an unmasked handle try the one-launch conjugate
    gradients first), 'cholesky' or 'cg': td_set_solver."""
    self.check(self.lib.td_set_solver(self.ptr, self.SOLVERS[mode]))

  def set_option(self, name, value):
    """td_set_option: 'cca_whitening' (0 automatic / 1 eigen route), 'cg_limit_ticks' (< 0 default),
    'narrow16' (1 default: <= 16 channels x <= 16 lags on the one-kernel streaming accumulate; 0: the tiled
    kernels) and 'async_cg' (1: ridge_solve_async may run conjugate gradients on the compact statistics; its
    flag can then be 2 = the solver gave up, W and b are NOT usable -- solve again with ridge_solve, as
    pipeline.FitPipeline does; 0 default: flags 0 / 1 only); 'cca_fused' (1 default: the dense stage of a small
    CCA in one launch; 0: the chain of launches); 'reserve_workspace' (bytes: grow the workspace arena now);
    'targets_f16' (1 default: y^T x~ of 33 .. 64 channels per tile on the float16 matrix pipe; 0: the float32 kernel)."""
    self.check(self.lib.td_set_option(self.ptr, name.encode(), int(value)))

  def scratch_bytes(self):
    """Bytes the handle's kernel scratch arena holds (td_scratch_bytes): its high-water mark x 1.25."""
    n = ctypes.c_int64(0)
    self.check(self.lib.td_scratch_bytes(self.ptr, ctypes.byref(n)))
    return int(n.value)

  def last_solve_info(self):
    """What the last synchronous ridge solve on this handle did: {'solver': 'cholesky' | 'cg',
    'iterations': n, 'cg_status': 0 converged / 2 not converged / 3 aborted} (td_last_solve_info)."""
    s, it, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    self.check(self.lib.td_last_solve_info(self.ptr, ctypes.byref(s), ctypes.byref(it), ctypes.byref(st)))
    return {'solver': {1: 'cholesky', 2: 'cg'}.get(s.value, 'none'), 'iterations': int(it.value),
            'cg_status': int(st.value)}

  def last_cg_plan(self):
    """Which conjugate-gradient kernel the last ridge solve on this handle launched (td_last_cg_plan; cleared at
    the start of every ridge solve): {'kernel': 'resident' | 'compact' | 'none', 'rows': R of the resident kernel
    or 0, 'channels_per_workgroup': 1 / 2 of the compact kernel or 0, 'workgroups': n}."""
    kn, pr, wg = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    self.check(self.lib.td_last_cg_plan(self.ptr, ctypes.byref(kn), ctypes.byref(pr), ctypes.byref(wg)))
    kernel = {1: 'resident', 2: 'compact'}.get(kn.value, 'none')
    return {'kernel': kernel, 'rows': int(pr.value) if kernel == 'resident' else 0,
            'channels_per_workgroup': int(pr.value) if kernel == 'compact' else 0, 'workgroups': int(wg.value)}

  def timer_start(self):
    self.check(self.lib.td_timer_start(self.ptr))

  def timer_stop(self):
    ms = ctypes.c_float(0)
    self.check(self.lib.td_timer_stop(self.ptr, ctypes.byref(ms)))
    return float(ms.value)

  def profile_enable(self, on=True):
    self.check(self.lib.td_profile_enable(self.ptr, 1 if on else 0))

  def profile_read(self):
    """(launches, total_ms, samples) of the dominant kernel since the last read."""
    n, ms, smp = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
    self.check(self.lib.td_profile_read(self.ptr, ctypes.byref(n), ctypes.byref(ms),
                                        ctypes.byref(smp)))
    return int(n.value), float(ms.value), float(smp.value)

  def probe_bf16_mfma(self, split_shaped=True):
    """TFLOP/s a bare bf16 MFMA loop sustains on this handle's CUs (td_probe_bf16_mfma)."""
    t = ctypes.c_double(0)
    self.check(self.lib.td_probe_bf16_mfma(self.ptr, 1 if split_shaped else 0, ctypes.byref(t)))
    return float(t.value)

  # -- memory plumbing ------------------------------------------------------
  def to_device(self, array, dtype=np.float32):
    """Host array (or tensor) -> contiguous 2-D device tensor."""
    torch = _torch()
    if isinstance(array, torch.Tensor):
      t = array.to(self.device)
      want = {np.float32: torch.float32, np.float64: torch.float64}[dtype]
      if t.dtype != want:
        t = t.to(want)
      return t.contiguous()
    arr = np.ascontiguousarray(array, dtype=dtype)
    return torch.from_numpy(arr).to(self.device)

  def zeros(self, shape, dtype='float32'):
    torch = _torch()
    return torch.zeros(shape, dtype=getattr(torch, dtype), device=self.device)

  def empty(self, shape, dtype='float32'):
    """Uninitialised device tensor: for outputs a kernel writes completely."""
    torch = _torch()
    return torch.empty(shape, dtype=getattr(torch, dtype), device=self.device)

  def __del__(self):
    try:
      if getattr(self, 'ptr', None):
        self.lib.td_destroy(self.ptr)
        self.ptr = None
    except Exception:  # interpreter shutdown
      pass


# The default handle reserves its workspace arena when it is created (td_set_option "reserve_workspace"): the dense
# stage of a leave-one-out sweep asks for 1.9 GB at C5 (32 folds x 35 MB of dense moments, 20 factors), and a hipMalloc
# of that size is ~55 ms -- five times the sweep.  2.5 GB of 288; 0 = grow on demand (as every other Handle does).
DEFAULT_WORKSPACE_BYTES = 2560 << 20


def default_handle():
  """The handle of the current device (created on first use, with DEFAULT_WORKSPACE_BYTES of workspace reserved)."""
  torch = _torch()
  if not gpu_available():
    raise _lib.HotPathUnavailable(
        'No MI355X visible to HIP: the hot path has no CPU fallback.')
  dev = torch.cuda.current_device()
  if dev not in _handles:
    _handles[dev] = Handle(dev)
    if DEFAULT_WORKSPACE_BYTES:
      _handles[dev].set_option('reserve_workspace', DEFAULT_WORKSPACE_BYTES)
  h = _handles[dev]
  h.use_torch_stream()
  return h


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class LagStats(object):
  """Device-resident sufficient statistics of lagged inputs (C-ABI td_stats).
  `LagStats.last_loso_status`: what the last ridge_solve_loso call of this process reported.

  Replaces the accumulate loops of
  brain_model.calculate_linear_regressor_parameters_from_dataset
  (brain_model.py:422-446) and cca.calculate_cca_parameters_from_dataset
  (cca.py:304-332) together with the lag-matrix builder (brain_data.py:425-483).
  """

  def __init__(self, c1, pre1=0, post1=0, c2=0, pre2=0, post2=0, d=0, handle=None):
    self.h = handle or default_handle()
    self.c1, self.pre1, self.post1 = int(c1), int(pre1), int(post1)
    self.c2, self.pre2, self.post2, self.d = int(c2), int(pre2), int(post2), int(d)
    self.l1 = self.pre1 + 1 + self.post1
    self.l2 = (self.pre2 + 1 + self.post2) if self.c2 else 0
    self.k1 = self.l1 * self.c1
    self.k2 = self.l2 * self.c2
    # half width of a boundary window = the halo a time-range shard needs (TimeShardPlan)
    self.hw = self.pre1 + self.post1 + self.pre2 + self.post2 + 1
    ptr = ctypes.c_void_p()
    self.h.check(self.h.lib.td_stats_create(
        self.h.ptr, self.c1, self.pre1, self.post1, self.c2, self.pre2, self.post2,
        self.d, ctypes.byref(ptr)))
    self.ptr = ptr

  def like(self):
    return LagStats(self.c1, self.pre1, self.post1, self.c2, self.pre2, self.post2,
                    self.d, handle=self.h)

  def reset(self):
    self.h.check(self.h.lib.td_stats_reset(self.h.ptr, self.ptr))

  def accumulate(self, x, x2=None, y=None, file_offsets=None, input_offset=0,
                 rows_used=None, parts=3, handle=None, ranges=None, edges=None):
    """x [rows, c1], x2 [rows, c2] / y [rows, d]: device float32 tensors holding
    the files concatenated along time; file_offsets has F+1 row offsets.
    parts: | 8 (with 3; TD_ACC_DEFER) leaves the finalize launch of the call pending: complete(handle)
    queues it on another handle's stream (pipeline.FitPipeline hands it to the solve stream).
    parts: 1 = covariances + windows + counters, 2 = targets / bias moments (after part 1 of
    the same files, possibly on another handle's stream), 3 = both; 2 | 4 = the targets part
    AHEAD of part 1 of the same files (TD_ACC_TARGETS_FIRST: it also leaves the channel maxima
    the float16 matrix kernel of part 1 scales by in the statistics).
    ranges: per file (begin, end) rows of the file that this call sums, for ranks that share a
    long recording by time range (each holds its range plus a halo of pre + post rows);
    edges: per file bit 0 / bit 1 = the piece holds the recording's first / last row
    (td_stats_accumulate_ranges)."""
    rows = int(x.shape[0])
    if file_offsets is None:
      file_offsets = [0, rows]
    offs, offs_p = _lib.i64_array(file_offsets)
    if offs[-1] != rows:
      raise ValueError('file_offsets[-1] (%d) != rows (%d)' % (offs[-1], rows))
    used_p = None
    if rows_used is not None:
      used, used_p = _lib.i64_array(rows_used)
    for t, w, name in ((x, self.c1, 'input_1'), (x2, self.c2, 'input_2'), (y, self.d, 'output')):
      if w and (t is None or t.dim() != 2 or t.shape[1] != w or t.shape[0] != rows):
        raise ValueError('%s must be [%d, %d], not %s' %
                         (name, rows, w, None if t is None else tuple(t.shape)))
      if t is not None and w and (str(t.dtype) != 'torch.float32' or not t.is_cuda):
        raise TypeError('%s must be a float32 device tensor' % name)
    h = handle or self.h
    if ranges is None and edges is None:
      h.check(h.lib.td_stats_accumulate_parts(
          h.ptr, self.ptr, _ptr(x), x.stride(0),
          _ptr(x2 if self.c2 else None), x2.stride(0) if self.c2 else 0,
          _ptr(y if self.d else None), y.stride(0) if self.d else 0,
          offs_p, len(offs) - 1, int(input_offset), used_p, int(parts)))
      return
    nf = len(offs) - 1
    rb_p = re_p = None
    if ranges is not None:
      rb, rb_p = _lib.i64_array([r[0] for r in ranges])
      re, re_p = _lib.i64_array([r[1] for r in ranges])
      if len(rb) != nf:
        raise ValueError('ranges must have one (begin, end) pair per file')
    fl = None
    if edges is not None:
      fl = (ctypes.c_int * nf)(*[int(e) for e in edges])
    h.check(h.lib.td_stats_accumulate_ranges(
        h.ptr, self.ptr, _ptr(x), x.stride(0),
        _ptr(x2 if self.c2 else None), x2.stride(0) if self.c2 else 0,
        _ptr(y if self.d else None), y.stride(0) if self.d else 0,
        offs_p, nf, int(input_offset), used_p, rb_p, re_p, fl, int(parts)))

  def complete(self, handle=None):
    """Queues the finalize launch an accumulate(parts=3 | 8) call left pending on `handle`'s stream,
    behind an event of that call (td_stats_complete); nothing to do without one."""
    h = handle or self.h
    h.check(h.lib.td_stats_complete(h.ptr, self.ptr))

  def counts(self):
    frames, files = ctypes.c_int64(0), ctypes.c_int64(0)
    self.h.check(self.h.lib.td_stats_counts(self.h.ptr, self.ptr, ctypes.byref(frames),
                                            ctypes.byref(files)))
    return int(frames.value), int(files.value)

  def combine(self, parts):
    arr = (ctypes.c_void_p * len(parts))(*[p.ptr for p in parts])
    self.h.check(self.h.lib.td_stats_combine(self.h.ptr, self.ptr, arr, len(parts)))
    return self

  def packed_len(self, total_file_slots):
    n = ctypes.c_int64(0)
    self.h.check(self.h.lib.td_stats_packed_len(self.h.ptr, self.ptr, int(total_file_slots),
                                                ctypes.byref(n)))
    return int(n.value)

  def pack(self, total_file_slots, file_slot, handle=None):
    """handle: the handle (= stream) to queue the kernel on, if not the statistics' own."""
    h = handle or self.h
    buf = h.empty((self.packed_len(total_file_slots),), 'float64')
    h.check(h.lib.td_stats_pack(h.ptr, self.ptr, _ptr(buf), int(total_file_slots),
                                int(file_slot)))
    return buf

  def unpack(self, buf, total_file_slots, total_frames=None, handle=None):
    """total_frames (frames of all ranks, if the caller knows them) avoids a device-to-host
    read that synchronises the stream."""
    h = handle or self.h
    h.check(h.lib.td_stats_unpack_known(
        h.ptr, self.ptr, _ptr(buf), int(total_file_slots),
        -1 if total_frames is None else int(total_frames)))

  def moments(self, want_xtx=True, want_xty=True, want_cca=False):
    """Dense float64 device matrices (see td_stats_moments)."""
    out = {}
    n = self.k1 + 1
    xtx = self.h.empty((n, n), 'float64') if want_xtx else None
    xty = self.h.empty((n, self.d), 'float64') if (want_xty and self.d) else None
    x2 = xx2 = s2 = None
    if want_cca and self.c2:
      x2 = self.h.empty((self.k2, self.k2), 'float64')
      xx2 = self.h.empty((self.k1, self.k2), 'float64')
      s2 = self.h.empty((self.k2,), 'float64')
    self.h.check(self.h.lib.td_stats_moments(self.h.ptr, self.ptr, _ptr(xtx), _ptr(xty),
                                             _ptr(x2), _ptr(xx2), _ptr(s2)))
    out.update(xtx=xtx, xty=xty, x2tx2=x2, xtx2=xx2, sum_x2=s2)
    return out

  def ridge_solve(self, lambdas, handle=None):
    """Returns device tensors W [n_lambda, k1, d], b [n_lambda, d] (float32).  `handle`
    selects the handle (stream, workspaces) the solve runs on; the caller orders it after
    the accumulation (pipeline.FitPipeline)."""
    h = handle or self.h
    lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
    w = h.empty((len(lam), self.k1, self.d), 'float32')
    b = h.empty((len(lam), self.d), 'float32')
    h.check(h.lib.td_ridge_solve(h.ptr, self.ptr, lam_p, len(lam), _ptr(w), _ptr(b)))
    return w, b

  def ridge_solve_async(self, lambdas, handle=None):
    """ridge_solve without waiting for the device: returns (W, b, flag) where flag() reads the
    singular-system flag (1 = some system was not positive definite) from the handle's pinned
    host ring -- call it only after waiting for an event recorded behind this call.  On a handle with
    set_option('async_cg', 1) the flag can also be 2: the conjugate-gradient solver gave up and W / b hold
    nothing usable -- repeat the solve with ridge_solve (any non-zero flag is NOT "singular" then)."""
    h = handle or self.h
    lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
    w = h.empty((len(lam), self.k1, self.d), 'float32')
    b = h.empty((len(lam), self.d), 'float32')
    ptr = ctypes.POINTER(ctypes.c_int)()
    h.check(h.lib.td_ridge_solve_async(h.ptr, self.ptr, lam_p, len(lam), _ptr(w), _ptr(b),
                                       ctypes.byref(ptr)))
    return w, b, (lambda: int(ptr[0]))

  @staticmethod
  def ridge_solve_multi(stats_list, lambdas, handle=None, wait=True):
    """Every (statistics, lambda) pair in ONE batched factorisation (td_ridge_solve_multi):
    W [n_stats, n_lambda, k1, d], b [n_stats, n_lambda, d] float32 device tensors.  wait=False
    returns (W, b, flag) like ridge_solve_async."""
    first = stats_list[0]
    h = handle or first.h
    lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
    w = h.empty((len(stats_list), len(lam), first.k1, first.d), 'float32')
    b = h.empty((len(stats_list), len(lam), first.d), 'float32')
    arr = (ctypes.c_void_p * len(stats_list))(*[s.ptr for s in stats_list])
    if wait:
      h.check(h.lib.td_ridge_solve_multi(h.ptr, arr, len(stats_list), lam_p, len(lam), _ptr(w),
                                         _ptr(b), None))
      return w, b
    ptr = ctypes.POINTER(ctypes.c_int)()
    h.check(h.lib.td_ridge_solve_multi(h.ptr, arr, len(stats_list), lam_p, len(lam), _ptr(w),
                                       _ptr(b), ctypes.byref(ptr)))
    return w, b, (lambda: int(ptr[0]))

  @staticmethod
  def ridge_solve_loso(total, folds, lambdas, max_iter=40, tol=1e-12, handle=None):
    """The (fold x lambda) systems of a leave-one-out sweep by preconditioned conjugate gradients
    (td_ridge_solve_loso): `total` = statistics of all recordings, folds[f] = training statistics
    of fold f.  Returns (W [n_folds, n_lambda, k1, d], b [n_folds, n_lambda, d], iterations), or
    None when the solver reports that it did not converge / the preconditioner is not positive
    definite (the caller then takes the direct batched solve)."""
    h = handle or total.h
    lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
    w = h.empty((len(folds), len(lam), total.k1, total.d), 'float32')
    b = h.empty((len(folds), len(lam), total.d), 'float32')
    arr = (ctypes.c_void_p * len(folds))(*[s.ptr for s in folds])
    status, iters = ctypes.c_int(0), ctypes.c_int(0)
    h.check(h.lib.td_ridge_solve_loso(h.ptr, total.ptr, arr, len(folds), lam_p, len(lam), int(max_iter),
                                      float(tol), _ptr(w), _ptr(b), ctypes.byref(status),
                                      ctypes.byref(iters)))
    LagStats.last_loso_status = {0: 'converged', 1: 'not converged', 2: 'preconditioner not positive definite'}.get(
        status.value, 'status %d' % status.value)
    if status.value:
      return None
    return w, b, int(iters.value)

  @staticmethod
  def accumulate_each(stats_list, x, y, file_offsets, input_offset=0, rows_used=None, handle=None):
    """File f of x / y into stats_list[f] (fresh regression statistics) with ONE targets launch and ONE matrix
    launch over all the recordings (td_stats_accumulate_each).  False: not a shape of that form, nothing was
    queued -- accumulate file by file."""
    h = handle or stats_list[0].h
    offs, offs_p = _lib.i64_array(file_offsets)
    used, used_p = (_lib.i64_array(rows_used) if rows_used is not None else (None, None))
    arr = (ctypes.c_void_p * len(stats_list))(*[s.ptr for s in stats_list])
    handled = ctypes.c_int(0)
    h.check(h.lib.td_stats_accumulate_each(h.ptr, arr, _ptr(x), x.stride(0), _ptr(y), y.stride(0), offs_p,
                                           len(offs) - 1, int(input_offset), used_p, ctypes.byref(handled)))
    LagStats.last_each_status = int(handled.value)      # (<= 0: which check sent the caller back to the per-file loop)
    return handled.value > 0

  @staticmethod
  def ridge_solve_loso_terms(total, fold_terms, lambdas, max_iter=40, tol=1e-12, handle=None, k_major=False):
    """The same sweep with every fold given as total + a few signed terms (td_ridge_solve_loso_terms):
    fold_terms[f] = [(LagStats, +1 or -1), ...] -- minus the held-out recording, and for a fold whose
    minibatch stream drops a remainder minus the last training recording plus its truncated twin.  No fold
    statistics are summed; the folds' dense moments come from the total's in one launch.  Returns as
    ridge_solve_loso; k_major: W comes as [n_folds, k1, n_lambda * d] (a fold's models as the output columns of one
    filter: what predict_fir_per_file takes)."""
    h = handle or total.h
    lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
    n_folds = len(fold_terms)
    w = h.empty((n_folds, total.k1, len(lam) * total.d) if k_major else (n_folds, len(lam), total.k1, total.d), 'float32')
    b = h.empty((n_folds, len(lam), total.d), 'float32')
    flat = [t for terms in fold_terms for t in terms]
    arr = (ctypes.c_void_p * max(1, len(flat)))(*[s.ptr for s, _ in flat])
    begin = np.concatenate(([0], np.cumsum([len(t) for t in fold_terms]))).astype(np.int32)
    signs = np.asarray([float(sg) for _, sg in flat] or [0.0], np.float64)
    status, iters = ctypes.c_int(0), ctypes.c_int(0)
    h.check(h.lib.td_ridge_solve_loso_terms(
        h.ptr, total.ptr, arr, begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        signs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n_folds, lam_p, len(lam), int(max_iter), float(tol),
        1 if k_major else 0, _ptr(w), _ptr(b), ctypes.byref(status), ctypes.byref(iters)))
    LagStats.last_loso_status = {0: 'converged', 1: 'not converged', 2: 'preconditioner not positive definite'}.get(
        status.value, 'status %d' % status.value)
    if status.value:
      return None
    return w, b, int(iters.value)

  @staticmethod
  def cca_solve_loso_terms(total, fold_terms, fold_batches, batch_size, lambdas, dim, eps_eig=1e-12, handle=None):
    """One CCA model per (fold, lambda) of a leave-one-file-out sweep (td_cca_solve_loso_terms): `total` = the CCA
    statistics of all recordings, fold_terms[f] = [(LagStats, +1 or -1), ...] as ridge_solve_loso_terms takes them,
    fold_batches[f] = minibatches of `batch_size` frames in fold f's training stream.  Returns float32 device tensors
    (rot_x [F, k1, L * dim], rot_y [F, k2, L * dim], mean_x [F, k1], mean_y [F, k2], bias_x [F, L * dim],
    bias_y [F, L * dim], e [F, L, dim]) and the int32 device tensor status [F, L] (0 solved, 1 refit that pair with
    cca_solve); nothing waits for the device.  ValueError: k2 > 64, a fold of more than four terms, a bad dim."""
    h = handle or total.h
    lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
    n_folds, n_lam, dim = len(fold_terms), len(lam), int(dim)
    k1, k2 = total.k1, total.k2
    rot_x = h.empty((n_folds, k1, n_lam * dim), 'float32')
    rot_y = h.empty((n_folds, k2, n_lam * dim), 'float32')
    mean_x, mean_y = h.empty((n_folds, k1), 'float32'), h.empty((n_folds, k2), 'float32')
    bias_x, bias_y = h.empty((n_folds, n_lam * dim), 'float32'), h.empty((n_folds, n_lam * dim), 'float32')
    e = h.empty((n_folds, n_lam, dim), 'float32')
    status = h.empty((n_folds, n_lam), 'int32')
    flat = [t for terms in fold_terms for t in terms]
    arr = (ctypes.c_void_p * max(1, len(flat)))(*[s.ptr for s, _ in flat])
    begin = np.concatenate(([0], np.cumsum([len(t) for t in fold_terms]))).astype(np.int32)
    signs = np.asarray([float(sg) for _, sg in flat] or [0.0], np.float64)
    nb, nb_p = _lib.i64_array(fold_batches)
    h.check(h.lib.td_cca_solve_loso_terms(
        h.ptr, total.ptr, arr, begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        signs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n_folds, nb_p, int(batch_size), lam_p, n_lam, dim,
        float(eps_eig), _ptr(rot_x), _ptr(rot_y), _ptr(mean_x), _ptr(mean_y), _ptr(bias_x), _ptr(bias_y), _ptr(e),
        _ptr(status)))
    return rot_x, rot_y, mean_x, mean_y, bias_x, bias_y, e, status

  def cca_solve(self, denom, regularization, dim, eps_eig=1e-12, handle=None):
    """CCA dense stage on the device (td_cca_solve; reference cca.py:337-367): returns float32
    device tensors (rot_x [k1, dim], rot_y [k2, dim], mean_x [1, k1], mean_y [1, k2], e [dim])
    and the Jacobi sweep counts (eig xx, eig yy, svd)."""
    h = handle or self.h
    # (one buffer, five views: a caller that wants the results on the host copies it once -- cca_results_host)
    k1, k2, dim = self.k1, self.k2, int(dim)
    buf = h.empty(((k1 + k2) * dim + k1 + k2 + dim,), 'float32')
    o = [0, k1 * dim, (k1 + k2) * dim, (k1 + k2) * dim + k1, (k1 + k2) * dim + k1 + k2]
    rot_x = buf[o[0]:o[1]].view(k1, dim)
    rot_y = buf[o[1]:o[2]].view(k2, dim)
    mean_x = buf[o[2]:o[3]].view(1, k1)
    mean_y = buf[o[3]:o[4]].view(1, k2)
    e = buf[o[4]:]
    self._cca_buf = (buf, o, k1, k2, dim)
    info = (ctypes.c_int * 4)()
    h.check(h.lib.td_cca_solve(h.ptr, self.ptr, float(denom), float(regularization),
                               float(eps_eig), int(dim), _ptr(rot_x), _ptr(rot_y), _ptr(mean_x),
                               _ptr(mean_y), _ptr(e), info))
    self.last_cca_route = 'cholesky' if info[3] & 1 else 'eigen'     # whitening of the x side
    self.last_cca_route_y = 'cholesky' if info[3] & 2 else 'eigen'   # ... of the other side
    self.last_cca_fused = bool(info[3] & 4)                           # the one-launch dense stage (K1 <= 64, K2 <= 16)
    return rot_x, rot_y, mean_x, mean_y, e, tuple(info[:3])

  def cca_results_host(self):
    """The last cca_solve's five results as float32 NumPy arrays from ONE device-to-host copy."""
    buf, o, k1, k2, dim = self._cca_buf
    a = buf.cpu().numpy()
    return (a[o[0]:o[1]].reshape(k1, dim), a[o[1]:o[2]].reshape(k2, dim), a[o[2]:o[3]].reshape(1, k1),
            a[o[3]:o[4]].reshape(1, k2), a[o[4]:].copy())

  def __del__(self):
    try:
      if getattr(self, 'ptr', None):
        self.h.lib.td_stats_destroy(self.h.ptr, self.ptr)
        self.ptr = None
    except Exception:
      pass


# ---------------------------------------------------------------- decode wrappers
REDUCTIONS = {'first': 0, 'second': 1, 'mean': 2, 'mean-squared': 3, 'lda': 4, 'all': 5}


def predict_fir(x, file_offsets, w, b, pre, post, out=None, handle=None, input_offset=0):
  """out[t] = b + sum_{l,c} x~[t+l-pre][c] W[l*C+c]   (td_predict_fir).

  x [rows, C] device float32; w [K, D], b [D] device float32.  Output row
  file_offsets[f] + t is frame t of file f's zipped streams."""
  h = handle or default_handle()
  rows, c = int(x.shape[0]), int(x.shape[1])
  d = int(w.shape[1])
  if int(w.shape[0]) != c * (pre + 1 + post):
    raise ValueError('weight matrix has %d rows, expected %d' %
                     (w.shape[0], c * (pre + 1 + post)))
  if out is None:
    out = h.empty((rows, d), 'float32')
  offs, offs_p = _lib.i64_array(file_offsets)
  h.check(h.lib.td_predict_fir(h.ptr, _ptr(x), x.stride(0), offs_p, len(offs) - 1, c, pre, post,
                               int(input_offset), _ptr(w), _ptr(b), d, _ptr(out),
                               out.stride(0)))
  return out


def predict_fir_per_file(x, file_offsets, w, b, pre, post, out=None, handle=None, input_offset=0):
  """predict_fir with every file under its own model (td_predict_fir_per_file): w [files, K, D],
  b [files, D] device float32 -- the held-out recordings of a leave-one-out sweep in one launch."""
  h = handle or default_handle()
  rows, c = int(x.shape[0]), int(x.shape[1])
  offs, offs_p = _lib.i64_array(file_offsets)
  n_files, d = len(offs) - 1, int(w.shape[2])
  if int(w.shape[0]) != n_files or int(w.shape[1]) != c * (pre + 1 + post):
    raise ValueError('weights are %s, expected (%d, %d, D)' %
                     (tuple(w.shape), n_files, c * (pre + 1 + post)))
  if out is None:
    out = h.empty((rows, d), 'float32')
  w = w.contiguous()
  b = b.contiguous()
  h.check(h.lib.td_predict_fir_per_file(h.ptr, _ptr(x), x.stride(0), offs_p, n_files, c, pre, post,
                                        int(input_offset), _ptr(w), _ptr(b), d, _ptr(out),
                                        out.stride(0)))
  return out


def cca_transform(x, x2, file_offsets, mean1, rot1, mean2, rot2, pre1, post1, pre2, post2,
                  handle=None, input_offset=0, out=None):
  h = handle or default_handle()
  rows = int(x.shape[0])
  dims = int(rot1.shape[1])
  if out is None:
    out = h.empty((rows, 2 * dims), 'float32')
  offs, offs_p = _lib.i64_array(file_offsets)
  h.check(h.lib.td_cca_transform(
      h.ptr, _ptr(x), x.stride(0), int(x.shape[1]), pre1, post1, _ptr(x2), x2.stride(0),
      int(x2.shape[1]), pre2, post2, offs_p, len(offs) - 1, int(input_offset), _ptr(mean1),
      _ptr(rot1),
      _ptr(mean2), _ptr(rot2), dims, _ptr(out), out.stride(0)))
  return out


def window_layout(trial_offsets, width, hop):
  """(window_offsets[T+1], total_windows) for full windows of each trial."""
  lib = _lib.load()
  offs, offs_p = _lib.i64_array(trial_offsets)
  wo = np.zeros(len(offs), np.int64)
  total = ctypes.c_int64(0)
  _lib.check(None, lib.td_window_count(offs_p, len(offs) - 1, int(width), int(hop),
                                       wo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                       ctypes.byref(total)))
  return wo, int(total.value)


def general_solve(a, rhs, handle=None):
  """np.linalg.solve(a, rhs) in float64 on the device (LU, partial pivoting): a [n, n] and
  rhs [n, nrhs] float64 device tensors; returns the solution, inputs untouched."""
  h = handle or default_handle()
  a = a.clone().contiguous()
  x = rhs.clone().contiguous()
  h.check(h.lib.td_general_solve(h.ptr, _ptr(a), _ptr(x), int(a.shape[0]), int(x.shape[1])))
  return x


def sym_eigh(a, handle=None):
  """Eigen-decomposition of a symmetric float64 device matrix (td_sym_eigh): (vals [n]
  unsorted, vecs [n, n] with the eigenvectors as columns, outer sweeps)."""
  h = handle or default_handle()
  a = a.contiguous()
  n = int(a.shape[0])
  vals = h.empty((n,), 'float64')
  vecs = h.empty((n, n), 'float64')
  sweeps = ctypes.c_int(0)
  h.check(h.lib.td_sym_eigh(h.ptr, _ptr(a), n, _ptr(vals), _ptr(vecs), ctypes.byref(sweeps)))
  return vals, vecs, int(sweeps.value)


def jacobi_svd(t, dim, handle=None):
  """The `dim` largest singular triplets of a float64 device matrix t [m, n] (td_jacobi_svd):
  (u [dim, m], s [dim] descending, v [dim, n]) with the singular vectors as rows, sweeps."""
  h = handle or default_handle()
  t = t.contiguous()
  m, n = int(t.shape[0]), int(t.shape[1])
  u = h.empty((dim, m), 'float64')
  sv = h.empty((dim,), 'float64')
  v = h.empty((dim, n), 'float64')
  sweeps = ctypes.c_int(0)
  h.check(h.lib.td_jacobi_svd(h.ptr, _ptr(t), m, n, int(dim), _ptr(u), _ptr(sv), _ptr(v),
                              ctypes.byref(sweeps)))
  return u, sv, v, int(sweeps.value)


def spd_solve(a, rhs, handle=None):
  """Solution of a x = rhs for a symmetric positive definite float64 device matrix a [n, n]
  and rhs [n, nrhs] (td_spd_solve, blocked Cholesky); inputs untouched."""
  h = handle or default_handle()
  n, nrhs = int(a.shape[0]), int(rhs.shape[1])
  if nrhs <= 8:
    a = a.clone().contiguous()
    x = rhs.clone().contiguous()
    h.check(h.lib.td_spd_solve(h.ptr, _ptr(a), _ptr(x), n, nrhs, 1))
    return x
  # td_spd_solve carries at most 8 right-hand sides through its factorisation (and overwrites
  # the matrix): wider ones go 8 columns at a time
  out = rhs.clone().contiguous()
  for c0 in range(0, nrhs, 8):
    x = rhs[:, c0:c0 + 8].clone().contiguous()
    m = a.clone().contiguous()
    h.check(h.lib.td_spd_solve(h.ptr, _ptr(m), _ptr(x), n, int(x.shape[1]), 1))
    out[:, c0:c0 + 8] = x
  return out


def shrinkage_moment(x, file_offsets, pre, post, batch_rows, input_offset=0, rows_used=None,
                     handle=None):
  """np.sum(sum_x2tx2) of the reference's Ledoit-Wolf branch (brain_model.py:440-443) for the
  lagged rows of `x` [rows, C] cut into minibatches of `batch_rows`: a Python float."""
  h = handle or default_handle()
  out = h.zeros((1,), 'float64')
  offs, offs_p = _lib.i64_array(file_offsets)
  used, used_p = (_lib.i64_array(rows_used) if rows_used is not None else (None, None))
  h.check(h.lib.td_shrinkage_moment(h.ptr, _ptr(x), x.stride(0), int(x.shape[1]), int(pre),
                                    int(post), offs_p, len(offs) - 1, int(input_offset), used_p,
                                    int(batch_rows), _ptr(out)))
  return float(out.cpu()[0])


def shrinkage_terms(moments, n, sum_row, frames, handle=None):
  """(trace(zc), sum(zc^2)) of zc = S - m^T m for the [n, n] corner of the float64 device matrix `moments` (row
  stride = its own), m = row `sum_row` of it / frames: the two reductions of the reference's shrinkage algebra
  (brain_model.py:449-462), td_shrinkage_terms."""
  h = handle or default_handle()
  out = (ctypes.c_double * 2)()
  row = moments[int(sum_row)]
  h.check(h.lib.td_shrinkage_terms(h.ptr, _ptr(moments), moments.stride(0), int(n), _ptr(row), float(frames), out))
  return float(out[0]), float(out[1])


def shrunk_covariance(moments, n, scale, diag, want64=True, want32=True, handle=None):
  """scale * moments[:n, :n] + diag * I as a float64 and / or a float32 device tensor (td_shrunk_covariance)."""
  h = handle or default_handle()
  o64 = h.empty((int(n), int(n)), 'float64') if want64 else None
  o32 = h.empty((int(n), int(n)), 'float32') if want32 else None
  h.check(h.lib.td_shrunk_covariance(h.ptr, _ptr(moments), moments.stride(0), int(n), float(scale), float(diag),
                                     _ptr(o64), _ptr(o32)))
  return o64, o32


WINDOW_SUMS_CYCLED = True      # window_sums takes a `b` with fewer columns than `a` (td_window_sums_cycled)


def _check_unit_columns(who, **tensors):
  """The window kernels take a row stride and step 1 from column to column: a transposed or column-strided view
  would be read as if its columns were adjacent.  (A single column has no step to get wrong.)"""
  for name, t in tensors.items():
    if t.dim() != 2:
      raise ValueError('%s: %s must have two dimensions, not %d' % (who, name, t.dim()))
    if int(t.shape[1]) > 1 and t.stride(1) != 1:
      raise ValueError('%s: the columns of %s must be contiguous (column stride %d)' % (who, name, t.stride(1)))


def window_sums(a, b, trial_offsets, width, hop, handle=None):
  """Five float64 sums per window and column: [n_windows, cols, 5].  b may hold fewer columns than a (a
  divisor of a's): column j of a is then paired with column j % b.shape[1] of b (td_window_sums_cycled: several
  models' predictions against one truth, no tiled copy of the truth).  a, b: unit column stride, row stride
  free."""
  _check_unit_columns('window_sums', a=a, b=b)
  h = handle or default_handle()
  cols, b_cols = int(a.shape[1]), int(b.shape[1])
  _, total = window_layout(trial_offsets, width, hop)
  out = h.zeros((total, cols, 5), 'float64')
  offs, offs_p = _lib.i64_array(trial_offsets)
  if b_cols != cols:
    h.check(h.lib.td_window_sums_cycled(h.ptr, _ptr(a), a.stride(0), _ptr(b), b.stride(0), cols, b_cols, offs_p,
                                        len(offs) - 1, int(width), int(hop), _ptr(out)))
    return out
  h.check(h.lib.td_window_sums(h.ptr, _ptr(a), a.stride(0), _ptr(b), b.stride(0), cols, offs_p,
                               len(offs) - 1, int(width), int(hop), _ptr(out)))
  return out


def window_scores(sums, width, mode, reduction='first', mean_a=None, mean_b=None, power=None,
                  handle=None, group=None):
  """group (mode 1): the columns are cols / group models of `group` outputs each; the Pearson
  zero rule (a constant column zeroes the result) is applied per model (td_window_pearson)."""
  h = handle or default_handle()
  total, cols = int(sums.shape[0]), int(sums.shape[1])
  out = h.zeros((total,) if mode == 0 else (total, cols), 'float64')
  if mode == 1 and group is not None and int(group) != cols:
    h.check(h.lib.td_window_pearson(h.ptr, _ptr(sums), total, cols, int(group), int(width),
                                    _ptr(out)))
    return out
  args = []
  for v in (mean_a, mean_b, power):
    if v is None:
      args.append((None, None))
    else:
      args.append(_lib.f64_array(np.broadcast_to(np.asarray(v, np.float64).reshape(-1), (cols,))
                                 if np.size(v) == 1 else v))
  red = REDUCTIONS[reduction] if mode == 0 else 0
  h.check(h.lib.td_window_scores(h.ptr, _ptr(sums), total, cols, int(width), int(mode), red,
                                 args[0][1], args[1][1], args[2][1], _ptr(out)))
  return out


def frame_scores(a, b, reduction, mean_a, mean_b, power, lda_w=None, lda_slope=1.0,
                 lda_intercept=0.0, handle=None):
  """Per-frame reduced correlation score (Decoder.infer_one).  a, b: unit column stride, row stride free."""
  _check_unit_columns('frame_scores', a=a, b=b)
  h = handle or default_handle()
  if reduction not in REDUCTIONS:
    raise ValueError('Unknown reduction technique: %s' % reduction)
  rows, cols = int(a.shape[0]), int(a.shape[1])
  red = REDUCTIONS[reduction]
  out = h.zeros((rows, cols) if red == 5 else (rows,), 'float64')

  def vec(v):
    v = np.asarray(v, np.float64).reshape(-1)
    if v.size == 1:
      v = np.repeat(v, cols)
    return _lib.f64_array(v)

  ma, mb, pw = vec(mean_a), vec(mean_b), vec(power)
  lw = vec(lda_w) if lda_w is not None else (None, None)
  h.check(h.lib.td_frame_scores(h.ptr, _ptr(a), a.stride(0), _ptr(b), b.stride(0), cols, rows,
                                red, ma[1], mb[1], pw[1], lw[1], float(lda_slope),
                                float(lda_intercept), _ptr(out)))
  return out


def window_means(v, trial_offsets, width, hop, handle=None):
  h = handle or default_handle()
  _, total = window_layout(trial_offsets, width, hop)
  out = h.zeros((total,), 'float64')
  offs, offs_p = _lib.i64_array(trial_offsets)
  h.check(h.lib.td_window_means(h.ptr, _ptr(v), offs_p, len(offs) - 1, int(width), int(hop),
                                _ptr(out)))
  return out


WINDOW_CLASS_MOMENTS_MAX_COLS = 32


def window_class_moments(a, b, width, mean_a, mean_b, power, want_means=False, handle=None):
  """Decoder.train's windowed training data in one pass (td_window_class_moments): the per-frame values
  frame_scores(a, b, 'all', ...) would give, averaged over consecutive windows of `width` frames
  (infer_decoder.average_data: the tail is dropped), and the moments [[M^T M, sum m], [sum m^T, n_win]] of
  those window means -- the layout scaled_lda._moments_to_scatter takes.  a, b: float32 device tensors
  [rows, cols] with unit column stride (row stride free), cols <= 32, width >= 2.  Returns the float64
  device tensor [cols + 1, cols + 1], or (moments, means [rows // width, cols]) with want_means.  Queued,
  not waited for."""
  _check_unit_columns('window_class_moments', a=a, b=b)
  h = handle or default_handle()
  rows, cols = int(a.shape[0]), int(a.shape[1])
  if tuple(b.shape) != (rows, cols):
    raise ValueError('window_class_moments: a is %s and b is %s' % (tuple(a.shape), tuple(b.shape)))
  torch = _torch()
  for name, t in (('a', a), ('b', b)):
    if t.dtype != torch.float32 or t.device != h.device:
      raise TypeError('window_class_moments: %s must be a float32 tensor on %s, not %s on %s' %
                      (name, h.device, t.dtype, t.device))
  width = int(width)
  if rows == 0 and 1 <= cols <= WINDOW_CLASS_MOMENTS_MAX_COLS and width >= 2:
    # (an empty tensor has no address to hand to the kernel: no window, all-zero moments)
    moments = h.zeros((cols + 1, cols + 1), 'float64')
    return (moments, h.zeros((0, cols), 'float64')) if want_means else moments

  def vec(v):
    v = np.asarray(v, np.float64).reshape(-1)
    if v.size == 1:
      v = np.repeat(v, cols)
    if v.size != cols:
      raise ValueError('window_class_moments: %d statistics for %d columns' % (v.size, cols))
    return _lib.f64_array(v)

  ma, mb, pw = vec(mean_a), vec(mean_b), vec(power)
  moments = h.empty((cols + 1, cols + 1), 'float64')
  means = h.empty((rows // width if width > 0 else 0, cols), 'float64') if want_means else None
  # (a one-column view's row stride is whatever the tensor says; an empty tensor has no rows to step over)
  lda = int(a.stride(0)) if rows > 1 else max(cols, int(a.stride(0)))
  ldb = int(b.stride(0)) if rows > 1 else max(cols, int(b.stride(0)))
  h.check(h.lib.td_window_class_moments(h.ptr, _ptr(a), lda, _ptr(b), ldb, cols, rows, width,
                                        ma[1], mb[1], pw[1], _ptr(means) if want_means else None,
                                        _ptr(moments)))
  return (moments, means) if want_means else moments


def decide_wta(s1, s2, handle=None):
  h = handle or default_handle()
  out = h.zeros((int(s1.shape[0]),), 'uint8')
  h.check(h.lib.td_decide_wta(h.ptr, _ptr(s1), _ptr(s2), int(s1.shape[0]), _ptr(out)))
  return out


def decide_step(s1, s2, window_offsets, state=None, handle=None):
  h = handle or default_handle()
  out = h.zeros((int(s1.shape[0]),), 'uint8')
  wo, wo_p = _lib.i64_array(window_offsets)
  st = np.full(len(wo) - 1, 0.5) if state is None else np.ascontiguousarray(state, np.float64)
  h.check(h.lib.td_decide_step(h.ptr, _ptr(s1), _ptr(s2), wo_p, len(wo) - 1, _ptr(out),
                               st.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
  return out, st


SWEEP_DECODERS = {'wta': 0, 'stepped': 1, 'step': 1, 'none': 2}
SWEEP_MAX_SIZES = 16

AttentionSweep = collections.namedtuple(
    'AttentionSweep', ['means', 'decisions', 'summary', 'window_offsets', 'packed'])


def attention_sweep(s1, s2, labels, sizes, decoder='wta', handle=None):
  """The window-size sweep of infer.run_reduction_test in one launch set (td_attention_sweep).

  s1, s2: the two speakers' per-frame scores, float64 device tensors [frames, cols] (or [frames]) with
  unit column stride; labels: float64 device tensor of `frames` entries; sizes: up to 16 (width, hop)
  pairs; decoder: 'wta', 'stepped' or 'none'.  Returns an AttentionSweep of device tensors, all views of
  one buffer `packed` (one copy brings everything to the host: attention_sweep_host): means
  [3, total] float64 (speaker 1, speaker 2, labels), decisions [total] uint8, summary [sizes, 2] int64
  {end_first_section, correct}; size k's windows are [window_offsets[k], window_offsets[k + 1]).
  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  if decoder not in SWEEP_DECODERS:
    raise ValueError('attention_sweep: unknown decoder %r' % (decoder,))
  sizes = np.ascontiguousarray(np.asarray(sizes, np.int64).reshape(-1, 2), np.intc)
  ns = int(sizes.shape[0])
  if s1.dim() == 1:
    s1 = s1.reshape(-1, 1)
  if s2.dim() == 1:
    s2 = s2.reshape(-1, 1)
  frames, cols = int(s1.shape[0]), int(s1.shape[1])
  if tuple(s2.shape) != (frames, cols) or int(labels.numel()) != frames:
    raise ValueError('attention_sweep: scores of %s and %s with %d labels' %
                     (tuple(s1.shape), tuple(s2.shape), int(labels.numel())))
  for name, t in (('s1', s1), ('s2', s2), ('labels', labels)):
    if t.dtype != torch.float64 or t.device != h.device:
      raise TypeError('attention_sweep: %s must be a float64 tensor on %s, not %s on %s' %
                      (name, h.device, t.dtype, t.device))
  if cols > 1 and (s1.stride(1) != 1 or s2.stride(1) != 1):
    raise ValueError('attention_sweep: the columns of the scores must be contiguous')
  labels = labels.reshape(-1).contiguous()
  if frames == 0:       # (an empty tensor has no address to hand to the library: no window of any size)
    s1 = s2 = h.zeros((1, max(cols, 1)), 'float64')
    labels = h.zeros((1,), 'float64')
  offsets = np.zeros(ns + 1, np.int64)
  for k in range(ns):
    width, hop = int(sizes[k, 0]), int(sizes[k, 1])
    n = (frames - width) // hop + 1 if width >= 1 and hop >= 1 and frames >= width else 0
    offsets[k + 1] = offsets[k] + n
  total = int(offsets[-1])
  # one buffer: summary | means | decisions (each at a multiple of 8 bytes)
  o_means = 16 * ns
  o_dec = o_means + 24 * total
  packed = h.empty((max(o_dec + total, 8),), 'uint8')      # (every byte is written: two calls, equal buffers)
  base = packed.data_ptr()
  # (a one-column view's row stride is whatever the tensor says)
  ld1 = int(s1.stride(0)) if frames > 1 else max(cols, int(s1.stride(0)))
  ld2 = int(s2.stride(0)) if frames > 1 else max(cols, int(s2.stride(0)))
  h.check(h.lib.td_attention_sweep(
      h.ptr, _ptr(s1), ld1, _ptr(s2), ld2, cols, _ptr(labels), frames,
      sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ns, SWEEP_DECODERS[decoder],
      ctypes.c_void_p(base + o_means), ctypes.c_void_p(base + o_dec), ctypes.c_void_p(base)))
  return AttentionSweep(packed[o_means:o_dec].view(torch.float64).reshape(3, total),
                        packed[o_dec:o_dec + total], packed[:o_means].view(torch.int64).reshape(ns, 2),
                        offsets, packed)


def attention_sweep_host(sweep):
  """An AttentionSweep's means, decisions and summary as host arrays, through ONE copy."""
  host = sweep.packed.cpu().numpy()
  ns = int(sweep.summary.shape[0])
  total = int(sweep.window_offsets[-1])
  o_means = 16 * ns
  o_dec = o_means + 24 * total
  return AttentionSweep(host[o_means:o_dec].view(np.float64).reshape(3, total),
                        host[o_dec:o_dec + total], host[:o_means].view(np.int64).reshape(ns, 2),
                        sweep.window_offsets, None)


def ssd_state(num_trials, handle=None):
  """Fresh state of `num_trials` state-space decoders for decode_ssd(..., state=): zeros
  [num_trials, td_ssd_state_doubles()] float64 on the device."""
  h = handle or default_handle()
  return h.zeros((int(num_trials), int(h.lib.td_ssd_state_doubles())), 'float64')


def decode_ssd(s1, s2, window_offsets, outer_iter=20, inner_iter=1, newton_iter=10,
               forward_lag=0, backward_lag=13, offset=0.0, prior=None, handle=None, state=None):
  """prior = (rho_d[2], mu_d[2]) from tune_log_normal_priors, or None.  state (ssd_state): the
  decoders pick up where the previous call with that state left them (td_decode_ssd_stream)."""
  h = handle or default_handle()
  out = h.zeros((int(s1.shape[0]), 3), 'float64')
  wo, wo_p = _lib.i64_array(window_offsets)
  params, params_p = _lib.f64_array([outer_iter, inner_iter, newton_iter, forward_lag,
                                     backward_lag, offset, 1.0 if prior is not None else 0.0, 0.0])
  pr_p = None
  if prior is not None:
    pr, pr_p = _lib.f64_array(list(prior[0]) + list(prior[1]))
  if state is not None:
    h.check(h.lib.td_decode_ssd_stream(h.ptr, _ptr(s1), _ptr(s2), wo_p, len(wo) - 1, params_p, pr_p,
                                       _ptr(state), _ptr(out)))
    return out
  h.check(h.lib.td_decode_ssd(h.ptr, _ptr(s1), _ptr(s2), wo_p, len(wo) - 1, params_p, pr_p,
                              _ptr(out)))
  return out


def decode_fused(eeg, env, trial_offsets, w, b, pre, post, width, hop, corr, handle=None):
  """corr = [mean_truth, mean_pred, power] for speaker 1 then speaker 2."""
  h = handle or default_handle()
  _, total = window_layout(trial_offsets, width, hop)
  # (every element is written by decode_finalize_kernel: no zero-fill launches)
  scores = h.empty((total, 2), 'float64')
  decisions = h.empty((total,), 'uint8')
  offs, offs_p = _lib.i64_array(trial_offsets)
  cr, cr_p = _lib.f64_array(np.asarray(corr, np.float64).reshape(-1))
  h.check(h.lib.td_decode_fused(h.ptr, _ptr(eeg), eeg.stride(0), int(eeg.shape[1]), pre, post,
                                _ptr(w), _ptr(b), _ptr(env), env.stride(0), offs_p,
                                len(offs) - 1, int(width), int(hop), cr_p, _ptr(scores),
                                _ptr(decisions)))
  return scores, decisions


ONLINE_REDUCTIONS = ('first', 'mean', 'mean-squared', 'lda')     # one model output: td_online_push
ONLINE_MAX_CHANNELS, ONLINE_MAX_LAGS = 128, 64

OnlinePlan = collections.namedtuple(
    'OnlinePlan', ['emitted_before', 'emitted_after', 'first_window', 'new_windows'])
OnlinePush = collections.namedtuple('OnlinePush', ['scores', 'decisions', 'pred', 'frame', 'plan'])


# -- what the online push wrappers share (each stated once; the wrappers keep their own messages and their order)
_I64, _I32_I64 = (ctypes.c_int64,), (ctypes.c_int, ctypes.c_int64)


def _lib_values(name, args, outs=_I64):
  """The integers the library's host function `name`(*args, &out, ...) gives through out-parameters of the ctypes
  `outs`: called without a handle, its status checked."""
  values = [kind(0) for kind in outs]
  _lib.check(None, getattr(_lib.load(), name)(*args, *[ctypes.byref(v) for v in values]))
  return [int(v.value) for v in values]


def _row_block(t, n, sessions, width):
  """(pointer, row stride, session stride) of the rows [S, n, width] of a push; a null pointer without rows.  A
  tensor with one row, or with one session, carries in that dimension whatever stride its view left it -- 0 after an
  expand, anything after a slice -- and an absent tensor carries none, while the kernels refuse a row stride under
  the width and a session stride under a block.  A stride nothing steps by is therefore reported as that of packed
  rows: `width` between rows, max(n, 1) * width between sessions."""
  live = n > 0
  return (_ptr(t if live else None), int(t.stride(1)) if live and n > 1 else width,
          int(t.stride(0)) if live and sessions > 1 else max(n, 1) * width)


def _state_stride(state, sessions):
  """Bytes between the sessions' blocks of a [S, bytes] state; one session's stride may be anything: its length."""
  return int(state.stride(0)) if sessions > 1 else int(state.shape[1])


def _check_tensors(who, h, tensors, short=False):
  """TypeError for the first of (name, tensor, dtype) that is not a `dtype` tensor on the handle's device; None is
  skipped.  short: the dtype is named float32, not torch.float32 (the wrappers differ in this)."""
  for name, t, dtype in tensors:
    if t is not None and (t.dtype != dtype or t.device != h.device):
      raise TypeError('%s: %s must be a %s tensor on %s, not %s on %s' %
                      (who, name, str(dtype).replace('torch.', '') if short else dtype, h.device, t.dtype, t.device))


def _spare(h, count, dtype, wanted=True):
  """A flat output of count + 1 elements (None when not wanted): every element a push emits is written, and an empty
  tensor has no address -- hence one spare element, which _shaped drops."""
  return h.empty((count + 1,), dtype) if wanted else None


def _shaped(t, *shape):
  return t[:-1].reshape(shape) if t is not None else None


def _check_reduction(who, reduction, reductions, decoder):
  if reduction not in reductions:
    raise ValueError('%s: reduction %r (one of %s)' % (who, reduction, ', '.join(reductions)))
  if decoder not in SWEEP_DECODERS:
    raise ValueError('%s: unknown decoder %r' % (who, decoder))


def _check_decoder_rows(who, h, torch, sessions, c, eeg, env, model, corr, lda, state):
  """The rows of a push of online_push / dnn_online_push, once the model has said how many channels it implies:
  their shapes, every tensor's dtype and device (`model`: the wrapper's own triples, checked behind the rows), unit
  column strides.  Returns n."""
  n = 0 if eeg is None else int(eeg.shape[1])
  if eeg is not None and (tuple(eeg.shape) != (sessions, n, c) or env is None or
                          tuple(env.shape) != (sessions, n, 2)):
    raise ValueError('%s: eeg of %s and env of %s for %d sessions of %d channels' %
                     (who, tuple(eeg.shape), None if env is None else tuple(env.shape), sessions, c))
  _check_tensors(who, h, (('eeg', eeg, torch.float32), ('env', env, torch.float32)) + model +
                 (('corr', corr, torch.float64), ('lda', lda, torch.float64), ('state', state, torch.uint8)))
  if n > 0 and (eeg.stride(2) != 1 and c > 1 or env.stride(2) != 1):
    raise ValueError('%s: the columns of eeg and env must be contiguous' % who)
  return n


def _decoder_push(who, h, push, model_args, sessions, eeg, env, n, c, pre, post, corr, lda, state, frames_before,
                  width, hop, reduction, decoder, flush, want_frames):
  """The rest of online_push / dnn_online_push behind their model checks: the statistics' shapes, the plan, the
  outputs, the launch and the OnlinePush.  push: the wrapper's library function, which takes model_args between the
  context and the statistics.  (The outputs are _spare's and _shaped's, written out: eight calls fewer per push.)"""
  if tuple(corr.shape) != (sessions, 2, 3) or (lda is not None and tuple(lda.shape) != (sessions, 3)):
    raise ValueError('%s: corr must be [%d, 2, 3] and lda [%d, 3]' % (who, sessions, sessions))
  corr = corr.contiguous()
  lda = lda.contiguous() if lda is not None else None
  plan = online_plan(frames_before, n, post, width, hop, flush)
  new, emitted = plan.new_windows, plan.emitted_after - plan.emitted_before
  scores = h.empty((2 * sessions * new + 1,), 'float64')
  decisions = h.empty((sessions * new + 1,), 'uint8')
  pred = h.empty((sessions * emitted + 1,), 'float32') if want_frames else None
  frame = h.empty((2 * sessions * emitted + 1,), 'float64') if want_frames else None
  h.check(push(
      h.ptr, sessions, *_row_block(eeg, n, sessions, c), *_row_block(env, n, sessions, 2), n, c, int(pre), int(post),
      *model_args, _ptr(corr), REDUCTIONS[reduction], _ptr(lda), int(width), int(hop), SWEEP_DECODERS[decoder],
      int(frames_before), 1 if flush else 0, _ptr(state), _state_stride(state, sessions),
      _ptr(scores), _ptr(decisions), _ptr(pred), _ptr(frame)))
  return OnlinePush(scores[:-1].reshape(2, sessions, new), decisions[:-1].reshape(sessions, new),
                    pred[:-1].reshape(sessions, emitted) if want_frames else None,
                    frame[:-1].reshape(2, sessions, emitted) if want_frames else None, plan)


def online_state_bytes(c, pre, post, width):
  """Bytes of one online session's state block (td_online_state_bytes); all zeros = a fresh session."""
  return _lib_values('td_online_state_bytes', (int(c), int(pre), int(post), int(width)))[0]


def online_plan(frames_before, n, post, width, hop, flush=False):
  """What a push of n frames behind `frames_before` pushed ones emits (td_online_plan, host integers):
  OnlinePlan(emitted_before, emitted_after, first_window, new_windows)."""
  return OnlinePlan(*_lib_values('td_online_plan', (int(frames_before), int(n), int(post), int(width), int(hop),
                                                    1 if flush else 0), _I64 * 4))


def online_push(eeg, env, w, b, corr, state, frames_before, pre, post, width, hop, reduction='first',
                lda=None, decoder='wta', flush=False, want_frames=False, handle=None):
  """One push of a bank of online decoding sessions, in one launch (td_online_push).

  eeg [S, n, c] and env [S, n, 2]: float32 device tensors with unit column stride (None for a flush
  without rows); w [S or 1, (pre + 1 + post) c] and b [S or 1] float32 (one row: the model every session
  shares); corr [S, 2, 3] float64 {mean_truth, mean_pred, power} per speaker; lda [S, 3] float64
  {lda_w, slope, intercept} for reduction 'lda'; state: uint8 device tensor [S, >= online_state_bytes()]
  with a row stride that is a multiple of 8, updated in place; frames_before: frames pushed so far.
  decoder 'wta', 'stepped' or 'none'.  Returns OnlinePush(scores [2, S, new] float64, decisions [S, new]
  uint8, pred [S, emitted] float32 and frame [2, S, emitted] float64 (None without want_frames), plan).
  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  _check_reduction('online_push', reduction, ONLINE_REDUCTIONS, decoder)
  sessions = int(state.shape[0])
  k = int(w.shape[1])
  nl = int(pre) + 1 + int(post)
  if nl < 1 or k % nl:
    raise ValueError('online_push: %d weights for %d lags' % (k, nl))
  c = k // nl
  n = _check_decoder_rows('online_push', h, torch, sessions, c, eeg, env,
                          (('w', w, torch.float32), ('b', b, torch.float32)), corr, lda, state)
  if int(w.shape[0]) not in (1, sessions) or int(b.numel()) != int(w.shape[0]):
    raise ValueError('online_push: %d models and %d biases for %d sessions' %
                     (int(w.shape[0]), int(b.numel()), sessions))
  w, b = w.contiguous(), b.reshape(-1).contiguous()
  shared = int(w.shape[0]) == 1
  return _decoder_push('online_push', h, h.lib.td_online_push,
                       (_ptr(w), 0 if shared else k, _ptr(b), 0 if shared else 1), sessions, eeg, env, n, c, pre, post,
                       corr, lda, state, frames_before, width, hop, reduction, decoder, flush, want_frames)


CCA_ONLINE_REDUCTIONS = ('first', 'second', 'mean', 'mean-squared', 'lda')     # td_cca_online_push
CCA_ONLINE_MAX_CHANNELS, CCA_ONLINE_MAX_FEATURES, CCA_ONLINE_MAX_DIMS = 128, 32, 16
CCA_ONLINE_LDS_BYTES = 163840                                                   # TD_CCA_ONLINE_LDS_BYTES

CcaOnlinePush = collections.namedtuple('CcaOnlinePush', ['scores', 'decisions', 'proj', 'frame', 'plan'])


def cca_online_state_bytes(c1, pre1, post1, c2, pre2, post2, width):
  """Bytes of one CCA online session's state block (td_cca_online_state_bytes); all zeros = a fresh session."""
  return _lib_values('td_cca_online_state_bytes', (int(c1), int(pre1), int(post1), int(c2), int(pre2), int(post2),
                                                   int(width)))[0]


def cca_online_lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, emitted=64):
  """(frames per pass, LDS bytes) of a td_cca_online_push launch that emits `emitted` frames
  (td_cca_online_lds_bytes); ValueError with the byte budget for a shape that does not fit at a pass of one."""
  return tuple(_lib_values('td_cca_online_lds_bytes', (int(c1), int(pre1), int(post1), int(c2), int(pre2), int(post2),
                                                       int(dims), int(emitted)), _I32_I64))


def cca_online_push(eeg, feat1, feat2, mean_x, rot_x, mean_y, rot_y, corr, state, frames_before, pre1, post1,
                    pre2, post2, width, hop, reduction='first', lda=None, decoder='wta', flush=False,
                    want_frames=False, handle=None):
  """One push of a bank of online CCA decoding sessions, in one launch (td_cca_online_push).

  eeg [S, n, c1], feat1 and feat2 [S, n, c2]: float32 device tensors with unit column stride (None for a
  flush without rows; the two feature tensors share their strides); mean_x [M, k1], rot_x [M, k1, dims],
  mean_y [M, k2], rot_y [M, k2, dims] float32 with M = S or 1 (one model for every session), k1 =
  c1 (pre1 + 1 + post1), k2 = c2 (pre2 + 1 + post2); corr [S, 2, 3, dims] float64 {mean_a, mean_b, power}
  per speaker; lda [S, dims + 2] float64 {weights, slope, intercept} for reduction 'lda'; state: uint8 device
  tensor [S, >= cca_online_state_bytes()] with a row stride that is a multiple of 8, updated in place.
  Returns CcaOnlinePush(scores [2, S, new] float64, decisions [S, new] uint8, proj [S, emitted, 3 dims]
  float32 (a | b1 | b2) and frame [2, S, emitted] float64 (None without want_frames), plan) with
  plan = online_plan(frames_before, n, max(post1, post2), ...).  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  _check_reduction('cca_online_push', reduction, CCA_ONLINE_REDUCTIONS, decoder)
  sessions = int(state.shape[0])
  pre1, post1, pre2, post2 = int(pre1), int(post1), int(pre2), int(post2)
  nl1, nl2 = pre1 + 1 + post1, pre2 + 1 + post2
  if rot_x.dim() != 3 or rot_y.dim() != 3 or mean_x.dim() != 2 or mean_y.dim() != 2:
    raise ValueError('cca_online_push: the means are [M, k] and the rotations [M, k, dims]')
  models, k1, dims = (int(v) for v in rot_x.shape)
  k2 = int(rot_y.shape[1])
  if (nl1 < 1 or nl2 < 1 or k1 % nl1 or k2 % nl2 or tuple(rot_y.shape) != (models, k2, dims) or
      tuple(mean_x.shape) != (models, k1) or tuple(mean_y.shape) != (models, k2) or models not in (1, sessions)):
    raise ValueError('cca_online_push: rotations of %s and %s with means of %s and %s for %d + %d lags and %d '
                     'sessions' % (tuple(rot_x.shape), tuple(rot_y.shape), tuple(mean_x.shape),
                                   tuple(mean_y.shape), nl1, nl2, sessions))
  c1, c2 = k1 // nl1, k2 // nl2
  n = 0 if eeg is None else int(eeg.shape[1])
  if eeg is not None and (tuple(eeg.shape) != (sessions, n, c1) or feat1 is None or feat2 is None or
                          tuple(feat1.shape) != (sessions, n, c2) or tuple(feat2.shape) != (sessions, n, c2)):
    raise ValueError('cca_online_push: eeg of %s and features of %s and %s for %d sessions of %d channels and %d '
                     'features' % (tuple(eeg.shape), None if feat1 is None else tuple(feat1.shape),
                                   None if feat2 is None else tuple(feat2.shape), sessions, c1, c2))
  _check_tensors('cca_online_push', h, (
      ('eeg', eeg, torch.float32), ('feat1', feat1, torch.float32), ('feat2', feat2, torch.float32),
      ('mean_x', mean_x, torch.float32), ('rot_x', rot_x, torch.float32), ('mean_y', mean_y, torch.float32),
      ('rot_y', rot_y, torch.float32), ('corr', corr, torch.float64), ('lda', lda, torch.float64),
      ('state', state, torch.uint8)))
  if n > 0:
    if (c1 > 1 and eeg.stride(2) != 1) or (c2 > 1 and (feat1.stride(2) != 1 or feat2.stride(2) != 1)):
      raise ValueError('cca_online_push: the columns of eeg and the features must be contiguous')
    if feat2.stride() != feat1.stride():      # (one pair of strides serves both speakers)
      feat1, feat2 = feat1.contiguous(), feat2.contiguous()
  if tuple(corr.shape) != (sessions, 2, 3, dims) or (lda is not None and tuple(lda.shape) != (sessions, dims + 2)):
    raise ValueError('cca_online_push: corr must be [%d, 2, 3, %d] and lda [%d, %d]' %
                     (sessions, dims, sessions, dims + 2))
  mean_x, rot_x, mean_y, rot_y = (t.contiguous() for t in (mean_x, rot_x, mean_y, rot_y))
  corr = corr.contiguous()
  lda = lda.contiguous() if lda is not None else None
  plan = online_plan(frames_before, n, max(post1, post2), width, hop, flush)
  emitted = plan.emitted_after - plan.emitted_before
  new = plan.new_windows
  # (_spare's and _shaped's, written out as in _decoder_push: eight calls fewer per push)
  scores = h.empty((2 * sessions * new + 1,), 'float64')
  decisions = h.empty((sessions * new + 1,), 'uint8')
  proj = h.empty((sessions * emitted * 3 * dims + 1,), 'float32') if want_frames else None
  frame = h.empty((2 * sessions * emitted + 1,), 'float64') if want_frames else None
  feat1_p, feat_row, feat_session = _row_block(feat1, n, sessions, c2)     # (one pair of strides for both speakers)
  h.check(h.lib.td_cca_online_push(
      h.ptr, sessions, *_row_block(eeg, n, sessions, c1), feat1_p, _ptr(feat2 if n > 0 else None), feat_row,
      feat_session, n, c1, pre1, post1, c2, pre2, post2, dims, _ptr(mean_x), _ptr(rot_x), _ptr(mean_y), _ptr(rot_y),
      0 if models == 1 else 1, _ptr(corr), REDUCTIONS[reduction], _ptr(lda), int(width), int(hop),
      SWEEP_DECODERS[decoder], int(frames_before), 1 if flush else 0, _ptr(state), _state_stride(state, sessions),
      _ptr(scores), _ptr(decisions), _ptr(proj), _ptr(frame)))
  return CcaOnlinePush(scores[:-1].reshape(2, sessions, new), decisions[:-1].reshape(sessions, new),
                       proj[:-1].reshape(sessions, emitted, 3 * dims) if want_frames else None,
                       frame[:-1].reshape(2, sessions, emitted) if want_frames else None, plan)


DNN_ONLINE_MAX_HIDDEN, DNN_ONLINE_MAX_UNITS, DNN_ONLINE_MAX_INPUTS = 4, 64, 8192     # td_mlp_*'s limits
DNN_ONLINE_LDS_BYTES = 163840                                                         # TD_FC_ONLINE_LDS_BYTES


def dnn_param_count(k, hidden):
  """Parameters of the packed buffer [W1, b1, W2, b2, ...] of a regressor with k inputs and one output."""
  widths = [int(k)] + [int(v) for v in hidden] + [1]
  return sum(widths[i] * widths[i + 1] + widths[i + 1] for i in range(len(widths) - 1))


def dnn_online_lds_bytes(c, pre, post, hidden, emitted=64):
  """(frames per pass, LDS bytes) of a td_fc_online_push launch that emits `emitted` frames
  (td_fc_online_lds_bytes); ValueError for a shape outside the limits or over the byte budget."""
  hid, hid_p = _i32_array(list(hidden) or [0])
  return tuple(_lib_values('td_fc_online_lds_bytes', (int(c), int(pre), int(post), len(hidden), hid_p, int(emitted)),
                           _I32_I64))


def dnn_online_push(eeg, env, params, hidden, corr, state, frames_before, pre, post, width, hop, reduction='first',
                    lda=None, decoder='wta', flush=False, want_frames=False, handle=None):
  """One push of a bank of online decoding sessions around fully connected regressors, in one launch
  (td_fc_online_push).

  eeg, env, corr, lda, state, frames_before, width, hop, reduction, decoder, flush: as online_push.  params [S or 1,
  P] float32: the packed parameters of td_mlp_* ([W1, b1, W2, b2, ...], one output) of a network with the hidden
  layers `hidden` on c (pre + 1 + post) inputs; one row: the model every session shares.  Returns
  OnlinePush(scores [2, S, new] float64, decisions [S, new] uint8, pred [S, emitted] float32 -- mlp_forward's bits
  -- and frame [2, S, emitted] float64 (None without want_frames), plan).  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  _check_reduction('dnn_online_push', reduction, ONLINE_REDUCTIONS, decoder)
  hidden = [int(v) for v in hidden]
  sessions = int(state.shape[0])
  nl = int(pre) + 1 + int(post)
  if params.dim() != 2 or int(params.shape[0]) not in (1, sessions):
    raise ValueError('dnn_online_push: params of %s for %d sessions ([S or 1, P])' % (tuple(params.shape), sessions))
  # P = k h1 + the rest: k from the parameter count
  first = hidden[0] if hidden else 1
  rest = dnn_param_count(0, hidden)
  count = int(params.shape[1])
  k = (count - rest) // first if first > 0 else 0
  if nl < 1 or k < 1 or k % nl or dnn_param_count(k, hidden) != count:
    raise ValueError('dnn_online_push: %d parameters for hidden layers %s on %d lags' % (count, hidden, nl))
  c = k // nl
  n = _check_decoder_rows('dnn_online_push', h, torch, sessions, c, eeg, env, (('params', params, torch.float32),),
                          corr, lda, state)
  if params.stride(1) != 1 and count > 1:
    params = params.contiguous()
  shared = int(params.shape[0]) == 1
  hid, hid_p = _i32_array(hidden or [0])
  return _decoder_push('dnn_online_push', h, h.lib.td_fc_online_push,
                       (hid_p, len(hidden), _ptr(params), 0 if shared else int(params.stride(0))), sessions, eeg, env,
                       n, c, pre, post, corr, lda, state, frames_before, width, hop, reduction, decoder, flush,
                       want_frames)


def sos_filter(x, file_offsets, sos, zi, stage_split, state, reset, out_rows=None, out_offsets=None, handle=None):
  """The SOS cascade over x [N, C] (float32 / float64 device tensor), files concatenated along time:
  float64 output [N, C], or only the file-local rows out_rows (device int64, file f's at
  out_offsets[f]:out_offsets[f+1]) -- the resample fused into the store.  state [S, 2, C] float64 on the
  device carries the filter between calls (td_sos_filter)."""
  h = handle or default_handle()
  offs, offs_p = _lib.i64_array(file_offsets)
  sos_a, sos_p = _lib.f64_array(sos)
  zi_a, zi_p = _lib.f64_array(zi)
  c = int(x.shape[1])
  if out_rows is not None:
    oo, oo_p = _lib.i64_array(out_offsets)
    y = h.empty((int(oo[-1]), c), 'float64')
  else:
    oo_p = None
    y = h.empty((int(offs[-1]), c), 'float64')
  is64 = 1 if x.dtype == _torch().float64 else 0
  h.check(h.lib.td_sos_filter(h.ptr, _ptr(x), is64, x.stride(0), c, offs_p, len(offs) - 1, sos_p,
                              int(sos_a.shape[0]), int(stage_split), zi_p, 1 if reset else 0, _ptr(state),
                              _ptr(out_rows), oo_p, _ptr(y), y.stride(0)))
  return y


def audio_intensity(x, buf, rows_out, fs_in, fs_out, half_window, square, post, exponent, windows=False,
                    handle=None):
  """The windowed means of AudioFeatures.audio_resample over [buf ; f(x)] (td_audio_intensity): float64
  [rows_out, C].  x [N, C] float32 / float64 device tensor; buf [B, C] float64 (contiguous) or None;
  f(x) = float32(x)^2 when square; post: sqrt then ** exponent fused into the store.  windows=True also
  returns the (t1, t2) of every row as a device int64 [rows_out, 2]."""
  h = handle or default_handle()
  c = int(x.shape[1])
  y = h.empty((int(rows_out), c), 'float64')
  win = h.empty((int(rows_out), 2), 'int64') if windows else None
  nb = int(buf.shape[0]) if buf is not None else 0
  is64 = 1 if x.dtype == _torch().float64 else 0
  h.check(h.lib.td_audio_intensity(h.ptr, _ptr(buf), nb, _ptr(x), is64, x.stride(0), int(x.shape[0]), c,
                                   1 if square else 0, int(rows_out), float(fs_in), float(fs_out),
                                   float(half_window), 1 if post else 0, float(exponent), _ptr(y), _ptr(win)))
  return (y, win) if windows else y


def audio_passthrough(x, buf, row_begin, row_end, square, post, exponent, dtype='float64', handle=None):
  """Rows [row_begin, row_end) of [buf ; f(x)] as `dtype` -- the pass-through of audio_resample and its
  carried buffer (td_audio_passthrough).  post 0: as they are; 1: sqrt and ** exponent in `dtype`; 2 (float64
  only): sqrt in float32, ** exponent in float64."""
  h = handle or default_handle()
  c = int(x.shape[1])
  y = h.empty((int(row_end) - int(row_begin), c), dtype)
  o32, o64 = (y, None) if dtype == 'float32' else (None, y)
  nb = int(buf.shape[0]) if buf is not None else 0
  is64 = 1 if x.dtype == _torch().float64 else 0
  h.check(h.lib.td_audio_passthrough(h.ptr, _ptr(buf), nb, _ptr(x), is64, x.stride(0), int(x.shape[0]), c,
                                     1 if square else 0, int(row_begin), int(row_end), int(post),
                                     float(exponent), _ptr(o32), _ptr(o64)))
  return y


def audio_spectrogram(wave, seg, hop, nfft, taps, frames, handle=None):
  """AudioFeatures.compute_spectrogram of a float32 device wave [n] (td_audio_spectrogram): float64
  [nfft // 2 + 1, frames]."""
  h = handle or default_handle()
  taps_a, taps_p = _lib.f64_array(taps)
  y = h.empty((int(nfft) // 2 + 1, int(frames)), 'float64')
  h.check(h.lib.td_audio_spectrogram(h.ptr, _ptr(wave), int(wave.shape[0]), int(seg), int(hop), int(nfft), taps_p,
                                     int(taps_a.shape[0]), int(frames), _ptr(y)))
  return y


def _check_rows(t, what):
  """A 2-D float32 / float64 device tensor whose rows are contiguous."""
  torch = _torch()
  if t.dim() != 2 or t.dtype not in (torch.float32, torch.float64) or (t.shape[1] > 1 and t.stride(1) != 1):
    raise ValueError('%s: a 2-D float32 / float64 device tensor with contiguous rows is needed, not %s %s' %
                     (what, tuple(t.shape), t.dtype))
  return t


def _row_stride(t):
  """Elements between rows (a one-row tensor's stride may be anything: report its width)."""
  return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def ingest_moments(arrays, handle=None):
  """The joint two-pass float64 moments of a list of [rows_i, W] float32 / float64 device tensors (row-strided
  is fine): a device float64 [2 + 2 W] = mean and std of everything, the W column means, the W column stds
  (td_ingest_moments)."""
  h = handle or default_handle()
  arrays = [_check_rows(a, 'ingest_moments') for a in arrays]
  width = int(arrays[0].shape[1])
  if any(int(a.shape[1]) != width for a in arrays):
    raise ValueError('ingest_moments: the arrays differ in width: %s' % [tuple(a.shape) for a in arrays])
  n = len(arrays)
  ptrs = (ctypes.c_void_p * n)(*[a.data_ptr() for a in arrays])
  keep_rows_p, rows_p = _lib.i64_array([int(a.shape[0]) for a in arrays])
  keep_ld_p, ld_p = _lib.i64_array([_row_stride(a) for a in arrays])
  keep_f64_p, f64_p = _i32_array([1 if a.dtype == _torch().float64 else 0 for a in arrays])
  out = h.empty((2 + 2 * width,), 'float64')
  h.check(h.lib.td_ingest_moments(h.ptr, ptrs, rows_p, ld_p, f64_p, n, width, _ptr(out)))
  return out


def ingest_normalize(a, mean, std, sub_f64, out_f64, divide=True, handle=None):
  """(a - mean) / std of a [rows, W] float32 / float64 device tensor (td_ingest_normalize).  mean / std: one value
  or W values (host).  sub_f64 / out_f64: the dtype of the subtraction and of the division (and the result), as
  numpy would choose them; divide=False only centres."""
  h = handle or default_handle()
  a = _check_rows(a, 'ingest_normalize')
  rows, width = int(a.shape[0]), int(a.shape[1])
  mean_a, mean_p = _lib.f64_array(np.asarray(mean, np.float64).reshape(-1))
  std_a, std_p = _lib.f64_array(np.asarray(std, np.float64).reshape(-1))
  if mean_a.size != std_a.size or mean_a.size not in (1, width):
    raise ValueError('ingest_normalize: mean and std need 1 or %d values, not %d and %d' %
                     (width, mean_a.size, std_a.size))
  per_column = 1 if (mean_a.size == width and width > 1) else 0
  out = h.empty((rows, width), 'float64' if out_f64 else 'float32')
  h.check(h.lib.td_ingest_normalize(h.ptr, _ptr(a), 1 if a.dtype == _torch().float64 else 0, _row_stride(a), rows,
                                    width, mean_p, std_p, per_column, 1 if sub_f64 else 0, 1 if out_f64 else 0,
                                    1 if divide else 0, _ptr(out), width))
  return out


def tfrecord_route(stride):
  """(staged, records per workgroup, lanes per record's CRC) of tfrecord_encode for records of `stride` bytes
  (td_tfrecord_route).  staged False: the record does not fit the LDS staging area; one workgroup writes each
  record directly.  Needs the library, not a GPU."""
  lib = _lib.load()
  staged, group, lanes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
  if lib.td_tfrecord_route(int(stride), ctypes.byref(staged), ctypes.byref(group), ctypes.byref(lanes)) != 0:
    raise ValueError('tfrecord_route: bad record stride %d' % stride)
  return bool(staged.value), int(group.value), int(lanes.value)


def tfrecord_encode(template, features, frames, handle=None):
  """The TFRecord file image of one trial as a device uint8 [frames * len(template)] tensor
  (td_tfrecord_encode).  template: the bytes of one record with zero payloads (tfrecord.record_template);
  features: [(device tensor [frames, width] float32 / float64, payload byte offset, reversed)]."""
  h = handle or default_handle()
  template = bytes(template)
  stride, n = len(template), len(features)
  tensors = [_check_rows(t, 'tfrecord_encode') for t, _, _ in features]
  if any(int(t.shape[0]) != int(frames) for t in tensors):
    raise ValueError('tfrecord_encode: every feature needs %d rows: %s' % (frames, [tuple(t.shape) for t in tensors]))
  ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
  keep_ld_p, ld_p = _lib.i64_array([_row_stride(t) for t in tensors])
  keep_width_p, width_p = _i32_array([int(t.shape[1]) for t in tensors])
  keep_off_p, off_p = _i32_array([int(o) for _, o, _ in features])
  keep_f64_p, f64_p = _i32_array([1 if t.dtype == _torch().float64 else 0 for t in tensors])
  keep_rev_p, rev_p = _i32_array([1 if r else 0 for _, _, r in features])
  out = h.empty((int(frames) * stride,), 'uint8')
  h.check(h.lib.td_tfrecord_encode(h.ptr, template, stride, n, ptrs, ld_p, width_p, off_p, f64_p, rev_p, int(frames),
                                   _ptr(out)))
  return out


TFRECORD_MAX_OUTPUTS = 16


def tfrecord_decode(image, plan, outputs, handle=None, status=None):
  """Checks the TFRecord file image `image` (device uint8, 16-byte aligned, plan['frames'] * plan['stride'] bytes)
  and scatters its float payloads (td_tfrecord_decode).  plan: tfrecord.decode_plan of the file; outputs:
  [(feature name, destination float32 device tensor with contiguous rows, first row, column)], at most
  TFRECORD_MAX_OUTPUTS, a feature as often as wanted.  Returns the status, a device int64 [1] (`status`, when
  given): -1 when every record passed, else (record << 2 | kind) of the lowest failing record, kind 1 = its bytes
  outside the payloads differ from the first record's, 2 = its data CRC.  Nothing waits for the device here; the
  destinations of a file that failed are unspecified."""
  torch = _torch()
  h = handle or default_handle()
  stride, frames = int(plan['stride']), int(plan['frames'])
  if image.dtype != torch.uint8 or image.dim() != 1 or not image.is_contiguous() or image.numel() < frames * stride:
    raise ValueError('tfrecord_decode: a contiguous uint8 device image of %d bytes is needed' % (frames * stride))
  where = {name: (offset, count) for name, offset, count in plan['layout']}
  n = len(outputs)
  ptrs, lds, cols, offs, counts = [], [], [], [], []
  for name, dst, row0, col in outputs:
    offset, count = where[name]
    row0, col = int(row0), int(col)
    if (dst.dim() != 2 or dst.dtype != torch.float32 or (dst.shape[1] > 1 and dst.stride(1) != 1) or row0 < 0 or
        col < 0 or row0 + frames > dst.shape[0] or col + count > dst.shape[1]):
      raise ValueError('tfrecord_decode: %s: rows [%d, +%d) x columns [%d, +%d) do not fit a float32 %s tensor with '
                       'contiguous rows' % (name, row0, frames, col, count, tuple(dst.shape)))
    ld = _row_stride(dst)
    ptrs.append(dst.data_ptr() + 4 * row0 * ld)
    lds.append(ld); cols.append(col); offs.append(offset); counts.append(count)
  if status is None:
    with torch.cuda.stream(h._stream):     # (the handle's stream need not be torch's current one)
      status = torch.full((1,), -1, dtype=torch.int64, device=h.device)
  ptr_p = (ctypes.c_void_p * max(n, 1))(*ptrs)
  keep_ld, ld_p = _lib.i64_array(lds)
  keep_col, col_p = _i32_array(cols)
  keep_off, off_p = _i32_array(offs)
  keep_count, count_p = _i32_array(counts)
  h.check(h.lib.td_tfrecord_decode(h.ptr, _ptr(image), stride, frames, bytes(plan['template']), bytes(plan['mask']), n,
                                   off_p, count_p, ptr_p, ld_p, col_p, _ptr(status)))
  return status


RAW_INT16, RAW_FLOAT32 = 0, 1
RAW_MAX_SIGNALS = 1024
COLUMNS_MAX_SOURCES = 1024


def raw_route(samples_per_record, sample_bytes, record_bytes):
  """(transposed, records per workgroup) of raw_decode for records of `record_bytes` bytes whose signals hold
  `samples_per_record` samples of `sample_bytes` bytes each (td_raw_route).  transposed False: the direct route,
  loads in runs of one signal's samples.  Needs the library, not a GPU."""
  lib = _lib.load()
  transposed, tile = ctypes.c_int(0), ctypes.c_int(0)
  if lib.td_raw_route(int(samples_per_record), int(sample_bytes), int(record_bytes), ctypes.byref(transposed),
                      ctypes.byref(tile)) != 0:
    raise ValueError('raw_route: bad sizes (%s samples of %s bytes in a record of %s bytes)' %
                     (samples_per_record, sample_bytes, record_bytes))
  return bool(transposed.value), int(tile.value)


def raw_decode(image, data_offset, records, record_bytes, samples_per_record, sample_kind, signal_offsets, scales,
               offsets=None, out=None, handle=None):
  """The signals of a raw recording's file image as a channel-major device matrix [signals, records *
  samples_per_record] (td_raw_decode).  image: contiguous device uint8, 16-byte aligned; record r is the
  record_bytes bytes at data_offset + r * record_bytes, signal s its samples_per_record samples (RAW_INT16 or
  RAW_FLOAT32, little-endian) from byte signal_offsets[s] of the record.  offsets None: float32,
  float32(x) * float32(scales[s]); else float64, scales[s] * (offsets[s] + float64(x)).  out: a matrix of that dtype
  with contiguous rows of at least records * samples_per_record elements, filled and returned.  Waits for nothing."""
  torch = _torch()
  h = handle or default_handle()
  if image.dtype != torch.uint8 or image.dim() != 1 or not image.is_contiguous():
    raise ValueError('raw_decode: a contiguous uint8 device image is needed')
  if sample_kind not in (RAW_INT16, RAW_FLOAT32):
    raise ValueError('raw_decode: unknown sample kind %s' % (sample_kind,))
  n, records = int(samples_per_record), int(records)
  num = len(signal_offsets)
  if not 1 <= num <= RAW_MAX_SIGNALS:
    raise ValueError('raw_decode: 1 .. %d signals, not %d' % (RAW_MAX_SIGNALS, num))
  arith = 0 if offsets is None else 1
  if len(scales) != num or (arith and len(offsets) != num):
    raise ValueError('raw_decode: %d signals need as many scales and offsets' % num)
  dtype = torch.float64 if arith else torch.float32
  if out is None:
    out = h.empty((num, records * n), 'float64' if arith else 'float32')
  if (out.dim() != 2 or out.dtype != dtype or out.shape[0] < num or out.shape[1] < records * n or
      (out.shape[1] > 1 and out.stride(1) != 1)):
    raise ValueError('raw_decode: a %s [>= %d, >= %d] matrix with contiguous rows is needed, not %s %s' %
                     (dtype, num, records * n, tuple(out.shape), out.dtype))
  keep_off, off_p = _lib.i64_array([int(o) for o in signal_offsets])
  keep_scale, scale_p = _lib.f64_array(np.asarray(scales, np.float64).reshape(-1))
  keep_add, add_p = _lib.f64_array(np.zeros(num) if offsets is None else np.asarray(offsets, np.float64).reshape(-1))
  h.check(h.lib.td_raw_decode(h.ptr, _ptr(image), int(image.numel()), int(data_offset), records, int(record_bytes), n,
                              int(sample_kind), num, off_p, scale_p, add_p, arith, _ptr(out), _row_stride(out)))
  return out


def raw24_decode(image, data_offset, records, record_bytes, samples_per_record, signal_offsets, scales, offsets,
                 out=None, handle=None):
  """The signals of a BDF recording's file image as a float64 channel-major device matrix [signals, records *
  samples_per_record] (td_raw24_decode): scales[s] * (offsets[s] + float64(x)), x the sign-extended 24-bit
  little-endian sample.  The layout is raw_decode's, but data_offset, record_bytes and the signal offsets may be any
  byte values.  image: contiguous device uint8, 16-byte aligned.  out: a float64 matrix with contiguous rows of at
  least records * samples_per_record elements, filled and returned.  Waits for nothing."""
  torch = _torch()
  h = handle or default_handle()
  if image.dtype != torch.uint8 or image.dim() != 1 or not image.is_contiguous():
    raise ValueError('raw24_decode: a contiguous uint8 device image is needed')
  n, records = int(samples_per_record), int(records)
  num = len(signal_offsets)
  if not 1 <= num <= RAW_MAX_SIGNALS:
    raise ValueError('raw24_decode: 1 .. %d signals, not %d' % (RAW_MAX_SIGNALS, num))
  if len(scales) != num or len(offsets) != num:
    raise ValueError('raw24_decode: %d signals need as many scales and offsets' % num)
  if out is None:
    out = h.empty((num, max(records * n, 0)), 'float64')
  if (out.dim() != 2 or out.dtype != torch.float64 or out.shape[0] < num or out.shape[1] < records * n or
      (out.shape[1] > 1 and out.stride(1) != 1)):
    raise ValueError('raw24_decode: a %s [>= %d, >= %d] matrix with contiguous rows is needed, not %s %s' %
                     (torch.float64, num, records * n, tuple(out.shape), out.dtype))
  keep_off, off_p = _lib.i64_array([int(o) for o in signal_offsets])
  keep_scale, scale_p = _lib.f64_array(np.asarray(scales, np.float64).reshape(-1))
  keep_add, add_p = _lib.f64_array(np.asarray(offsets, np.float64).reshape(-1))
  h.check(h.lib.td_raw24_decode(h.ptr, _ptr(image), int(image.numel()), int(data_offset), records, int(record_bytes),
                                n, num, off_p, scale_p, add_p, _ptr(out), _row_stride(out)))
  return out


CODE_MASK_MAX = 0xffffff


def code_onsets_plan(n):
  """(chunk, groups) of code_onsets for a signal of n samples: the samples one workgroup takes and the number of
  workgroups, ceil(n / chunk) (td_code_onsets_plan).  Needs the library, not a GPU."""
  lib = _lib.load()
  chunk, groups = ctypes.c_int(0), ctypes.c_int64(0)
  if lib.td_code_onsets_plan(int(n), ctypes.byref(chunk), ctypes.byref(groups)) != 0:
    raise ValueError('code_onsets_plan: bad size (%s samples)' % (n,))
  return int(chunk.value), int(groups.value)


def code_onsets(signal, mask=0xffff, handle=None):
  """(sample indices int64, codes int32) of the events of a trigger channel on the device, in increasing order of
  the index: code = int64(signal) & mask (truncation toward zero), an event wherever the code differs from the one
  before (0 before the first sample) and is not 0 (td_code_onsets_count, td_code_onsets_fill).  signal: a float64
  device tensor [n] or [n, 1] with any element stride (a column of a matrix is read where it lies).  The number of
  events (8 bytes) and the events come back; the signal does not."""
  torch = _torch()
  h = handle or default_handle()
  if signal.dim() == 2 and signal.shape[1] == 1:
    signal = signal[:, 0]
  if signal.dim() != 1 or signal.dtype != torch.float64 or not signal.is_cuda:
    raise ValueError('code_onsets: a float64 device tensor [n] or [n, 1] is needed, not %s %s' %
                     (tuple(signal.shape), signal.dtype))
  mask = int(mask)
  if not 0 < mask <= CODE_MASK_MAX:
    raise ValueError('code_onsets: a mask of %#x is outside 1 .. %#x' % (mask, CODE_MASK_MAX))
  n = int(signal.shape[0])
  stride = int(signal.stride(0)) if n > 1 else 1
  if stride < 1:
    raise ValueError('code_onsets: a signal with an element stride of %d' % stride)
  groups = code_onsets_plan(n)[1]
  with torch.cuda.stream(h._stream):
    offsets = h.empty((groups + 1,), 'int64')
    h.check(h.lib.td_code_onsets_count(h.ptr, _ptr(signal), n, stride, mask, _ptr(offsets)))
    total = int(offsets[groups:].cpu()[0])
    at, codes = h.empty((total,), 'int64'), h.empty((total,), 'int32')
    h.check(h.lib.td_code_onsets_fill(h.ptr, _ptr(signal), n, stride, mask, _ptr(offsets), total, _ptr(at),
                                      _ptr(codes)))
    return at.cpu().numpy(), codes.cpu().numpy()


def columns_route(num_sources, max_width):
  """Whether columns_assemble takes the tiled transpose for that many sources, the widest of `max_width` columns
  (td_columns_route).  Needs the library, not a GPU."""
  lib = _lib.load()
  transposed = ctypes.c_int(0)
  if lib.td_columns_route(int(num_sources), int(max_width), ctypes.byref(transposed)) != 0:
    raise ValueError('columns_route: bad sizes (%s sources, width %s)' % (num_sources, max_width))
  return bool(transposed.value)


def columns_assemble(sources, frames=None, out=None, handle=None):
  """[frames, sum of widths] float32 = the first `frames` rows (default: the fewest any has) of the [rows_k, w_k]
  float32 / float64 device tensors `sources` side by side, in one launch (td_columns_assemble); float64 is rounded
  to nearest even as astype does.  Waits for nothing."""
  h = handle or default_handle()
  sources = [_check_rows(s, 'columns_assemble') for s in sources]
  n = len(sources)
  if not 1 <= n <= COLUMNS_MAX_SOURCES:
    raise ValueError('columns_assemble: 1 .. %d sources, not %d' % (COLUMNS_MAX_SOURCES, n))
  fewest = min(int(s.shape[0]) for s in sources)
  frames = fewest if frames is None else int(frames)
  if not 0 <= frames <= fewest:
    raise ValueError('columns_assemble: %d frames of sources with %d rows' % (frames, fewest))
  width = sum(int(s.shape[1]) for s in sources)
  if out is None:
    out = h.empty((frames, width), 'float32')
  if (out.dim() != 2 or out.dtype != _torch().float32 or out.shape[0] < frames or out.shape[1] < width or
      (out.shape[1] > 1 and out.stride(1) != 1)):
    raise ValueError('columns_assemble: a float32 [>= %d, >= %d] matrix with contiguous rows is needed, not %s %s' %
                     (frames, width, tuple(out.shape), out.dtype))
  ptrs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in sources])
  keep_ld, ld_p = _lib.i64_array([_row_stride(s) for s in sources])
  keep_width, width_p = _i32_array([int(s.shape[1]) for s in sources])
  keep_f64, f64_p = _i32_array([1 if s.dtype == _torch().float64 else 0 for s in sources])
  h.check(h.lib.td_columns_assemble(h.ptr, n, ptrs, ld_p, width_p, f64_p, frames, _ptr(out), _row_stride(out)))
  return out


def sos_filter_plan(n_total, n_max, c, handle=None):
  """(chunk, scan levels) that sos_filter uses for files of n_total rows in all, the longest n_max, over c
  channels (td_sos_filter_plan)."""
  h = handle or default_handle()
  chunk, levels = ctypes.c_int(0), ctypes.c_int(0)
  rc = h.lib.td_sos_filter_plan(int(n_total), int(n_max), int(c), ctypes.byref(chunk), ctypes.byref(levels))
  if rc != 0:
    raise ValueError('sos_filter_plan: bad sizes (%d, %d, %d)' % (n_total, n_max, c))
  return int(chunk.value), int(levels.value)


def _i32_array(values):
  arr = np.ascontiguousarray(values, dtype=np.int32)
  return arr, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def reref_select(x, rows=None, groups=(), select=None, handle=None):
  """Re-referencing by groups and channel selection (td_reref_select): float64 [M, len(select)].
  groups: [(reference channels, channels to re-reference)] in order; rows: device int64 row gather."""
  h = handle or default_handle()
  c = int(x.shape[1])
  m = int(rows.shape[0]) if rows is not None else int(x.shape[0])
  sel = list(range(c)) if select is None else [int(v) for v in select]
  ref_ptr, ref_idx, ch_ptr, ch_idx = [0], [], [0], []
  for ref, chans in groups:
    ref_idx += [int(v) for v in ref]
    ch_idx += [int(v) for v in chans]
    ref_ptr.append(len(ref_idx))
    ch_ptr.append(len(ch_idx))
  keep = [_i32_array(v or [0]) for v in (ref_ptr, ref_idx, ch_ptr, ch_idx, sel)]
  z = h.empty((m, len(sel)), 'float64')
  is64 = 1 if x.dtype == _torch().float64 else 0
  h.check(h.lib.td_reref_select(h.ptr, _ptr(x), is64, x.stride(0), c, _ptr(rows), m, len(groups),
                                keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4][1], len(sel), _ptr(z),
                                z.stride(0)))
  return z


def mean_f64(z, handle=None):
  """The float64 mean of every entry of z, as a device scalar tensor (td_mean_f64)."""
  h = handle or default_handle()
  out = h.empty((1,), 'float64')
  h.check(h.lib.td_mean_f64(h.ptr, _ptr(z), int(z.shape[0]), int(z.shape[1]), z.stride(0), _ptr(out)))
  return out


def context_out(z, state, pre, post, mean, std, dtype='float32', handle=None):
  """[state ; (z - mean) / std] with pre / post rows of temporal context (td_context_out):
  returns (output [rows, (pre + post + 1) * C] of `dtype`, the new state [<= pre + post, C] float64)."""
  h = handle or default_handle()
  cs = int(z.shape[1])
  state_rows = int(state.shape[0]) if state is not None else 0
  rows = state_rows + int(z.shape[0]) - pre - post
  if rows < 0:
    raise ValueError('%d rows cannot hold %d + %d rows of temporal context' % (rows + pre + post, pre, post))
  if int(z.shape[0]) == 0:      # (a file that resampled to no rows: nothing to write, the state carries on)
    return h.empty((0, (pre + post + 1) * cs), dtype), state
  out = h.empty((rows, (pre + post + 1) * cs), dtype)
  keep = min(state_rows + int(z.shape[0]), pre + post)
  new_state = h.empty((keep, cs), 'float64') if keep else None
  o32, o64 = (out, None) if dtype == 'float32' else (None, out)
  h.check(h.lib.td_context_out(h.ptr, _ptr(z), int(z.shape[0]), cs, z.stride(0), _ptr(state), state_rows, int(pre),
                               int(post), float(mean), float(std), _ptr(o32), _ptr(o64), out.stride(0) if rows else
                               (pre + post + 1) * cs, _ptr(new_state)))
  return out, new_state


# ---------------------------------------------------------------- online front end
FRONTEND_MAX_CHANNELS, FRONTEND_MAX_SECTIONS, FRONTEND_MAX_GROUPS = 128, 16, 32    # td_frontend_push's limits
FRONTEND_LDS_BYTES = 49152                                                          # TD_FRONTEND_LDS_BYTES

FrontendPlan = collections.namedtuple('FrontendPlan', ['frames_before', 'frames_after', 'held'])
FrontendPush = collections.namedtuple('FrontendPush', ['out32', 'out64', 'plan'])


def frontend_state_bytes(c, num_sections):
  """Bytes of one front-end session's state block (td_frontend_state_bytes): the filter state [sections, 2, c], the
  held row and the last row, float64; all zeros = a fresh session."""
  return _lib_values('td_frontend_state_bytes', (int(c), int(num_sections)))[0]


def frontend_plan(rows_before, n, fs_in, fs_out, flush=False):
  """What a push of n raw rows behind `rows_before` pushed ones emits (td_frontend_plan, host arithmetic in the
  reference's float64 order): FrontendPlan(frames_before, frames_after, held)."""
  return FrontendPlan(*_lib_values('td_frontend_plan', (int(rows_before), int(n), float(fs_in), float(fs_out),
                                                        1 if flush else 0), _I64 * 3))


def frontend_lds_bytes(c, num_groups, emitted=64):
  """(frames per pass, LDS bytes) of a td_frontend_push launch that emits `emitted` frames (td_frontend_lds_bytes)."""
  return tuple(_lib_values('td_frontend_lds_bytes', (int(c), int(num_groups), int(emitted)), _I32_I64))


def frontend_push(x, sos, stage_split, zi, fs_in, fs_out, groups, select, mean, std, state, rows_before, c=None,
                  flush=False, want32=True, want64=False, handle=None):
  """One push of a bank of online front-end sessions, in one launch (td_frontend_push).

  x [S, n, c]: float32 or float64 device tensor with unit column stride (None for a flush without rows: give c);
  sos [sections, 6] and zi [sections, 2] host float64 (None: no filter), stage_split as sos_filter's; groups
  [(reference channels, channels to re-reference)] and select (None: every channel) as reref_select's; mean and
  std float64 device tensors of S values or of one that every session shares; state: uint8 device tensor
  [S, >= frontend_state_bytes()] with a row stride that is a multiple of 8, updated in place; rows_before: raw rows
  pushed so far (0: the filter resets).  Returns FrontendPush(out32 [S, m, cs] float32, out64 [S, m, cs] float64
  (None when not wanted), plan).  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  sessions = int(state.shape[0])
  n = 0 if x is None else int(x.shape[1])
  if x is not None:
    c = int(x.shape[2])
    if x.dim() != 3 or int(x.shape[0]) != sessions:
      raise ValueError('frontend_push: x of %s for %d sessions' % (tuple(x.shape), sessions))
    if x.dtype not in (torch.float32, torch.float64) or x.device != h.device:
      raise TypeError('frontend_push: x must be a float32 or float64 tensor on %s, not %s on %s' %
                      (h.device, x.dtype, x.device))
    if n > 0 and c > 1 and x.stride(2) != 1:
      raise ValueError('frontend_push: the columns of x must be contiguous')
  if c is None:
    raise ValueError('frontend_push: a flush without rows needs the channel count c')
  _check_tensors('frontend_push', h, (('mean', mean, torch.float64), ('std', std, torch.float64),
                                      ('state', state, torch.uint8)))
  mean, std = mean.reshape(-1).contiguous(), std.reshape(-1).contiguous()
  if int(mean.numel()) not in (1, sessions) or int(std.numel()) != int(mean.numel()):
    raise ValueError('frontend_push: %d means and %d stds for %d sessions' %
                     (int(mean.numel()), int(std.numel()), sessions))
  if not want32 and not want64:
    raise ValueError('frontend_push: neither the float32 nor the float64 output is wanted')
  sections = 0 if sos is None else int(np.shape(sos)[0])
  sos_a, sos_p = _lib.f64_array(sos if sections else np.zeros((1, 6)))
  zi_a, zi_p = _lib.f64_array(zi if sections else np.zeros((1, 2)))
  sel = list(range(int(c))) if select is None else [int(v) for v in select]
  ref_ptr, ref_idx, ch_ptr, ch_idx = [0], [], [0], []
  for ref, chans in groups:
    ref_idx += [int(v) for v in ref]
    ch_idx += [int(v) for v in chans]
    ref_ptr.append(len(ref_idx))
    ch_ptr.append(len(ch_idx))
  keep = [_i32_array(v or [0]) for v in (ref_ptr, ref_idx, ch_ptr, ch_idx, sel)]
  plan = frontend_plan(rows_before, n, fs_in, fs_out, flush)
  m, cs = plan.frames_after - plan.frames_before, len(sel)
  out32 = _spare(h, sessions * m * cs, 'float32', want32)
  out64 = _spare(h, sessions * m * cs, 'float64', want64)
  x_p, x_row, x_session = _row_block(x, n, sessions, int(c))
  h.check(h.lib.td_frontend_push(
      h.ptr, sessions, x_p, 1 if n > 0 and x.dtype == torch.float64 else 0, x_row, x_session,
      n, int(c), sos_p if sections else None, sections, int(stage_split), zi_p if sections else None, float(fs_in),
      float(fs_out), len(groups), keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4][1], cs, _ptr(mean),
      _ptr(std), 0 if int(mean.numel()) == 1 else 1, int(rows_before), 1 if flush else 0, _ptr(state),
      _state_stride(state, sessions), _ptr(out32), _ptr(out64), cs, max(m, 1) * cs))
  return FrontendPush(_shaped(out32, sessions, m, cs), _shaped(out64, sessions, m, cs), plan)


# ---------------------------------------------------------------- online audio front end
AUDIO_ONLINE_MAX_CHANNELS, AUDIO_ONLINE_MAX_TAIL = 8, 8192       # td_audio_online_push's limits
AUDIO_X_TYPES = {'int16': 0, 'float32': 1, 'float64': 2}          # TD_AUDIO_X_*

AudioOnlinePlan = collections.namedtuple('AudioOnlinePlan', ['frames_before', 'frames_after', 'held', 'tail_rows'])
AudioOnlinePush = collections.namedtuple('AudioOnlinePush', ['out32', 'out64', 'windows', 'plan', 'live'])


def audio_online_plan(rows_before, n, fs_in, fs_out, window, flush=False):
  """What a push of n audio rows behind `rows_before` pushed ones emits (td_audio_online_plan, host arithmetic in
  the reference's float64 order): AudioOnlinePlan(frames_before, frames_after, held, tail_rows)."""
  return AudioOnlinePlan(*_lib_values('td_audio_online_plan', (int(rows_before), int(n), float(fs_in), float(fs_out),
                                                               float(window), 1 if flush else 0), _I64 * 4))


def audio_online_state_bytes(c, tail_rows):
  """Bytes of one online audio session's state block (td_audio_online_state_bytes): two tail copies of
  [tail_rows, c] float32 squares; all zeros = a fresh session."""
  return _lib_values('td_audio_online_state_bytes', (int(c), int(tail_rows)))[0]


def audio_online_push(x, fs_in, fs_out, window, exponent, state, live, rows_before, c=None, flush=False, want32=True,
                      want64=False, windows=False, handle=None):
  """One push of a bank of online audio sessions, in one launch (td_audio_online_push).

  x [S, n, c]: int16, float32 or float64 device tensor with unit column stride (None for a flush without rows: give
  c); state: uint8 device tensor [S, >= audio_online_state_bytes()] with a row stride that is a multiple of 8 -- the
  launch reads tail copy `live` and writes the other one; rows_before: rows pushed so far.  Returns
  AudioOnlinePush(out32 [S, m, c] float32, out64 [S, m, c] float64, windows [m, 2] int64 (None when not wanted),
  plan, the copy that is live after the push: flipped when n > 0).  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  sessions = int(state.shape[0])
  n = 0 if x is None else int(x.shape[1])
  x_type = 1
  if x is not None:
    if x.dim() != 3 or int(x.shape[0]) != sessions:
      raise ValueError('audio_online_push: x of %s for %d sessions' % (tuple(x.shape), sessions))
    c = int(x.shape[2])
    name = str(x.dtype).replace('torch.', '')
    if name not in AUDIO_X_TYPES or x.device != h.device:
      raise TypeError('audio_online_push: x must be an int16, float32 or float64 tensor on %s, not %s on %s' %
                      (h.device, x.dtype, x.device))
    x_type = AUDIO_X_TYPES[name]
    if n > 0 and c > 1 and x.stride(2) != 1:
      raise ValueError('audio_online_push: the columns of x must be contiguous')
  if c is None:
    raise ValueError('audio_online_push: a flush without rows needs the channel count c')
  _check_tensors('audio_online_push', h, (('state', state, torch.uint8),), short=True)
  if not want32 and not want64:
    raise ValueError('audio_online_push: neither the float32 nor the float64 output is wanted')
  c = int(c)
  plan = audio_online_plan(rows_before, n, fs_in, fs_out, window, flush)
  m = plan.frames_after - plan.frames_before
  out32 = _spare(h, sessions * m * c, 'float32', want32)
  out64 = _spare(h, sessions * m * c, 'float64', want64)
  win = h.empty((m + 1, 2), 'int64') if windows else None       # (a spare ROW: the same reason)
  x_p, x_row, x_session = _row_block(x, n, sessions, c)
  h.check(h.lib.td_audio_online_push(
      h.ptr, sessions, x_p, x_type, x_row, x_session, n, c, int(rows_before), 1 if flush else 0,
      float(fs_in), float(fs_out), float(window), float(exponent), _ptr(state), _state_stride(state, sessions),
      int(live), _ptr(out32), _ptr(out64), c, max(m, 1) * c, _ptr(win)))
  return AudioOnlinePush(_shaped(out32, sessions, m, c), _shaped(out64, sessions, m, c),
                         win[:m] if windows else None, plan, 1 - int(live) if n > 0 else int(live))


# ---------------------------------------------------------------- online ridge fit
# td_fit_online_push's limits
ONLINE_FIT_MAX_CHANNELS, ONLINE_FIT_MAX_LAGS, ONLINE_FIT_MAX_K, ONLINE_FIT_MAX_OUTPUTS = 128, 64, 2048, 8


def online_fit_state_bytes(c, pre, post, d):
  """Bytes of one online fit session's state block (td_fit_online_state_bytes): A [(K + 1)^2] and B [(K + 1) d]
  float64, then two tail copies of {EEG [pre + post, c], target [post, d]} float32; all zeros = a fresh session."""
  return _lib_values('td_fit_online_state_bytes', (int(c), int(pre), int(post), int(d)))[0]


def _check_fit_state(who, h, state):
  """(sessions, state stride) of the fit's and the calibration's state, refused in their words unless [S, bytes]."""
  if state.dtype != _torch().uint8 or state.device != h.device or state.dim() != 2:
    raise TypeError('%s: state must be a [S, bytes] uint8 tensor on %s, not %s %s on %s' %
                    (who, h.device, tuple(state.shape), state.dtype, state.device))
  sessions = int(state.shape[0])
  return sessions, _state_stride(state, sessions)


def _moments_push(who, push, words, shape, eeg, side, widths, state, frames_before, pushes_before, flush, forget,
                  handle):
  """What online_fit_push and online_ccafit_push are: the checks of the rows beside the EEG (`side`), in their order,
  and the launch.  words: (side's argument name, what the messages call it, the same with its article, what a flush
  without rows needs); widths: (c, c2) as given, None where not; shape(c, c2): the library's shape arguments."""
  h = handle or default_handle()
  torch = _torch()
  name, noun, the_noun, needs = words
  sessions, stride = _check_fit_state(who, h, state)
  c, c2 = widths
  n = 0 if eeg is None else int(eeg.shape[1])
  if eeg is not None:
    if eeg.dim() != 3 or side is None or side.dim() != 3 or int(eeg.shape[0]) != sessions or \
        tuple(side.shape[:2]) != (sessions, n):
      raise ValueError('%s: eeg of %s and %s of %s for %d sessions' %
                       (who, tuple(eeg.shape), noun, None if side is None else tuple(side.shape), sessions))
    c, c2 = int(eeg.shape[2]), int(side.shape[2])
    _check_tensors(who, h, (('eeg', eeg, torch.float32), (name, side, torch.float32)), short=True)
    if n > 0 and (eeg.stride(2) != 1 and c > 1 or side.stride(2) != 1 and c2 > 1):
      raise ValueError('%s: the columns of eeg and %s must be contiguous' % (who, the_noun))
  if c is None or c2 is None:
    raise ValueError('%s: a flush without rows needs %s' % (who, needs))
  c, c2 = int(c), int(c2)
  h.check(getattr(h.lib, push)(
      h.ptr, sessions, *_row_block(eeg, n, sessions, c), *_row_block(side, n, sessions, c2), n, *shape(c, c2),
      int(frames_before), int(pushes_before), 1 if flush else 0, float(forget), _ptr(state), stride))
  return int(frames_before) + n


def online_fit_push(eeg, target, state, frames_before, pushes_before, pre, post, c=None, d=None, flush=False,
                    forget=1.0, handle=None):
  """One push of a bank of online fit sessions, in one launch (td_fit_online_push).

  eeg [S, n, c] and target [S, n, d]: float32 device tensors with unit column stride (None for a flush without
  rows: give c and d); state: uint8 device tensor [S, >= online_fit_state_bytes()] with a row stride that is a
  multiple of 8, updated in place; frames_before: rows pushed so far; pushes_before: pushes WITH rows so far (its
  parity says which tail copy is live).  Returns the rows pushed after the call.  Queued, not waited for."""
  return _moments_push(
      'online_fit_push', 'td_fit_online_push',
      ('target', 'target', 'target', 'the channel count c and the output count d'),
      lambda c, d: (c, int(pre), int(post), d), eeg, target, (c, d), state, frames_before, pushes_before, flush, forget,
      handle)


def online_fit_moments(state, c, pre, post, d, handle=None):
  """(xtx [S, K + 1, K + 1], xty [S, K + 1, d]) float64 device tensors: the mirrored dense moments of a bank of
  online fit sessions in the layout of LagStats.moments (td_fit_online_moments)."""
  h = handle or default_handle()
  sessions, stride = _check_fit_state('online_fit_moments', h, state)
  n1 = (int(pre) + 1 + int(post)) * int(c) + 1
  if not 1 <= n1 - 1 <= ONLINE_FIT_MAX_K:       # (the call refuses it by name; no tensor of a wild size first)
    n1 = 1
  xtx = h.empty((sessions, n1, n1), 'float64')
  xty = h.empty((sessions, n1, max(int(d), 1)), 'float64')
  h.check(h.lib.td_fit_online_moments(h.ptr, sessions, _ptr(state), stride, int(c), int(pre), int(post), int(d),
                                      _ptr(xtx), _ptr(xty)))
  return xtx, xty


def online_fit_solve(state, c, pre, post, d, frames_emitted, lambdas, handle=None):
  """Ridge weights of every (session, lambda) from a bank's moments (td_fit_online_solve): device tensors
  W [S, n_lambda, K, d] and b [S, n_lambda, d] float32.  ValueError / HotPathError (no frame emitted yet) /
  MemoryError (the dense systems over the limit) / numpy.linalg.LinAlgError (not positive definite)."""
  h = handle or default_handle()
  sessions, stride = _check_fit_state('online_fit_solve', h, state)
  lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
  k = (int(pre) + 1 + int(post)) * int(c)
  if not 1 <= k <= ONLINE_FIT_MAX_K or not 1 <= int(d) <= ONLINE_FIT_MAX_OUTPUTS:
    k = 1
  w = h.empty((sessions, len(lam), k, max(int(d), 1)), 'float32')
  b = h.empty((sessions, len(lam), max(int(d), 1)), 'float32')
  h.check(h.lib.td_fit_online_solve(h.ptr, sessions, _ptr(state), stride, int(c), int(pre), int(post), int(d),
                                    int(frames_emitted), lam_p, len(lam), _ptr(w), _ptr(b)))
  return w, b


# ---------------------------------------------------------------- online CCA fit
# td_ccafit_online_push's limits (TD_ONLINE_CCAFIT_MAX_*)
ONLINE_CCAFIT_MAX_CHANNELS, ONLINE_CCAFIT_MAX_FEATURES, ONLINE_CCAFIT_MAX_LAGS = 128, 32, 64
ONLINE_CCAFIT_MAX_K, ONLINE_CCAFIT_MAX_DIMS = 2048, 16

OnlineCcaFitSolve = collections.namedtuple('OnlineCcaFitSolve',
                                           ['rot_x', 'rot_y', 'mean_x', 'mean_y', 'e', 'corr', 'info'])


def _ccafit_views(c1, pre1, post1, c2, pre2, post2):
  """The two views as the library takes them, and (k1, k2) -- (1, 1) for a shape the call will refuse by name, so
  that no tensor of a wild size is made first."""
  views = tuple(int(v) for v in (c1, pre1, post1, c2, pre2, post2))
  k1, k2 = (views[1] + 1 + views[2]) * views[0], (views[4] + 1 + views[5]) * views[3]
  if min(views) < 0 or k1 < 1 or k2 < 1 or k1 + k2 > ONLINE_CCAFIT_MAX_K:
    k1 = k2 = 1
  return views, k1, k2


def online_ccafit_state_bytes(c1, pre1, post1, c2, pre2, post2):
  """Bytes of one online CCA fit session's state block (td_ccafit_online_state_bytes): M [(k1 + k2 + 1)^2] float64,
  then two tail copies of {EEG [pre1 + post, c1], features [pre2 + post, c2]} float32, post = max(post1, post2); all
  zeros = a fresh session."""
  return _lib_values('td_ccafit_online_state_bytes', _ccafit_views(c1, pre1, post1, c2, pre2, post2)[0])[0]


def online_ccafit_push(eeg, feat, state, frames_before, pushes_before, pre1, post1, pre2, post2, c1=None, c2=None,
                       flush=False, forget=1.0, handle=None):
  """One push of a bank of online CCA fit sessions, in one launch (td_ccafit_online_push).

  eeg [S, n, c1] and feat [S, n, c2]: float32 device tensors with unit column stride (None for a flush without
  rows: give c1 and c2); state: uint8 device tensor [S, >= online_ccafit_state_bytes()] with a row stride that is a
  multiple of 8, updated in place; frames_before: rows pushed so far; pushes_before: pushes WITH rows so far (its
  parity says which tail copy is live).  Returns the rows pushed after the call.  Queued, not waited for."""
  return _moments_push(
      'online_ccafit_push', 'td_ccafit_online_push',
      ('feat', 'features', 'the features', 'the channel count c1 and the feature count c2'),
      lambda c1, c2: (c1, int(pre1), int(post1), c2, int(pre2), int(post2)), eeg, feat, (c1, c2), state, frames_before,
      pushes_before, flush, forget, handle)


def online_ccafit_moments(state, c1, pre1, post1, c2, pre2, post2, handle=None):
  """(xtx [S, k1 + 1, k1 + 1], x2tx2 [S, k2, k2], xtx2 [S, k1, k2], sum2 [S, k2]) float64 device tensors: the mirrored
  dense moments of a bank of online CCA fit sessions in the layout of LagStats.moments, the ones row and column of
  xtx last (td_ccafit_online_moments)."""
  h = handle or default_handle()
  sessions, stride = _check_fit_state('online_ccafit_moments', h, state)
  views, k1, k2 = _ccafit_views(c1, pre1, post1, c2, pre2, post2)
  xtx = h.empty((sessions, k1 + 1, k1 + 1), 'float64')
  x2tx2 = h.empty((sessions, k2, k2), 'float64')
  xtx2 = h.empty((sessions, k1, k2), 'float64')
  sum2 = h.empty((sessions, k2), 'float64')
  h.check(h.lib.td_ccafit_online_moments(h.ptr, sessions, _ptr(state), stride, *views, _ptr(xtx), _ptr(x2tx2),
                                         _ptr(xtx2), _ptr(sum2)))
  return xtx, x2tx2, xtx2, sum2


def online_ccafit_solve(state, c1, pre1, post1, c2, pre2, post2, frames_emitted, lambdas, dim, eps_eig=1e-12,
                        handle=None):
  """The CCA model of every (session, lambda) from a bank's moments (td_ccafit_online_solve):
  OnlineCcaFitSolve(rot_x [S, n_lambda, k1, dim], rot_y [S, n_lambda, k2, dim], mean_x [S, k1], mean_y [S, k2],
  e [S, n_lambda, dim] float32 device tensors, corr [S, n_lambda, 3, dim] float64 {mean_a, mean_b, power} of the
  fitted stretch, info [S, n_lambda, 4] host int32 as cca_solve's).  ValueError / HotPathError (fewer than 2 frames
  counted)."""
  h = handle or default_handle()
  sessions, stride = _check_fit_state('online_ccafit_solve', h, state)
  lam, lam_p = _lib.f64_array(np.atleast_1d(lambdas))
  views, k1, k2 = _ccafit_views(c1, pre1, post1, c2, pre2, post2)
  dims = int(dim) if 1 <= int(dim) <= ONLINE_CCAFIT_MAX_DIMS else 1
  nl = max(len(lam), 1)
  rot_x = h.empty((sessions, nl, k1, dims), 'float32')
  rot_y = h.empty((sessions, nl, k2, dims), 'float32')
  mean_x = h.empty((sessions, k1), 'float32')
  mean_y = h.empty((sessions, k2), 'float32')
  e = h.empty((sessions, nl, dims), 'float32')
  corr = h.empty((sessions, nl, 3, dims), 'float64')
  info = np.zeros((sessions, nl, 4), np.int32)
  h.check(h.lib.td_ccafit_online_solve(
      h.ptr, sessions, _ptr(state), stride, *views, int(frames_emitted), lam_p, len(lam), int(dim), float(eps_eig),
      _ptr(rot_x), _ptr(rot_y), _ptr(mean_x), _ptr(mean_y), _ptr(e), _ptr(corr),
      info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
  return OnlineCcaFitSolve(rot_x, rot_y, mean_x, mean_y, e, corr, info)


# ---------------------------------------------------------------- online calibration
# td_calib_online_push's limits, the number of float64 sums in a state block, td_calib_online_finish's statuses
ONLINE_CALIB_MAX_CHANNELS, ONLINE_CALIB_MAX_LAGS, ONLINE_CALIB_SUMS = 128, 64, 29
CALIB_OK, CALIB_NO_WINDOW, CALIB_NO_POWER, CALIB_SAME_MEANS = 0, 1, 2, 3

OnlineCalibFinish = collections.namedtuple('OnlineCalibFinish', ['corr', 'lda', 'dprime', 'status'])


def online_calib_state_bytes(c, pre, post):
  """Bytes of one online calibration session's state block (td_calib_online_state_bytes): ONLINE_CALIB_SUMS float64
  sums, then the EEG tail [pre + post, c] and the envelope tail [post, 2] float32; all zeros = a fresh session."""
  return _lib_values('td_calib_online_state_bytes', (int(c), int(pre), int(post)))[0]


def online_calib_push(eeg, env, w, b, state, frames_before, pre, post, width, c=None, flush=False, handle=None):
  """One push of a bank of online calibration sessions, in one launch (td_calib_online_push).

  eeg [S, n, c] and env [S, n, 2] (attended, unattended): float32 device tensors with unit column stride (None for a
  flush without rows: give c); w [S or 1, (pre + 1 + post) c] and b [S or 1] float32 (one row: the model every
  session shares) -- read where they are at every push; state: uint8 device tensor [S, >=
  online_calib_state_bytes()] with a row stride that is a multiple of 8, updated in place; frames_before: rows
  pushed so far; width: the window of the LDA's training data.  Returns the rows pushed after the call.  Queued,
  not waited for."""
  h = handle or default_handle()
  torch = _torch()
  sessions, stride = _check_fit_state('online_calib_push', h, state)
  n = 0 if eeg is None else int(eeg.shape[1])
  if eeg is not None:
    if eeg.dim() != 3 or env is None or env.dim() != 3 or int(eeg.shape[0]) != sessions or \
        tuple(env.shape) != (sessions, n, 2):
      raise ValueError('online_calib_push: eeg of %s and env of %s for %d sessions' %
                       (tuple(eeg.shape), None if env is None else tuple(env.shape), sessions))
    c = int(eeg.shape[2])
  if c is None:
    raise ValueError('online_calib_push: a flush without rows needs the channel count c')
  c = int(c)
  _check_tensors('online_calib_push', h, (('eeg', eeg, torch.float32), ('env', env, torch.float32),
                                          ('w', w, torch.float32), ('b', b, torch.float32)), short=True)
  if n > 0 and (eeg.stride(2) != 1 and c > 1 or env.stride(2) != 1):
    raise ValueError('online_calib_push: the columns of eeg and env must be contiguous')
  if w.dim() != 2 or int(w.shape[0]) not in (1, sessions) or int(b.numel()) != int(w.shape[0]):
    raise ValueError('online_calib_push: %s weights and %d biases for %d sessions' %
                     (tuple(w.shape), int(b.numel()), sessions))
  k = int(w.shape[1])
  if k != (int(pre) + 1 + int(post)) * c:
    raise ValueError('online_calib_push: %d weights for %d lags of %d channels' % (k, int(pre) + 1 + int(post), c))
  w, b = w.contiguous(), b.reshape(-1).contiguous()
  shared = int(w.shape[0]) == 1
  h.check(h.lib.td_calib_online_push(
      h.ptr, sessions, *_row_block(eeg, n, sessions, c), *_row_block(env, n, sessions, 2),
      _ptr(w), 0 if shared else k, _ptr(b), 0 if shared else 1,
      n, int(frames_before), c, int(pre), int(post), int(width), 1 if flush else 0, _ptr(state), stride))
  return int(frames_before) + n


def _calib_sums(who, sums, count, dims, state, handle):
  """What online_calib_sums and online_ccacalib_sums are: [S, count] float64 from the library's `sums`, which takes
  `dims` (nothing, or the CCA model's columns) behind the state."""
  h = handle or default_handle()
  sessions, stride = _check_fit_state(who, h, state)
  out = h.empty((sessions, count), 'float64')
  h.check(getattr(h.lib, sums)(h.ptr, sessions, _ptr(state), stride, *dims, _ptr(out)))
  return out


def _calib_finish(who, finish, corr_shape, lda_width, dims, state, frames_emitted, width, handle):
  """What online_calib_finish and online_ccacalib_finish are: the four outputs and the library's `finish`, which
  takes `dims` (nothing, or the CCA model's columns) behind the state."""
  h = handle or default_handle()
  sessions, stride = _check_fit_state(who, h, state)
  corr = h.empty((sessions,) + corr_shape, 'float64')
  lda = h.empty((sessions, lda_width), 'float64')
  dprime = h.empty((sessions,), 'float64')
  status = h.empty((sessions,), 'int32')
  h.check(getattr(h.lib, finish)(h.ptr, sessions, _ptr(state), stride, *dims, int(frames_emitted), int(width),
                                 _ptr(corr), _ptr(lda), _ptr(dprime), _ptr(status)))
  return OnlineCalibFinish(corr, lda, dprime, status)


def online_calib_sums(state, handle=None):
  """The float64 sums of a bank of online calibration sessions, [S, ONLINE_CALIB_SUMS] on the device, in
  td_calib_online_sums' order: sum p, p^2, a, a^2, u, u^2 | class 0: sum z [3], upper sum z z^T [6] | class 1 | the
  open window's sum p, a, a p, u, u p."""
  return _calib_sums('online_calib_sums', 'td_calib_online_sums', ONLINE_CALIB_SUMS, (), state, handle)


def online_calib_finish(state, frames_emitted, width, handle=None):
  """The closed form of Decoder.train on a bank's sums, in one launch (td_calib_online_finish):
  OnlineCalibFinish(corr [S, 2, 3] float64, lda [S, 3] float64 {1, slope, intercept}, dprime [S] float64, status [S]
  int32 -- CALIB_OK, CALIB_NO_WINDOW, CALIB_NO_POWER, CALIB_SAME_MEANS), device tensors.  The state is not modified.
  Queued, not waited for."""
  return _calib_finish('online_calib_finish', 'td_calib_online_finish', (2, 3), 3, (), state, frames_emitted, width,
                       handle)


# ---------------------------------------------------------------- online calibration of a CCA model
CALIB_NOT_POSITIVE = 4                     # TD_CALIB_NOT_POSITIVE: td_ccacalib_online_finish's fifth status


def online_ccacalib_sums_count(dims):
  """T(dims) = 9 dims^2 + 20 dims: the float64 sums at the head of an online CCA calibration session's state."""
  return 9 * int(dims) * int(dims) + 20 * int(dims)


def online_ccacalib_state_bytes(c1, pre1, post1, c2, pre2, post2, dims):
  """Bytes of one online CCA calibration session's state block (td_ccacalib_online_state_bytes):
  online_ccacalib_sums_count(dims) float64 sums, then the EEG tail [pre1 + post, c1] and the feature tails
  [2, pre2 + post, c2] float32, post = max(post1, post2); all zeros = a fresh session."""
  return _lib_values('td_ccacalib_online_state_bytes', (int(c1), int(pre1), int(post1), int(c2), int(pre2),
                                                        int(post2), int(dims)))[0]


def online_ccacalib_lds_bytes(c1, pre1, post1, c2, pre2, post2, dims, emitted=64):
  """(frames per pass, LDS bytes) of a td_ccacalib_online_push launch that emits `emitted` frames
  (td_ccacalib_online_lds_bytes); ValueError with the byte budget for a shape that does not fit at a pass of one."""
  return tuple(_lib_values('td_ccacalib_online_lds_bytes', (int(c1), int(pre1), int(post1), int(c2), int(pre2),
                                                            int(post2), int(dims), int(emitted)), _I32_I64))


def online_ccacalib_push(eeg, attended, unattended, mean_x, rot_x, mean_y, rot_y, state, frames_before, pre1, post1,
                         pre2, post2, width, flush=False, handle=None):
  """One push of a bank of online CCA calibration sessions, in one launch (td_ccacalib_online_push).

  eeg [S, n, c1], attended and unattended [S, n, c2]: float32 device tensors with unit column stride (None for a
  flush without rows; the two feature tensors share their strides); mean_x [M, k1], rot_x [M, k1, dims], mean_y
  [M, k2], rot_y [M, k2, dims] float32 with M = S or 1 (one model for every session) -- read where they are at every
  push; state: uint8 device tensor [S, >= online_ccacalib_state_bytes()] with a row stride that is a multiple of 8,
  updated in place; frames_before: rows pushed so far; width: the window of the LDA's training data.  Returns the
  rows pushed after the call.  Queued, not waited for."""
  h = handle or default_handle()
  torch = _torch()
  who = 'online_ccacalib_push'
  sessions, stride = _check_fit_state(who, h, state)
  pre1, post1, pre2, post2 = int(pre1), int(post1), int(pre2), int(post2)
  nl1, nl2 = pre1 + 1 + post1, pre2 + 1 + post2
  if rot_x.dim() != 3 or rot_y.dim() != 3 or mean_x.dim() != 2 or mean_y.dim() != 2:
    raise ValueError('%s: the means are [M, k] and the rotations [M, k, dims]' % who)
  models, k1, dims = (int(v) for v in rot_x.shape)
  k2 = int(rot_y.shape[1])
  if (nl1 < 1 or nl2 < 1 or k1 % nl1 or k2 % nl2 or tuple(rot_y.shape) != (models, k2, dims) or
      tuple(mean_x.shape) != (models, k1) or tuple(mean_y.shape) != (models, k2) or models not in (1, sessions)):
    raise ValueError('%s: rotations of %s and %s with means of %s and %s for %d + %d lags and %d sessions' %
                     (who, tuple(rot_x.shape), tuple(rot_y.shape), tuple(mean_x.shape), tuple(mean_y.shape), nl1, nl2,
                      sessions))
  c1, c2 = k1 // nl1, k2 // nl2
  n = 0 if eeg is None else int(eeg.shape[1])
  if eeg is not None and (tuple(eeg.shape) != (sessions, n, c1) or attended is None or unattended is None or
                          tuple(attended.shape) != (sessions, n, c2) or tuple(unattended.shape) != (sessions, n, c2)):
    raise ValueError('%s: eeg of %s and features of %s and %s for %d sessions of %d channels and %d features' %
                     (who, tuple(eeg.shape), None if attended is None else tuple(attended.shape),
                      None if unattended is None else tuple(unattended.shape), sessions, c1, c2))
  _check_tensors(who, h, (
      ('eeg', eeg, torch.float32), ('attended', attended, torch.float32), ('unattended', unattended, torch.float32),
      ('mean_x', mean_x, torch.float32), ('rot_x', rot_x, torch.float32), ('mean_y', mean_y, torch.float32),
      ('rot_y', rot_y, torch.float32)), short=True)
  if n > 0:
    if (c1 > 1 and eeg.stride(2) != 1) or (c2 > 1 and (attended.stride(2) != 1 or unattended.stride(2) != 1)):
      raise ValueError('%s: the columns of eeg and the features must be contiguous' % who)
    if unattended.stride() != attended.stride():      # (one pair of strides serves both classes)
      attended, unattended = attended.contiguous(), unattended.contiguous()
  mean_x, rot_x, mean_y, rot_y = (t.contiguous() for t in (mean_x, rot_x, mean_y, rot_y))
  att_p, feat_row, feat_session = _row_block(attended, n, sessions, c2)
  h.check(h.lib.td_ccacalib_online_push(
      h.ptr, sessions, *_row_block(eeg, n, sessions, c1), att_p, _ptr(unattended if n > 0 else None), feat_row,
      feat_session, n, c1, pre1, post1, c2, pre2, post2, dims, _ptr(mean_x), _ptr(rot_x), _ptr(mean_y), _ptr(rot_y),
      0 if models == 1 else 1, int(width), int(frames_before), 1 if flush else 0, _ptr(state), stride))
  return int(frames_before) + n


def online_ccacalib_sums(state, dims, handle=None):
  """The float64 sums of a bank of online CCA calibration sessions, [S, online_ccacalib_sums_count(dims)] on the
  device, in td_ccacalib_online_sums' order: sum a, a^2, b1, b1^2, b0, b0^2 [dims each] | class 0: sum z [3 dims],
  upper sum z z^T | class 1 | the open window's sum a, b1, a b1, b0, a b0 [dims each]."""
  count = online_ccacalib_sums_count(dims) if 1 <= int(dims) <= CCA_ONLINE_MAX_DIMS else 1   # (refused by name)
  return _calib_sums('online_ccacalib_sums', 'td_ccacalib_online_sums', count, (int(dims),), state, handle)


def online_ccacalib_finish(state, dims, frames_emitted, width, handle=None):
  """The closed form of Decoder.train on a CCA bank's sums, in one launch (td_ccacalib_online_finish):
  OnlineCalibFinish(corr [S, 2, 3, dims] float64, lda [S, dims + 2] float64 {w, slope, intercept}, dprime [S] float64,
  status [S] int32 -- CALIB_OK, CALIB_NO_WINDOW, CALIB_NO_POWER, CALIB_SAME_MEANS, CALIB_NOT_POSITIVE), device
  tensors.  The state is not modified.  Queued, not waited for."""
  d = int(dims) if 1 <= int(dims) <= CCA_ONLINE_MAX_DIMS else 1                               # (refused by name)
  return _calib_finish('online_ccacalib_finish', 'td_ccacalib_online_finish', (2, 3, d), d + 2, (int(dims),), state,
                       frames_emitted, width, handle)


# ---------------------------------------------------------------- online calibration of a DNN decoder
def online_dnn_calib_state_bytes(c, pre, post):
  """Bytes of one online DNN calibration session's state block (td_fccalib_online_state_bytes):
  online_calib_state_bytes', byte for byte -- online_calib_sums and online_calib_finish serve the state as they are."""
  return _lib_values('td_fccalib_online_state_bytes', (int(c), int(pre), int(post)))[0]


def online_dnn_calib_lds_bytes(c, pre, post, hidden, emitted=64):
  """(frames per pass, LDS bytes) of a td_fccalib_online_push launch that emits `emitted` frames
  (td_fccalib_online_lds_bytes); ValueError for a shape outside the limits or over the byte budget."""
  hid, hid_p = _i32_array(list(hidden) or [0])
  return tuple(_lib_values('td_fccalib_online_lds_bytes', (int(c), int(pre), int(post), len(hidden), hid_p,
                                                           int(emitted)), _I32_I64))


def online_dnn_calib_push(eeg, env, params, hidden, state, frames_before, pre, post, width, flush=False, handle=None):
  """One push of a bank of online DNN calibration sessions, in one launch (td_fccalib_online_push).

  eeg [S, n, c] and env [S, n, 2] (attended, unattended): float32 device tensors with unit column stride (None for a
  flush without rows); params [S or 1, P] float32: the packed parameters of td_mlp_* ([W1, b1, W2, b2, ...], one
  output) of a network with the hidden layers `hidden` on c (pre + 1 + post) inputs -- one row: the model every
  session shares; read where they are at every push; state: uint8 device tensor [S, >=
  online_dnn_calib_state_bytes()] with a row stride that is a multiple of 8, updated in place; frames_before: rows
  pushed so far; width: the window of the LDA's training data.  Returns the rows pushed after the call.  Queued, not
  waited for."""
  h = handle or default_handle()
  torch = _torch()
  who = 'online_dnn_calib_push'
  sessions, stride = _check_fit_state(who, h, state)
  hidden = [int(v) for v in hidden]
  nl = int(pre) + 1 + int(post)
  if params.dim() != 2 or int(params.shape[0]) not in (1, sessions):
    raise ValueError('%s: params of %s for %d sessions ([S or 1, P])' % (who, tuple(params.shape), sessions))
  # P = k h1 + the rest: k from the parameter count (as dnn_online_push)
  first = hidden[0] if hidden else 1
  count = int(params.shape[1])
  k = (count - dnn_param_count(0, hidden)) // first if first > 0 else 0
  if nl < 1 or k < 1 or k % nl or dnn_param_count(k, hidden) != count:
    raise ValueError('%s: %d parameters for hidden layers %s on %d lags' % (who, count, hidden, nl))
  c = k // nl
  n = 0 if eeg is None else int(eeg.shape[1])
  if eeg is not None and (tuple(eeg.shape) != (sessions, n, c) or env is None or
                          tuple(env.shape) != (sessions, n, 2)):
    raise ValueError('%s: eeg of %s and env of %s for %d sessions of %d channels' %
                     (who, tuple(eeg.shape), None if env is None else tuple(env.shape), sessions, c))
  _check_tensors(who, h, (('eeg', eeg, torch.float32), ('env', env, torch.float32),
                          ('params', params, torch.float32)), short=True)
  if n > 0 and (eeg.stride(2) != 1 and c > 1 or env.stride(2) != 1):
    raise ValueError('%s: the columns of eeg and env must be contiguous' % who)
  if params.stride(1) != 1 and count > 1:
    params = params.contiguous()
  shared = int(params.shape[0]) == 1
  hid, hid_p = _i32_array(hidden or [0])
  h.check(h.lib.td_fccalib_online_push(
      h.ptr, sessions, *_row_block(eeg, n, sessions, c), *_row_block(env, n, sessions, 2), n, int(frames_before), c,
      int(pre), int(post), hid_p, len(hidden), _ptr(params), 0 if shared else int(params.stride(0)), int(width),
      1 if flush else 0, _ptr(state), stride))
  return int(frames_before) + n


# ---------------------------------------------------------------- fully connected regressor / match-mismatch classifier
MLP_LOSSES = {'mse': 0, 'pearson': 1}


def _mlp_loss(loss):
  if loss not in MLP_LOSSES:
    raise ValueError('loss %r: one of %s' % (loss, sorted(MLP_LOSSES)))
  return MLP_LOSSES[loss]


def _check_x2(x, x2):
  if int(x2.shape[0]) != int(x.shape[0]):
    raise ValueError('x2 has %d rows, x %d: both inputs cover the same files' % (int(x2.shape[0]), int(x.shape[0])))


def _mlp_views(h, x, x2, context, file_offsets, input_offset, hidden):
  """What every td_mlp_* (x2 None) / td_mlpc_* prototype begins with, as ctypes arguments: (the handle through
  input_offset, [hidden_host, num_hidden], the host arrays those point into -- file offsets first -- which the
  caller keeps alive over the call).  context = (pre, post) or (pre, post, pre2, post2)."""
  offs, offs_p = _lib.i64_array(file_offsets)
  hid, hid_p = _i32_array(list(hidden) or [0])
  ptrs, sizes = [_ptr(x), x.stride(0)], [int(x.shape[1]), int(context[0]), int(context[1])]
  if x2 is not None:
    ptrs += [_ptr(x2), x2.stride(0)]
    sizes += [int(x2.shape[1]), int(context[2]), int(context[3])]
  return [h.ptr] + ptrs + [offs_p, len(offs) - 1] + sizes + [int(input_offset)], [hid_p, len(hidden)], [offs, hid]


def _mlp_fit(h, x, x2, y, context, file_offsets, input_offset, hidden, rows_used, batch_rows, nstat, epochs=None):
  """A train (epochs given) or grad call: (its arguments through batch_rows, the stats buffer -- [epochs, steps,
  nstat] or [nstat] float64 -- and the host arrays to keep alive over the call)."""
  head, net, keep = _mlp_views(h, x, x2, context, file_offsets, input_offset, hidden)
  used_p = None
  if rows_used is None:
    n = int(np.sum(np.maximum(np.diff(keep[0]) - abs(int(input_offset)), 0)))
  else:
    used, used_p = _lib.i64_array(rows_used)
    keep.append(used)
    n = int(np.sum(used))
  shape = (nstat,)
  if epochs is not None:
    shape = (max(int(epochs), 0), -(-n // int(batch_rows)) if batch_rows > 0 else 0, nstat)
  args = head + [used_p, _ptr(y), y.stride(0), int(y.shape[1])] + net + [int(batch_rows)]
  return args, h.empty(shape, 'float64'), keep


def _mlp_forward(h, fn, x, x2, context, file_offsets, input_offset, hidden, d, params):
  head, net, keep = _mlp_views(h, x, x2, context, file_offsets, input_offset, hidden)
  out = h.empty((int(x.shape[0]), int(d)), 'float32')
  h.check(fn(*head, int(d), *net, _ptr(params), _ptr(out), out.stride(0)))
  return out


def mlp_train(x, y, file_offsets, pre, post, hidden, params, state, batch_rows, epochs, lr, rho, eps,
              input_offset=0, rows_used=None, shuffle_seed=None, handle=None, loss='mse'):
  """`epochs` epochs of minibatch RMSprop on the lagged view of x (td_mlp_train): params / state are the packed
  float32 parameters and RMSprop accumulators (device, updated in place).  Returns the device float64 sums
  [epochs, steps, 6] of every step's forward pass (sum p, y, p^2, y^2, p y of output 0; sum (p - y)^2).
  loss='pearson' minimises the Pearson correlation loss instead (td_mlp_train_loss) and returns
  [epochs, steps, 7]: the six sums, then the step's loss -(1 / B) sum_o r_o."""
  h = handle or default_handle()
  code = _mlp_loss(loss)
  args, stats, keep = _mlp_fit(h, x, None, y, (pre, post), file_offsets, input_offset, hidden, rows_used, batch_rows,
                               7 if code else 6, epochs)
  args += [int(epochs), _ptr(params), _ptr(state), float(lr), float(rho), float(eps),
           -1 if shuffle_seed is None else int(shuffle_seed), _ptr(stats)]
  h.check(h.lib.td_mlp_train_loss(*args, code) if code else h.lib.td_mlp_train(*args))
  return stats


def mlp_grad(x, y, file_offsets, pre, post, hidden, params, batch_rows, batch_index, input_offset=0,
             rows_used=None, handle=None, loss='mse'):
  """(gradient [P] float32, sums [6] float64) of minibatch `batch_index` at params, no update (td_mlp_grad).
  loss='pearson': the gradient of the Pearson correlation loss and sums [7], the last one the loss
  (td_mlp_grad_loss)."""
  h = handle or default_handle()
  code = _mlp_loss(loss)
  args, stats, keep = _mlp_fit(h, x, None, y, (pre, post), file_offsets, input_offset, hidden, rows_used, batch_rows,
                               7 if code else 6)
  grad = h.empty((int(params.numel()),), 'float32')
  args += [int(batch_index), _ptr(params), _ptr(grad), _ptr(stats)]
  h.check(h.lib.td_mlp_grad_loss(*args, code) if code else h.lib.td_mlp_grad(*args))
  return grad, stats


def mlp_forward(x, file_offsets, pre, post, hidden, d, params, input_offset=0, handle=None):
  """The network on every row of x (td_mlp_forward): [rows, d]; row file_offsets[f] + t = frame t of file f."""
  h = handle or default_handle()
  return _mlp_forward(h, h.lib.td_mlp_forward, x, None, (pre, post), file_offsets, input_offset, hidden, d, params)


def mlpc_train(x, x2, y, file_offsets, pre, post, pre2, post2, hidden, params, state, batch_rows, epochs,
               lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, step0=0, update=True, input_offset=0, rows_used=None,
               shuffle_seed=None, handle=None):
  """`epochs` epochs of minibatch Adam on the binary cross-entropy of the sigmoid network over
  [lagged x | lagged x2] (td_mlpc_train): params [P] and state [2 P] (Adam's m, then v) are updated in place;
  `step0` = the updates already applied.  update=False runs the forward passes only (state may be None).
  Returns the device float64 sums [epochs, steps, 6] of every step's forward pass: slot 0 = the correct
  entries at threshold 0.5, slot 5 = the sum of the entry losses."""
  h = handle or default_handle()
  _check_x2(x, x2)
  args, stats, keep = _mlp_fit(h, x, x2, y, (pre, post, pre2, post2), file_offsets, input_offset, hidden, rows_used,
                               batch_rows, 6, epochs)
  h.check(h.lib.td_mlpc_train(*args, int(epochs), _ptr(params), _ptr(state), float(lr), float(beta1), float(beta2),
                              float(eps), int(step0), 1 if update else 0,
                              -1 if shuffle_seed is None else int(shuffle_seed), _ptr(stats)))
  return stats


def mlpc_grad(x, x2, y, file_offsets, pre, post, pre2, post2, hidden, params, batch_rows, batch_index,
              input_offset=0, rows_used=None, handle=None):
  """(gradient [P] float32, sums [6] float64) of minibatch `batch_index` at params, no update (td_mlpc_grad)."""
  h = handle or default_handle()
  _check_x2(x, x2)
  args, stats, keep = _mlp_fit(h, x, x2, y, (pre, post, pre2, post2), file_offsets, input_offset, hidden, rows_used,
                               batch_rows, 6)
  grad = h.empty((int(params.numel()),), 'float32')
  h.check(h.lib.td_mlpc_grad(*args, int(batch_index), _ptr(params), _ptr(grad), _ptr(stats)))
  return grad, stats


def mlpc_forward(x, x2, file_offsets, pre, post, pre2, post2, hidden, d, params, input_offset=0, handle=None):
  """The classifier's probabilities on every row of (x, x2) (td_mlpc_forward): [rows, d]; row
  file_offsets[f] + t = frame t of file f."""
  h = handle or default_handle()
  _check_x2(x, x2)
  return _mlp_forward(h, h.lib.td_mlpc_forward, x, x2, (pre, post, pre2, post2), file_offsets, input_offset, hidden,
                      d, params)


# td_dnn_train_many: models per call (TD_DNN_MANY_MAX_MODELS of include/td_hotpath.h); dnn_train_many splits a longer
# list into calls of this many.  A module attribute so that a test can lower it.
DNN_MANY_MAX_MODELS = 64


def _train_many(who, fn, h, x, x2, y, context, file_offsets, input_offset, hidden, params, per_model, rows_used,
                shuffle_seeds, batch_rows, epochs, mode, nstat, settings):
  """What dnn_train_many and clf_train_many share: the per-model lists checked against len(params), then one call of
  h.lib.<fn> (looked up here, at call time) per DNN_MANY_MAX_MODELS models -- the shared arguments, `mode` (the
  loss or the update flag), the chunk's rows_used and parameter pointers, settings(m0, m1) (the family's own
  arguments of models m0 .. m1: state pointers and optimizer arrays, as ctypes objects that own their memory), its seeds and its zeroed stats buffer
  [models, epochs, most steps, nstat] -- and every model's [epochs, its steps, nstat] slice of it."""
  n_models, epochs, batch_rows = len(params), int(epochs), int(batch_rows)
  seeds = [None] * n_models if shuffle_seeds is None else list(shuffle_seeds)
  used_all = np.ascontiguousarray(rows_used, dtype=np.int64).reshape(n_models, -1)
  if any(v is None or len(v) != n_models for v in [seeds] + list(per_model)):
    raise ValueError('%s: %d models, but a per-model argument of another length' % (who, n_models))
  head, net, keep = _mlp_views(h, x, x2, context, file_offsets, input_offset, hidden)
  if used_all.shape[1] != len(keep[0]) - 1:
    raise ValueError('%s: rows_used has %d files, the recordings %d' % (who, used_all.shape[1], len(keep[0]) - 1))
  out = []
  cap = max(1, int(DNN_MANY_MAX_MODELS))
  for m0 in range(0, n_models, cap):
    m1 = min(m0 + cap, n_models)
    n = m1 - m0
    used, used_p = _lib.i64_array(used_all[m0:m1])
    steps = [-(-int(u.sum()) // batch_rows) if batch_rows > 0 else 0 for u in used]
    stats = h.zeros((n, max(epochs, 0), max(steps + [0]), nstat), 'float64')
    seed, seed_p = _lib.i64_array([-1 if s is None else int(s) for s in seeds[m0:m1]])
    h.check(getattr(h.lib, fn)(*head, _ptr(y), y.stride(0), int(y.shape[1]), *net, batch_rows, epochs, mode, n, used_p,
                               _device_pointers(params[m0:m1]), *settings(m0, m1), seed_p, _ptr(stats)))
    out += [stats[i, :, :steps[i]] for i in range(n)]
  return out


def _device_pointers(tensors):
  return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _c_array(ctype, values):
  return (ctype * len(values))(*[float(v) for v in values])


def dnn_train_many(x, y, file_offsets, pre, post, hidden, params, states, batch_rows, epochs, lrs, rhos, epss,
                   rows_used, input_offset=0, shuffle_seeds=None, handle=None, loss='mse'):
  """mlp_train for many regressors of one architecture at once (td_dnn_train_many): params[m] / states[m] are model
  m's packed float32 parameters and RMSprop accumulators (device, updated in place), lrs / rhos / epss / shuffle_seeds
  (None: in order) its settings, rows_used[m][f] the rows of file f in its stream (0: a file it does not train on).
  Returns one device float64 tensor per model, [epochs, its steps, 6 or 7] as mlp_train returns it.  More than
  DNN_MANY_MAX_MODELS models go through several calls."""
  h = handle or default_handle()
  code = _mlp_loss(loss)

  def settings(m0, m1):
    return [_device_pointers(states[m0:m1])] + [_c_array(ctypes.c_float, v[m0:m1]) for v in (lrs, rhos, epss)]
  return _train_many('dnn_train_many', 'td_dnn_train_many', h, x, None, y, (pre, post), file_offsets, input_offset,
                     hidden, params, [states, lrs, rhos, epss], rows_used, shuffle_seeds, batch_rows, epochs, code,
                     7 if code else 6, settings)


def clf_train_many(x, x2, y, file_offsets, pre, post, pre2, post2, hidden, params, states, batch_rows, epochs,
                   rows_used, lrs=None, beta1s=None, beta2s=None, epss=None, step0s=None, update=True,
                   input_offset=0, shuffle_seeds=None, handle=None):
  """mlpc_train for many classifiers of one architecture at once (td_clf_train_many): params[m] / states[m] are
  model m's packed float32 parameters and Adam state [2 P] (device, updated in place), lrs / beta1s / beta2s / epss /
  step0s / shuffle_seeds (None: in order) its settings, rows_used[m][f] the rows of file f in its stream.
  update=False scores instead: one pass in order with nothing written; states and the settings may be None.
  Returns one device float64 tensor per model, [epochs, its steps, 6] as mlpc_train returns it.  More than
  DNN_MANY_MAX_MODELS models go through several calls."""
  h = handle or default_handle()
  _check_x2(x, x2)

  def settings(m0, m1):
    if not update:
      return [None] * 6                                      # scoring reads none of them
    return ([_device_pointers(states[m0:m1])] +
            [_c_array(ctypes.c_double, v[m0:m1]) for v in (lrs, beta1s, beta2s, epss)] +
            [(ctypes.c_int64 * (m1 - m0))(*[int(v) for v in step0s[m0:m1]])])
  return _train_many('clf_train_many', 'td_clf_train_many', h, x, x2, y, (pre, post, pre2, post2), file_offsets,
                     input_offset, hidden, params, [states, lrs, beta1s, beta2s, epss, step0s] if update else [],
                     rows_used, shuffle_seeds, batch_rows, epochs, 1 if update else 0, 6, settings)
