"""GPU sweep of the one-launch conjugate-gradient ridge solvers (csrc/cg.hip) over every kernel instance and edge:
cg_resident_kernel<R = 1..8> and cg_toeplitz_kernel<kCpw = 1, 2> at the cases of tests/cg_edges.py, each against
np.linalg.solve in float64 of the system built from the device's own float64 moments, within the derived bound of
cg_edges (in effect one float32 rounding of the output).  Handle.last_cg_plan() proves which instance ran and on how
many workgroups; the refused shapes must give the factorisation's answer bit for bit with no conjugate-gradient
launch at all."""
import ctypes

import numpy as np
import pytest

from tests import cg_edges as ce
from tests import parity_log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


@pytest.fixture(scope='module')
def handles(dev):
  """where -> (handle, stream or None): the default handle, ONE handle of the module's own whose declared CU count
  (td_set_cu_count) is set per case, and a really masked stream per CU count; the masked streams go at teardown."""
  import torch
  made = {}

  def get(where):
    if where[0] == 'default':
      return dev.default_handle(), None
    if where[0] == 'declared':
      if 'declared' not in made:
        made['declared'] = (dev.Handle(), None, None)
      h = made['declared'][0]
      h.check(h.lib.td_set_cu_count(h.ptr, ctypes.c_int(where[1])))
      return h, None
    if where not in made:
      made[where] = ce.masked_handle(dev, where[1])
    return made[where][0], made[where][1]
  yield get
  torch.cuda.synchronize()
  while made:
    _, (h, stream, keep) = made.popitem()
    if keep is not None:
      # The handle goes back to its own stream BEFORE the masked one is destroyed: the traceback of a failed case
      # keeps its handle and statistics alive past this teardown, and td_destroy / td_stats_destroy queue on and wait
      # for the handle's stream -- a destroyed one crashed the interpreter at exit.
      lib, p = keep
      h.check(lib.td_use_own_stream(h.ptr))
      lib.td_stream_destroy(p)
    del h


def _accumulate(dev, h, case):
  eeg, env, offs = ce.make_data(case)
  st = dev.LagStats(case.c, 0, case.post, d=case.d, handle=h)
  st.accumulate(h.to_device(eeg), None, h.to_device(env), offs, handle=h)
  return st


def _reference(st, case):
  m = st.moments()
  frames, files = st.counts()
  assert frames == case.files * case.frames and files == case.files
  return ce.reference(m['xtx'].cpu().numpy(), m['xty'].cpu().numpy(), frames, case.lams, ce.case_accept(case))


def _check(case, name, w, b, ref, plan, iterations):
  dw, db, ratio = ce.distance(w, b, ref)
  bw, bb = ce.bounds(ref)
  print('%s: |w - ref| %.3e  |b - ref| %.3e  distance / bound %.3f  cond %.2f  iterations %d' %
        (name, dw, db, ratio, ref.cond.max(), iterations))
  parity_log.record('cg_edges ' + name, kernel=plan['kernel'], rows=plan['rows'],
                    channels_per_workgroup=plan['channels_per_workgroup'], workgroups=plan['workgroups'],
                    w_vs_ref64=dw, b_vs_ref64=db, largest_bound=float(max(bw.max(), bb.max())),
                    distance_over_bound=ratio, cond=float(ref.cond.max()), iterations=iterations)
  assert np.all(np.abs(w.astype(np.float64) - ref.w) <= bw), (dw, ratio)
  assert np.all(np.abs(b.astype(np.float64) - ref.b) <= bb), (db, ratio)


@pytest.mark.parametrize('case', ce.RESIDENT_CASES, ids=ce.case_id)
def test_resident_kernel_instance_against_float64(dev, handles, case):
  h, _ = handles(('default',) if case.declared is None else ('declared', case.declared))
  st = _accumulate(dev, h, case)
  ref = _reference(st, case)
  h.set_solver('cg')
  try:
    w, b = (t.cpu().numpy() for t in st.ridge_solve(list(case.lams), handle=h))
    info, plan = h.last_solve_info(), h.last_cg_plan()
  finally:
    h.set_solver('auto')
  assert info['solver'] == 'cg' and info['cg_status'] == 0 and 0 < info['iterations'], info
  assert plan == {'kernel': 'resident', 'rows': case.rows, 'channels_per_workgroup': 0,
                  'workgroups': case.workgroups}, plan
  _check(case, ce.case_id(case), w, b, ref, plan, info['iterations'])


@pytest.mark.parametrize('case', ce.COMPACT_CASES, ids=ce.case_id)
def test_compact_kernel_instance_against_float64(dev, handles, case):
  import contextlib
  import torch
  h, stream = handles(case.where)
  with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
    st = _accumulate(dev, h, case)
    ref = _reference(st, case)
    if case.use_async:
      h.set_option('async_cg', 1)
      try:
        w, b, flag = st.ridge_solve_async(list(case.lams), handle=h)
        h.synchronize()
        assert flag() == 0
        info, plan = h.last_solve_info(), h.last_cg_plan()
      finally:
        h.set_option('async_cg', 0)
      assert info['solver'] == 'cg', info
    else:
      w, b = st.ridge_solve(list(case.lams), handle=h)
      info, plan = h.last_solve_info(), h.last_cg_plan()
      assert info['solver'] == 'cg' and info['cg_status'] == 0 and 0 < info['iterations'], (info, plan)
    w, b = w.cpu().numpy(), b.cpu().numpy()
  assert plan == {'kernel': 'compact', 'rows': 0, 'channels_per_workgroup': case.cpw,
                  'workgroups': case.workgroups}, plan
  _check(case, ce.case_id(case), w, b, ref, plan, info['iterations'])


@pytest.mark.parametrize('case', ce.REFUSED_CASES, ids=ce.case_id)
def test_refused_shapes_take_the_factorisation(dev, handles, case):
  """An odd channel count and 33 lags: td_cg_solve_compact refuses, the resident kernel does not fit the declared CUs
  either -- the answer is the factorisation's bit for bit and no conjugate-gradient kernel was launched."""
  h, _ = handles(case.where)
  st = _accumulate(dev, h, case)
  try:
    w, b = (t.cpu().numpy() for t in st.ridge_solve(list(case.lams), handle=h))
    info, plan = h.last_solve_info(), h.last_cg_plan()
    h.set_solver('cholesky')
    wc, bc = (t.cpu().numpy() for t in st.ridge_solve(list(case.lams), handle=h))
  finally:
    h.set_solver('auto')
  assert info['solver'] == 'cholesky', (case.why, info)
  assert plan == {'kernel': 'none', 'rows': 0, 'channels_per_workgroup': 0, 'workgroups': 0}, (case.why, plan)
  assert h.last_cg_plan()['kernel'] == 'none'
  assert np.array_equal(w, wc) and np.array_equal(b, bc), case.why
  # (and the factorisation is right: the same reference, a float32 rounding plus the factorisation's own float64 error)
  ref = _reference(st, case)
  assert np.max(np.abs(w - ref.w)) <= 2.5e-7 * np.max(np.abs(ref.w))
