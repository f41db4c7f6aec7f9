"""CPU tests of the conjugate-gradient edge sweep (tests/cg_edges.py): the tables reach every kernel instance of
csrc/cg.hip with the grids they state, the derived bound stays at one float32 rounding on the tables' data, and a
product that is wrong in one row, or lacks one head-window term, lands far outside it.  No GPU needed."""
import numpy as np
import pytest

from tests import cg_edges as ce


def test_tables_reach_every_instance_with_the_stated_grids():
  for case in ce.RESIDENT_CASES:
    k = case.c * (case.post + 1)
    cus = ce.case_cus(case)
    assert not ce.sync_takes_compact(k, cus), case
    assert ce.dense_plan(k, cus) == (case.rows, case.workgroups), case
    assert k + 1 >= 3
  assert {c.rows for c in ce.RESIDENT_CASES} == set(range(1, 9))
  # every R from 2 on with a ragged last workgroup, and at its own declared count
  ragged = {c.rows for c in ce.RESIDENT_CASES if (c.c * (c.post + 1)) % c.rows}
  assert ragged == set(range(2, 9))
  want = {97: [97, 49, 33, 25, 20, 17, 14, 13], 99: [99, 50, 33, 25, 20, 17, 15, 13]}
  for k, wgs in want.items():
    got = [c.workgroups for c in ce.RESIDENT_CASES if c.c * (c.post + 1) == k and len(c.lams) * c.d == 1]
    assert got == wgs and [c.declared for c in ce.RESIDENT_CASES if c.c * (c.post + 1) == k and c.d == 1] == wgs
  by_k = {c.c * (c.post + 1): (c.rows, c.workgroups) for c in ce.RESIDENT_CASES if c.declared is None}
  assert by_k == {1025: (5, 205), 1023: (4, 256), 2047: (8, 256), 2: (1, 2), 3: (1, 3)}

  for case in ce.COMPACT_CASES:
    k = case.c * (case.post + 1)
    cus = ce.case_cus(case)
    assert ce.compact_plan(case.c, case.post, case.files, cus, len(case.lams)) == (case.cpw, case.workgroups), case
    assert len(case.lams) * case.d <= 4
    if not case.use_async:          # the synchronous route asks the compact solver only where the dense one cannot run
      assert ce.sync_takes_compact(k, cus), case
  assert {c.cpw for c in ce.COMPACT_CASES} == {1, 2}
  # kCpw = 2 exactly when cus < C <= 2 cus
  for case in ce.COMPACT_CASES:
    cus = ce.case_cus(case)
    assert (case.cpw == 2) == (cus < case.c <= 2 * cus), case
  # the capacities the table claims: pairs == waves on 32 CUs (16 files) and for C = 4 on 2, 496 of 512 on 64
  full = [c for c in ce.COMPACT_CASES if c.cpw == 2 and c.files * ((c.post + 1) // 2) == ce.WAVES * c.workgroups]
  assert {(c.c, c.files) for c in full} == {(64, 16), (4, 1)}
  assert any(c.cpw == 1 and c.files * c.post == 496 for c in ce.COMPACT_CASES)
  assert any(c.cpw == 2 and c.post % 2 == 0 and c.post > 0 for c in ce.COMPACT_CASES)
  assert any(c.cpw == 2 and c.post == 0 for c in ce.COMPACT_CASES)

  for case in ce.REFUSED_CASES:
    k = case.c * (case.post + 1)
    cus = ce.case_cus(case)
    assert ce.sync_takes_compact(k, cus), case          # the compact solver IS asked ...
    assert ce.compact_plan(case.c, case.post, case.files, cus) is None, case      # ... and refuses
    assert ce.dense_plan(k, cus) is None, case          # and the resident kernel cannot step in
  ids = [ce.case_id(c) for c in ce.RESIDENT_CASES + ce.COMPACT_CASES + ce.REFUSED_CASES]
  assert len(set(ids)) == len(ids)


def _all_cases():
  return ce.RESIDENT_CASES + ce.COMPACT_CASES


@pytest.mark.parametrize('case', _all_cases(), ids=ce.case_id)
def test_the_bound_is_one_float32_rounding_on_the_tables_data(case):
  """E below a tenth of 2^-24 max|w_ref|, with the accept the case's solve runs with: what the GPU test checks is in
  effect the float32 rounding of the output.  (cond(A) is 1.1 .. 12 except where a case has fewer frames than
  unknowns -- C = 64 with 3 x 400 frames: the matrix is lambda I on a subspace, cond = 52.)"""
  xtx, xty, frames = ce.cpu_moments(case)
  ref = _reference(case)
  for li in range(len(case.lams)):
    for o in range(case.d):
      assert ref.e[li, o] < 0.1 * 2.0 ** -24 * np.max(np.abs(ref.w[li, :, o])), (ref.cond[li], ref.e[li, o])
  assert np.all(ref.cond < 60.0), ref.cond


_REFS = {}


def _reference(case):
  key = (case.c, case.post, case.frames, case.files, case.d, case.lams, ce.case_accept(case))
  if key not in _REFS:
    xtx, xty, frames = ce.cpu_moments(case)
    _REFS[key] = ce.reference(xtx, xty, frames, case.lams, ce.case_accept(case))
  return _REFS[key]


@pytest.mark.parametrize('case,row', [
    (ce.RESIDENT_CASES[1], 96),       # k = 97, R = 2: the single row of the ragged last workgroup
    (ce.RESIDENT_CASES[10], 98),      # k = 99, R = 3 ... the last row
    (ce.RESIDENT_CASES[12], 50),      # k = 99, R = 5: a row in the middle
], ids=lambda v: ce.case_id(v) if not isinstance(v, int) else 'row%d' % v)
def test_one_wrong_row_of_the_product_lands_far_outside_the_bound(case, row):
  xtx, xty, frames = ce.cpu_moments(case)
  ref = _reference(case)
  a = xtx / frames + case.lams[0] * np.eye(len(xtx))
  rhs = xty[:, 0] / frames
  good, ok = ce.cg_model(lambda v: a @ v, rhs)
  assert ok
  assert ce.distance(good[:-1].astype(np.float32)[None, :, None], good[-1:].astype(np.float32)[None, :], ref)[2] <= 1.0
  bad, _ = ce.cg_model(ce.wrong_row_product(a, row), rhs)
  # (wherever the iteration ends -- with such a product it does not even converge, which the GPU test's status
  # assertion sees first -- the weights are far off)
  ratio = ce.distance(bad[:-1][None, :, None], bad[-1:][None, :], ref)[2]
  assert ratio > 100.0, ratio


def test_one_head_window_term_left_out_lands_far_outside_the_bound():
  case = ce.COMPACT_CASES[7]          # C = 4, post = 31, one recording: k = 128
  eeg, env, offs = ce.make_data(case)
  xtx, xty, frames = ce.cpu_moments(case)
  ref = _reference(case)
  k = case.c * (case.post + 1)
  terms = dict(ce.head_terms(case, eeg, offs))
  assert len(terms) == case.files * case.post
  # the compact form IS the dense matrix
  m = ce.toeplitz_part(case, eeg, offs) - sum(terms.values())
  assert np.max(np.abs(m - xtx[:k, :k])) <= 1e-10 * np.max(np.abs(xtx))
  for key in ((0, 0), (0, 17), (0, case.post - 1)):      # the first, one in the middle, the last q number
    bad = xtx.copy()
    bad[:k, :k] += terms[key]
    a = bad / frames + case.lams[0] * np.eye(k + 1)
    sol = np.linalg.solve(a, xty[:, 0] / frames)           # what conjugate gradients with that product converge to
    ratio = ce.distance(sol[:-1][None, :, None], sol[-1:][None, :], ref)[2]
    assert ratio > 100.0, (key, ratio)
