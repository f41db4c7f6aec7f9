"""CPU checks of tests/cca_sweep_edges.py, from the reference alone (the sums of tests/host_cca_sweep.LagStats): every
table case meets the gap condition its bound assumes, every status case sits on the expected side of its rule with room,
every case reaches the host branch it is named for by the restated arithmetic, the right model of the kernel passes the
bound and the four wrong ones do not."""
import numpy as np
import pytest

from tests import cca_sweep_edges as ce
from tests import host_cca_sweep as hc


def _by_name(name):
  return next(c for c in ce.CASES if c.name == name)


@pytest.fixture(scope='module')
def refs():
  """case name -> (total, parts, Reference); computed once, not to be written."""
  made = {}

  def get(case):
    if case.name not in made:
      total, parts = ce.cpu_moments(case)
      made[case.name] = (total, parts, ce.reference(total, parts, case.folds, case.lambdas, case.dim))
    return made[case.name]
  return get


@pytest.mark.parametrize('case', ce.CASES + [ce.NAN_CASE], ids=ce.case_id)
def test_gap_condition_and_status_margins(refs, case):
  """g >= 1e-3 for every pair that is solved; a pair that must report 0 keeps every rule's quantity at least 8x (the
  pivot) / 1e3x (C_yy, sigma) -- here: the smallest of them 1e3x -- on the good side, a pair that must report 1 has the
  deciding quantity as far on the other."""
  _, _, ref = refs(case)
  expect = dict(case.expect)
  for f, row in enumerate(ref.pairs):
    for l, p in enumerate(row):
      if case.kind == 'nan' and f == 2:
        assert p.rules.status == 1 and p.rot_x is None
        continue
      assert p.rules.margin >= (8.0 if p.rules.rule == 1 else 1e3), (f, l, p.rules)
      if 'status' in expect:
        assert p.rules.status == expect['status'][f][l] and p.rules.rule == expect['rules'][l], (f, l, p.rules)
      else:
        assert p.rules.status == 0, (f, l, p.rules)
      if not p.rules.status:
        assert p.g >= ce.G_MIN, (f, l, p.g)
        assert p.d_e <= 1e-13 and max(p.d_x.max(), p.d_y.max()) <= 1e-10, (f, l, p.d_e, p.d_x, p.d_y)
  if case.kind is not None:     # pairs to be right beside pairs to be refused, in one launch
    flat = [p.rules.status for row in ref.pairs for p in row]
    assert (0 in flat or case.name == 'status_dup_x2_full_dim') and 1 in flat


@pytest.mark.parametrize('case', ce.CASES, ids=ce.case_id)
def test_case_reaches_the_branch_it_is_named_for(case):
  k1, k2 = ce.case_k(case)
  pl = ce.plan(k1, k2, case.dim, len(case.folds), len(case.lambdas))
  for key, want in case.expect:
    if key not in ('status', 'rules'):
      assert getattr(pl, key) == want, (key, getattr(pl, key), want)
  assert len(case.lambdas) * case.dim <= ce.MAX_COLUMNS and case.dim <= min(k1, k2) and k2 <= 64
  assert pl.by_bytes > pl.by_count or pl.by_bytes >= len(case.folds)      # (no case here is cut by bytes)
  assert all(len(f) <= 4 for f in case.folds) and all(n > 1 for n in ce.fold_frames(case))
  if case.kind is None:
    assert min(ce.fold_frames(case)) > k1 + k2                             # full rank without lambda's help


def test_the_table_covers_every_named_route():
  """The batch routes of chol_factor_forward at nblk = 3, both chunk cases, the second trip of the backward pass, the
  widths on both sides of every tile edge, and the term shapes."""
  routes = {}
  for case in ce.CASES:
    if case.name.startswith('batch_'):
      k1, k2 = ce.case_k(case)
      pl = ce.plan(k1, k2, case.dim, len(case.folds), len(case.lambdas))
      assert pl.nblk == 3 and len(pl.batches) == 1
      routes[pl.batches[0]] = ce.factor_plan(pl.nblk, pl.batches[0])
      assert len(set(case.folds)) == len(case.folds)                       # distinct folds: a mix-up shows
  assert sorted(routes) == [1, 2, 3, 7, 8, 9, 17]
  assert [routes[b].ow for b in (1, 2, 3)] == [1, 1, 4] and [routes[b].panel_tiles for b in (2, 3)] == [1, 3]
  assert [routes[b].by_xcd for b in (7, 8)] == [False, True]
  assert [routes[b].phantom for b in (8, 9, 17)] == [0, 7, 7] and routes[17].grid_systems == 24
  assert all(r.updates == 2 for r in routes.values())
  chunks = _by_name('chunks_8_1')
  pl = ce.plan(5, 2, 2, 9, 20)
  assert pl.chunks == ((0, 8), (8, 1)) and pl.batches == (160, 20) and not pl.clamped and pl.by_count == 8
  assert len(set(chunks.folds)) == 9
  pl = ce.plan(5, 2, 1, 2, 161)
  assert pl.by_count == 0 and pl.clamped and pl.chunks == ((0, 1), (1, 1)) and pl.batches == (161, 161)
  assert [ce.plan(70, 20, d, 2, 2).backward_trips for d in (1, 7, 8, 9, 16, 17, 20)] == [1, 1, 1, 2, 2, 3, 3]
  names = {c.name for c in ce.CASES}
  assert {'k1_%d' % k for k in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)} <= names
  assert {'k2_%d' % k for k in (1, 2, 7, 8, 9, 15, 16, 17, 33, 63, 64)} <= names
  assert ce.case_k(_by_name('k1_below_k2')) == (5, 12) and ce.case_k(_by_name('dim_20')) == (70, 20)
  terms = _by_name('terms')
  assert sorted(len(f) for f in terms.folds) == [0, 1, 2, 2, 3, 4] and terms.batch_size == 10
  assert all(n % 10 == 0 for n in terms.parts)
  assert sum(1 for f in terms.folds if any(p == 3 for p, _ in f)) >= 2     # one object in several folds
  assert terms.folds[-1] == ((2, 1.0), (2, -1.0)) and ce.fold_frames(terms)[-1] == ce.fold_frames(terms)[0]
  assert any({sg for _, sg in f} == {1.0, -1.0} for f in terms.folds[:-1])


@pytest.mark.parametrize('name', ['k1_65', 'k1_193', 'dim_9', 'dim_20', 'chunks_8_1', 'terms', 'batch_9'])
def test_the_right_model_is_inside_the_bound(refs, name):
  case = _by_name(name)
  total, parts, ref = refs(case)
  rep = ce.check(ce.model(total, parts, case.folds, case.lambdas, case.dim), ref)
  assert not rep.failures and rep.status_ok and rep.means_ok and rep.bias_ok, rep.failures
  assert rep.pairs_checked == len(case.folds) * len(case.lambdas)
  assert rep.ratio_e <= 1.0 and rep.ratio_rot <= 1.0
  # the bound is the float32 rounding of the output and little else
  assert rep.bound_e <= 2.0 ** -24 + 1e-9 and rep.bound_rot <= 2.0 ** -24 + 1e-8, (rep.bound_e, rep.bound_rot)


WRONG_ON = [('drop_last_block', 'k1_65'), ('drop_last_block', 'k1_129'), ('drop_last_block', 'k1_193'),
            ('ut_from_8_zero', 'dim_9'), ('ut_from_8_zero', 'dim_17'), ('ut_from_8_zero', 'dim_20'),
            ('chunk_state', 'chunks_8_1'), ('chunk_state', 'chunk_clamp'),
            ('flip_sign', 'terms'), ('flip_sign', 'k1_2'), ('flip_sign', 'batch_17')]


@pytest.mark.parametrize('wrong,name', WRONG_ON)
def test_the_bound_rejects_a_wrong_kernel(refs, wrong, name):
  """Each model of a wrong kernel leaves the bound of e or of the rotations on the cases meant to catch it -- by a
  factor of 100 at least, so the rejection does not hang on the bound's last digit."""
  case = _by_name(name)
  total, parts, ref = refs(case)
  rep = ce.check(ce.model(total, parts, case.folds, case.lambdas, case.dim, wrong=wrong), ref)
  if wrong == 'flip_sign':
    # (sums of one sign under the frame count of the other: where the covariance is still positive definite the bound
    # rejects the pair, where it is not the pair reports 1 against the reference's 0)
    flipped = [f for f, fold in enumerate(case.folds) if fold]
    assert all(any(m.startswith('pair (%d, ' % f) for m in rep.failures) for f in flipped), rep.failures
    assert not rep.status_ok or max(rep.ratio_e, rep.ratio_rot) > 100.0
    assert not rep.means_ok
    return
  assert rep.status_ok, rep.failures
  assert max(rep.ratio_e, rep.ratio_rot) > 100.0, (wrong, name, rep.ratio_e, rep.ratio_rot)
  if wrong == 'ut_from_8_zero':
    assert rep.ratio_e <= 1.0                    # (only rot_x shows it)
  if wrong == 'chunk_state':
    assert not rep.means_ok


def test_stand_in_follows_the_device_pivot_rule():
  """The NumPy stand-in of the device layer marks the pairs the reference's rules mark: LAPACK alone accepts a pivot of
  rounding noise that comes out positive."""
  for case in ce.STATUS_CASES:
    pre1, post1, pre2, post2 = ce.lags(case)
    stats = []
    for x, x2 in ce.make_parts(case):
      st = hc.LagStats(case.c1, pre1, post1, case.c2, pre2, post2, handle=object())
      st.accumulate(x, x2, None, [0, len(x)])
      stats.append(st)
    total = stats[0].__class__(case.c1, pre1, post1, case.c2, pre2, post2, handle=object()).combine(stats[:case.n_total])
    out = hc.LagStats.cca_solve_loso_terms(total, [[(stats[p], sg) for p, sg in f] for f in case.folds],
                                           ce.fold_batches(case), case.batch_size, case.lambdas, case.dim)
    assert np.asarray(out[7]).tolist() == [list(r) for r in dict(case.expect)['status']]


def test_end_to_end_case_splits_as_the_statuses_dictate():
  """The duplicated-channel sweep of the GPU test through the stand-in: the lambda = 0 pairs take the fallback, the
  others the batched route, and both agree with the from-scratch refits (atol as tests/test_cpu_cca_sweep.py)."""
  from telluride_decoding_amd import brain_data, regression
  c = ce.E2E
  ds = brain_data.Dataset(list(ce.e2e_files()), c['batch'], c['pre'], c['post'], c['pre2'], c['post2'])
  res = regression.jackknife_over_regularizations(ds, list(c['lambdas']), device=hc, model='cca', cca_dims=c['dim'])
  assert regression.LAST_SWEEP['cca_route'] == 'batched+per_fold'
  assert regression.LAST_SWEEP['cca_pairs'] == {'batched': 3, 'per_fold': 3}
  want = ce.e2e_oracle()
  for (f, li), r in want.items():
    assert abs(res['all_runs'][li, f] - r) <= 2e-6, (f, li, res['all_runs'][li, f], r)
