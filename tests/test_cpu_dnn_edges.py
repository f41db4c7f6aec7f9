"""The case tables of tests/dnn_edges.py without a GPU: every case of tests/test_gpu_dnn_edges.py is built here too and
must be accepted inside the redraw caps of the suites whose recipes it follows (a change to a recipe then fails here
and not as a pytest.fail on the GPU), and the plan arithmetic of mlp_check_and_plan, restated in tests/dnn_edges.plan,
must show that the tables reach what they claim to: every tile width of the slab kernel, dead tail columns, short row
chunks, short and several head workgroups, short last slices."""
import numpy as np
import pytest

from tests import dnn_edges as de
from tests.dnn_common import KINK
from tests.test_gpu_classifier import MARGIN, MARGIN_TRAJ, MAX_DRAWS


# ---- (a) every case is accepted within the caps ------------------------------------------------------------------
@pytest.mark.parametrize('loss,shape', [('mse', s) for s in de.MSE_GRID] + [('pearson', s) for s in de.PEARSON_GRID],
                         ids=lambda v: v if isinstance(v, str) else de.regressor_id(v))
def test_regressor_gradient_cases_are_accepted_at_the_first_draw(loss, shape):
  case = de.regressor_grad_case(loss, *shape)
  assert case is not None
  assert case['draws'] == 1 and case['kink'] >= KINK
  hidden, c, pre, post, batch, d, off = shape
  assert case['g64'][0].shape == (c * (pre + 1 + post), (hidden + [d])[0])
  if batch > 1:                                  # the tested minibatch lies across the first file boundary
    assert case['s'] * batch < case['first'] < (case['s'] + 1) * batch
  else:
    assert case['s'] == 7                        # (a batch of one row: the first row of the second file)
  if not hidden:
    assert case['kink'] == np.inf


@pytest.mark.parametrize('shape', de.CLASSIFIER_GRID, ids=de.classifier_id)
def test_classifier_gradient_cases_are_accepted_at_the_first_draw(shape):
  case = de.classifier_grad_case(*shape)          # (fails by itself past MAX_DRAWS; asserts the straddled boundary)
  assert case['draws'] == 1 and case['margin'] >= MARGIN
  hidden, c, pre, post, c2, pre2, post2, batch, d, off = shape
  k1, p = c * (pre + 1 + post), de.plan_of_classifier(shape)
  assert k1 % p['ks'] != 0 and k1 < case['widths'][0]          # one slice gathers from both views


# The draw (from 0) each trajectory is accepted at, in order and shuffled, as built when the cases were chosen.  The
# classifier's shape B, shuffled, takes the last of its MAX_DRAWS: if a change to the recipe moves it past the cap,
# change a length of TRAJ_CB, not the cap.
ACCEPTED_DRAW = {('mse', 'A'): (0, 0), ('mse', 'B'): (2, 4), ('mse', 'C'): (0, 0), ('pearson', 'A'): (0, 0),
                 ('pearson', 'B'): (3, 2), ('classifier', 'A'): (0, 0), ('classifier', 'B'): (1, 2)}


@pytest.mark.parametrize('shuffle', [None, de.SHUFFLE], ids=['in_order', 'shuffled'])
@pytest.mark.parametrize('loss,name', sorted(de.REGRESSOR_TRAJ))
def test_regressor_trajectories_are_accepted_within_the_cap(loss, name, shuffle):
  case = de.regressor_trajectory_case(loss, name, shuffle)
  assert case is not None
  assert case['draws'] <= de.REGRESSOR_DRAWS and case['kink'] >= de.KINK_TRAJ
  assert case['seed'] == ACCEPTED_DRAW[(loss, name)][shuffle is not None]
  t = case['t']
  assert case['steps'] == sum(t['lengths']) // t['batch'] and case['steps'] >= 4
  assert all(len(v) == t['epochs'] for v in case['hist64'].values())


@pytest.mark.parametrize('shuffle', [None, de.SHUFFLE], ids=['in_order', 'shuffled'])
@pytest.mark.parametrize('name', sorted(de.CLASSIFIER_TRAJ))
def test_classifier_trajectories_are_accepted_within_the_cap(name, shuffle):
  case = de.classifier_trajectory_case(name, shuffle)
  assert case is not None
  assert case['draws'] <= MAX_DRAWS and case['margin'] >= MARGIN_TRAJ
  assert case['seed'] == ACCEPTED_DRAW[('classifier', name)][shuffle is not None]
  t = case['t']
  assert case['steps'] == sum(t['lengths']) // t['batch'] and case['steps'] >= 4


# ---- (b) what the tables reach -------------------------------------------------------------------------------------
def test_plan_restatement_on_known_shapes():
  """The shapes whose plans the existing suites and csrc/mlp.hip spell out."""
  p = de.plan(2368 + 37, [20], 1, 512)           # the match-mismatch shape: ks = 40
  assert (p['ks'], p['nj'], p['n_head'], p['head_last']) == (40, 24, 8, 64)
  p = de.plan(8192, [], 1, 2048)                 # the largest K: 128 slices of 64 rows
  assert (p['ks'], p['nslices'], p['last_slice'], p['nj'], p['n_head']) == (64, 128, 64, 4, 32)
  p = de.plan(15, [8, 4], 2, 32)                 # test_gpu_dnn_many's recipe: slices of 4, 4, 4 and 3 rows
  assert (p['ks'], p['nslices'], p['last_slice'], p['nj'], p['n_head'], p['head_last']) == (4, 4, 3, 8, 1, 32)
  p = de.plan(504, [32], 5, 100)
  assert (p['ks'], p['nslices'], p['last_slice']) == (8, 63, 8)
  p = de.plan(130, [17], 1, 130)
  assert (p['ks'], p['nslices'], p['last_slice'], p['nj'], p['n_head'], p['head_last']) == (4, 33, 2, 24, 3, 2)


def _batch(shape):
  return shape[-3]


def test_gradient_tables_reach_every_tile_edge():
  families = {'mse': [(s, de.plan_of_regressor(s)) for s in de.MSE_GRID],
              'pearson': [(s, de.plan_of_regressor(s)) for s in de.PEARSON_GRID],
              'classifier': [(s, de.plan_of_classifier(s)) for s in de.CLASSIFIER_GRID]}
  # every instantiation of the slab kernel: in the mse grid alone, and so in the three together
  assert {p['nj'] for _, p in families['mse']} == set(de.SLAB_WIDTHS)
  for name, cases in families.items():
    # dead tail columns: a first layer wider than one float4 that is no multiple of it
    assert any(p['w1'] % 4 != 0 and p['w1'] > 4 for _, p in cases), name
    # a full tile too, so that the predicates are seen both ways
    assert any(p['w1'] == p['nj'] for _, p in cases), name
    # a short row chunk and a short head workgroup after a full one, of 1 or 6 rows
    assert any(_batch(s) > 64 and _batch(s) % 64 in (1, 6) for s, _ in cases), name
    assert any(p['n_head'] >= 2 and p['head_last'] < de.ROW_TILE for _, p in cases), name
    # a short last slice of W1
    assert any(p['last_slice'] < p['ks'] for _, p in cases), name
  # a batch below one row chunk, so that the only chunk and the only head workgroup are short: where the head is
  # mlp_head_kernel<0> (the Pearson grid of tests/test_gpu_dnn_pearson.py has its own, B = 32)
  for name in ('mse', 'classifier'):
    assert any(_batch(s) < 64 for s, _ in families[name]), name
  assert any(_batch(s) == 1 for s, _ in families['mse'])
  # ks > 4, K = 1, c > 128, 64 lags, no hidden layer, four hidden layers whose widest is not the first
  mse = [s for s, _ in families['mse']]
  assert any(p['ks'] > 4 for _, p in families['mse'])
  assert any(s[1] * (s[2] + s[3] + 1) == 1 for s in mse) and any(s[1] > 128 for s in mse)
  assert any(s[2] + s[3] + 1 == 64 for s in mse) and any(not s[0] for s in mse)
  assert any(len(s[0]) == 4 and max(s[0]) != s[0][0] for s in mse)


def test_trajectory_shapes_have_more_than_one_of_everything():
  shapes = list(de.REGRESSOR_TRAJ.values()) + list(de.CLASSIFIER_TRAJ.values())
  for t in shapes:
    p = de.plan_of_trajectory(t)
    assert p['n_head'] >= 2, t
    assert p['last_slice'] < p['ks'] or p['ks'] > 4, t
    assert p['nslices'] >= 7 and sum(t['lengths']) // t['batch'] >= 4, t
  plans = [de.plan_of_trajectory(t) for t in shapes]
  assert {p['nj'] for p in plans} >= {16, 24, 32}                   # the tiles of [13, 6], [20, 20] and [30]
  assert any(p['w1'] % 4 != 0 for p in plans)                        # the refreshed tile has dead columns
  assert any(p['head_last'] < de.ROW_TILE for p in plans) and any(p['n_head'] == 3 for p in plans)
  assert any(p['last_slice'] == 1 for p in plans) and any(p['ks'] == 8 for p in plans)
  # the many-model cases hold out recordings that exist, and leave every model at least one minibatch
  for t, held in ((de.TRAJ_A, de.MANY_HELD_A), (de.TRAJ_CB, de.MANY_HELD_CB)):
    for h in held:
      assert all(0 <= f < len(t['lengths']) for f in h)
      assert sum(n for f, n in enumerate(t['lengths']) if f not in h) >= t['batch']
  p = de.plan(de.PREDICT['c'] * (de.PREDICT['pre'] + 1 + de.PREDICT['post']), de.PREDICT['hidden'], de.PREDICT['d'],
              de.PREDICT['batch'])
  assert p['nj'] == 32 and p['w1'] == 27
  assert sum(de.PREDICT['lengths']) > 2 * 4096 and sum(de.PREDICT['lengths']) % 4096 != 0
