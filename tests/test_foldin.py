"""GPU: rk_als_foldin against the f32 restatement of tests/foldin_util.py bit for bit (X and status) at both ends of
every launch shape, and fold-in through ``Recoder``: PureSVD's own rows at alpha = reg = 0, the exact ALS half-step,
users no fit has seen, ``FoldInRecommender`` under ``RecommenderEvaluator``, and the serving path left as it was."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import foldin_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
X_PAD = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]      # what the padding of X holds before and after


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, pad, fill):
  out = np.full((a.shape[0], a.shape[1] + pad), fill, np.float32)
  out[:, :a.shape[1]] = a
  return out


def _run(csr, Y, G, v, bias, alpha, use_data=True, row_lo=0, row_hi=None, rows_out=None):
  """rk_als_foldin with ldy = h + 3 (NaN in the padding: a read of it poisons the row) and ldx = h + 5 (X_PAD in the
  padding, and in every row the call does not own); returns (the whole padded X, status with -7 where not written)."""
  from recoder_amd import als, foldin
  h = Y.shape[1]
  c = als.AlsCSR(csr, DEV)
  if not use_data:
    c.data = None
  elif c.data is None:
    c.data = _t(csr.data)
  n = csr.shape[0] if rows_out is None else rows_out
  Yt = _t(_padded(Y, 3, np.nan))
  Xt = _t(np.full((n, h + 5), X_PAD, np.float32))
  st = torch.full((n,), -7, dtype=torch.int32, device=DEV)
  row_hi = csr.shape[0] if row_hi is None else row_hi
  foldin.solve(c, Yt[:, :h], _t(G), _t(v), None if bias is None else _t(bias), alpha, X=Xt[row_lo:, :h],
               status=st[row_lo:], row_lo=row_lo, row_hi=row_hi)
  return Xt.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("h", U.HS)
def test_kernel_equals_the_restatement_bit_for_bit(h):
  p = U.problem(h)
  csr, B = p["csr"], p["csr"].shape[0]
  assert B == 37 and {0, 1, 5, 700} <= set(p["lens"]) and max(p["lens"]) > U.CHUNK
  for vi, (name, alpha, use_data, bias_given) in enumerate(U.VARIANTS):
    v, bias = U.variant_inputs(p, bias_given)
    want, want_st = U.want(h, vi)
    got, st = _run(csr, p["Y"], p["G"], v, bias, alpha, use_data)
    wrong = [(u, p["lens"][u]) for u in range(B) if got[u, :h].tobytes() != want[u].tobytes()]
    assert wrong == [], ("(row, entries) that differ from foldin_row32", name, wrong)
    assert np.array_equal(st, want_st) and not st.any(), name
    assert got[:, h:].tobytes() == np.full((B, 5), X_PAD, np.float32).tobytes(), "padding of X written"
    if not bias_given:                                       # an empty row without a bias: exactly zero
      assert not got[0, :h].any() and not got[10, :h].any()
    else:
      assert got[0, :h].any()
    if vi:
      continue
    again, st2 = _run(csr, p["Y"], p["G"], v, bias, alpha, use_data)
    assert again.tobytes() == got.tobytes() and np.array_equal(st, st2), "not bitwise repeatable"
    # a sub-batch [3, 9) gives the rows of the full call and touches no other row
    sub, sst = _run(csr, p["Y"], p["G"], v, bias, alpha, use_data, row_lo=3, row_hi=9)
    assert sub[3:9].tobytes() == got[3:9].tobytes() and np.array_equal(sst[3:9], st[3:9])
    assert (sub[:3].view(np.uint32) == 0xDEADBEEF).all() and (sub[9:].view(np.uint32) == 0xDEADBEEF).all()
    assert (sst[:3] == -7).all() and (sst[9:] == -7).all()
    # B = 1: the long row and the empty row alone
    for u in (3, 0):
      one, ost = _run(csr[u], p["Y"], p["G"], v, bias, alpha, use_data)
      assert one[0, :h].tobytes() == want[u].tobytes() and ost.tolist() == [0], u


def test_singular_row_comes_back_as_zeros_with_status_one():
  """reg = 0 and a rank-deficient Y: the second pivot is exactly 0.  The row is +0, its status 1, nothing faults, and
  a regular row in the same call is not touched by it."""
  s = U.singular_problem()
  want, want_st = U.foldin32(s["csr"], s["Y"], s["G"], s["v"], s["bias"], 10.0)
  got, st = _run(s["csr"], s["Y"], s["G"], s["v"], s["bias"], 10.0)
  assert st.tolist() == want_st.tolist() == [1]
  assert got[0, :3].tobytes() == want[0].tobytes() == np.zeros(3, np.float32).tobytes()
  G = s["G"] + np.eye(3, dtype=np.float32)                   # the same Y with reg = 1: a regular system
  two = sp.csr_matrix(np.array([[0, 0, 0, 0], [2.0, 0, 1.0, 0]], np.float32))
  want, want_st = U.foldin32(two, s["Y"], G, s["v"], s["bias"], 10.0)
  got, st = _run(two, s["Y"], G, s["v"], s["bias"], 10.0)
  assert st.tolist() == want_st.tolist() == [0, 0] and got[:, :3].tobytes() == want.tobytes()


def test_h_above_the_limit_is_an_error():
  from recoder_amd import _als_lib
  from recoder_amd._lib import RecoderHipError
  lib = _als_lib.load()
  z = torch.zeros(200 * 200, dtype=torch.float32, device=DEV)
  i = torch.zeros(8, dtype=torch.int64, device=DEV)
  rc = lib.rk_als_foldin(i.data_ptr(), i.data_ptr(), None, 1, z.data_ptr(), 129, 129, z.data_ptr(), z.data_ptr(), None,
                         1.0, z.data_ptr(), 129, i.data_ptr(), None)
  assert rc == -2
  with pytest.raises(RecoderHipError, match="1 <= h <= 128"):
    _als_lib.check(rc, "rk_als_foldin")


# ----------------------------------------------------------------------------------------------- through Recoder
def _recoder(h):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", loss_params={"confidence": 10.0}, optimizer_type="adam")


def _tables(rec):
  m = rec.model
  return (m.user_embedding_layer.weight.data, m.item_embedding_layer.weight.data, m.bias.data)


ALS_REG = 5.0


@pytest.fixture(scope="module")
def svd_fit():
  from recoder_amd.data import RecommendationDataset
  m = U.prop_matrix()
  rec = _recoder(8)
  rec.train_svd(RecommendationDataset(m), seed=3)
  return rec, m


@pytest.fixture(scope="module")
def als_fit():
  from recoder_amd.data import RecommendationDataset
  m = U.prop_matrix()
  rec = _recoder(16)
  rec.train_als(RecommendationDataset(m), num_iterations=5, reg=ALS_REG, cg_steps=3)
  return rec, m


def _unseen(m, n=20, seed=11):
  """n histories over the model's items that are not rows of ``m``, and as many held-out rows."""
  rng = np.random.RandomState(seed)
  x = (rng.rand(n, m.shape[1]) < 0.1).astype(np.float32)
  x[np.arange(n), rng.randint(0, m.shape[1], n)] = 1.0
  y = ((rng.rand(n, m.shape[1]) < 0.1) & (x == 0)).astype(np.float32)
  rows = {r.tobytes() for r in np.asarray(m.todense(), np.float32)}
  assert not any(r.tobytes() in rows for r in x)
  return sp.csr_matrix(x), sp.csr_matrix(y)


def test_puresvd_rows_fold_in_to_the_user_table(svd_fit):
  """alpha = 0, reg = 0: x = (V^T V)^-1 V^T r, and V^T V is the identity up to the SVD's residual, so the folded rows
  are the model's (U = A V) within the host test's bound at that G."""
  from recoder_amd import als
  rec, m = svd_fit
  Xu, Y, b = _tables(rec)
  assert not b.any()
  got = rec.fold_in(m, alpha=0.0, reg=0.0)
  assert got.shape == (U.PROP_USERS, 8) and got.dtype == torch.float32 and got.is_cuda
  G, _ = als.gram(Y, 0.0, b)
  cond = np.linalg.cond(G.cpu().numpy().astype(np.float64), 2)
  bound = U.bound(8, np.diff(m.indptr), cond)
  want = Xu.cpu().numpy().astype(np.float64)
  err = np.linalg.norm(got.cpu().numpy().astype(np.float64) - want, axis=1) / np.linalg.norm(want, axis=1)
  print("cond(V^T V) - 1 = %.3g; worst relative error %.3g at bound %.3g" % (cond - 1, err.max(), bound[err.argmax()]))
  assert (err <= bound).all(), (err.max(), bound.min())


def test_puresvd_recommend_folded_is_recommend_where_the_gaps_decide(svd_fit):
  """Position by position: the same id wherever the exact rows' score stands clear of both neighbours by more than
  2 * bound * |x| max|y| (each of the two scores moves by at most bound |x| |y|); at most 2 % of the positions may go
  undecided (1.2 % in float64: tests/test_foldin_host.py)."""
  from recoder_amd import als
  from recoder_amd.data import UsersInteractions
  rec, m = svd_fit
  Xu, Y, b = (t.cpu().numpy().astype(np.float64) for t in _tables(rec))
  users = np.arange(U.PROP_USERS)
  inp = UsersInteractions(users, m)
  plain = rec.recommend_array(inp, U.PROP_K)
  folded = rec.recommend_folded(inp, U.PROP_K, alpha=0.0, reg=0.0)
  shuffled = rec.recommend_folded(UsersInteractions(users[::-1].copy(), m), U.PROP_K, alpha=0.0, reg=0.0)
  assert np.array_equal(folded, shuffled), "users_interactions.users is read"
  G, _ = als.gram(_tables(rec)[1], 0.0, None)
  cond = np.linalg.cond(G.cpu().numpy().astype(np.float64), 2)
  thr = 2 * U.bound(8, np.diff(m.indptr), cond) * np.linalg.norm(Xu, axis=1) * np.linalg.norm(Y, axis=1).max()
  want, sure = U.decided(Xu @ Y.T + b, m, U.PROP_K, thr)
  print("undecided positions: %.2f %%; positions that differ: %d of %d"
        % (100 * (1 - sure.mean()), int((plain != folded).sum()), plain.size))
  assert 1 - sure.mean() <= 0.02
  assert np.array_equal(folded[sure], plain[sure])
  assert np.array_equal(folded[sure], want[sure])


def test_als_fold_in_of_the_training_rows_does_not_raise_the_objective(als_fit):
  """The exact minimiser of the user half-step cannot be worse than three CG steps."""
  from recoder_amd import als
  rec, m = als_fit
  X, Y, b = _tables(rec)
  ucsr, _ = als.csr_pair(m, X.shape[0], Y.shape[0], DEV)

  def objective(Xc):
    Gx, sx = als.gram(Xc, ALS_REG)
    Gy, cy = als.gram(Y, ALS_REG, b)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    als.objective(ucsr, Xc, Y, b, 10.0, ALS_REG, Gx, sx, Gy, cy, out)
    return float(out.item())
  before = objective(X)
  with warnings.catch_warnings():
    warnings.simplefilter("error")                           # (no row may fail at reg > 0)
    folded = rec.fold_in(m, alpha=10.0, reg=ALS_REG)
  after = objective(folded.contiguous())
  print("ALS objective: %.9g after 5 iterations, %.9g with the users folded in" % (before, after))
  assert after <= before * (1 + 1e-6)


def test_unseen_users_get_the_masked_top_k_of_their_folded_rows(als_fit):
  from recoder_amd.data import UsersInteractions
  rec, m = als_fit
  x, _ = _unseen(m)
  k = U.PROP_K
  inp = UsersInteractions(np.arange(x.shape[0]) + 10 ** 6, x)          # (ids no table has: they are not read)
  lists = rec.recommend_folded(inp, k, alpha=10.0, reg=ALS_REG)
  assert lists.shape == (20, k) and lists.dtype == np.int64
  rows = rec.fold_in(x, alpha=10.0, reg=ALS_REG)
  _, Y, b = _tables(rec)
  S = (rows @ Y.T + b).cpu().numpy().astype(np.float64)
  want = U.decided(S, x, k, np.zeros(20))[0]
  # the device scores in f32-class arithmetic (tests/test_svd.py): an item may trade places with one whose score is
  # within that rounding of it
  tol = 1e-5 * (np.abs(rows.cpu().numpy().astype(np.float64)) @ np.abs(Y.cpu().numpy()).max(axis=0).astype(np.float64)
                + float(b.abs().max()))
  for u in range(20):
    seen = x.indices[x.indptr[u]:x.indptr[u + 1]]
    assert len(set(lists[u])) == k and not np.isin(lists[u], seen).any()
    assert (np.abs(S[u, lists[u]] - S[u, want[u]]) <= tol[u]).all(), u
  same = float(np.mean(lists == want))
  print("unseen users: %.1f %% of the positions equal the torch top-%d" % (100 * same, k))
  assert same >= 0.9


def test_ties_go_to_the_lower_id(als_fit):
  """Two items with the same row and bias score the same bits: the lower id comes first."""
  from recoder_amd.data import UsersInteractions
  rec, m = als_fit
  x, _ = _unseen(m)
  _, Y, b = _tables(rec)
  keep = Y[11].clone(), b[11].clone()
  x = x.tolil()
  x[:, 10] = 0
  x[:, 11] = 0
  x = x.tocsr()
  try:
    Y[11], b[11] = Y[10], b[10]
    lists = rec.recommend_folded(UsersInteractions(np.arange(20), x), 150, alpha=10.0, reg=ALS_REG)
  finally:
    Y[11], b[11] = keep
    rec._sync_ranges()
  checked = 0
  for row in lists:
    pos = {int(i): p for p, i in enumerate(row)}
    if 10 in pos and pos[10] < len(row) - 1:
      assert pos.get(11) == pos[10] + 1
      checked += 1
    if 11 in pos:
      assert pos.get(10) == pos[11] - 1
  assert checked >= 10                                       # (150 of some 180 unseen items: most rows hold the pair)


def test_foldin_recommender_under_the_evaluator(als_fit):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import Recall, RecommenderEvaluator
  from recoder_amd.recommender import FoldInRecommender
  rec, m = als_fit
  x, y = _unseen(m, n=50, seed=12)
  recommender = FoldInRecommender(rec, 20, alpha=10.0, reg=ALS_REG)
  metric = Recall(k=20, normalize=True)
  torch.manual_seed(5)                                       # (the evaluator walks a random order drawn from torch's
  host = RecommenderEvaluator(recommender, [metric]).evaluate(RecommendationDataset(x, y), batch_size=25)
  torch.manual_seed(5)                                       #  global generator: the same order for both)
  dev = RecommenderEvaluator(recommender, [metric]).evaluate(RecommendationDataset(x, y), batch_size=25, on_device=True)
  a, d = np.asarray(host[metric], np.float64), np.asarray(dev[metric], np.float64)
  assert a.shape == d.shape == (50,) and np.array_equal(a, d, equal_nan=True)
  assert np.nanmean(a) > 0
  inp_lists = recommender.recommend(type("B", (), {"users": np.arange(50), "interactions_matrix": x})())
  assert isinstance(inp_lists, list) and len(inp_lists) == 50 and len(inp_lists[0]) == 20


def test_fold_in_leaves_the_serving_path_as_it_was(als_fit):
  from recoder_amd.data import UsersInteractions
  rec, m = als_fit
  users = np.arange(100)
  inp = UsersInteractions(users, m[users])
  tables = [t.clone() for t in _tables(rec)]
  before = rec.recommend_array(inp, 20)
  rec.fold_in(_unseen(m)[0], alpha=3.0, reg=1.0)
  rec.recommend_folded(UsersInteractions(np.arange(20), _unseen(m)[0]), 5)
  after = rec.recommend_array(inp, 20)
  assert np.array_equal(before, after)
  for t, t0 in zip(_tables(rec), tables):
    assert torch.equal(t, t0)


def test_fold_in_warns_once_with_the_count_of_failed_rows():
  """reg = 0 on an item table of duplicate rows: every system is singular; the rows are zero and one warning says so."""
  rec = _recoder(4)
  from recoder_amd.data import RecommendationDataset
  m = sp.csr_matrix(np.eye(6, 8, dtype=np.float32))
  rec.train_als(RecommendationDataset(m), num_iterations=1)
  _, Y, b = _tables(rec)
  Y[:] = 0                                                   # G = 4 y y^T, exact: the second pivot is 16 - 4 * 4
  Y[:4] = torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV)
  hist = sp.csr_matrix((3, 8), dtype=np.float32)
  with pytest.warns(RuntimeWarning, match="3 of 3 rows") as rec_w:
    out = rec.fold_in(hist, alpha=1.0, reg=0.0)
  assert len(rec_w) == 1 and not out.any()
