"""GPU: RP3beta (recoder_amd/rp3.py, librecoder_rp3.so, RandomWalkItemModel) against the restatements of
tests/rp3_util.py -- the fit bit for bit against the f32 chains (ids, weights, counts; both accumulator
paths; row ranges), the scores bit for bit against the fmaf chain, a fit on the ML-20M slice through
``Recoder.train_rp3beta`` and what the fitted model plugs into (recommend, evaluate, checkpoints, predict).

The float64 bound of a kept weight: rk_rp3_fit takes its three weight vectors as f32 INPUTS, so the float64
comparator uses the same three vectors (exact in float64).  What the kernel adds is m - 1 f32 additions
of positive terms (m: the users the pair shares) and two f32 multiplies, each within 2^-24 relative:
at most (m + 1) 2^-24 to first order, asserted as (m + 2) 2^-24.  (The vectors themselves are checked
against float64 powers in tests/test_rp3_host.py.)"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import ease_util, rp3_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALPHA, BETA, K_DEFAULT = 0.6, 0.3, 100


def _slice():
  z = np.load(rp3_util.SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def _pair(m):
  from recoder_amd import als
  return als.csr_pair(m, m.shape[0], m.shape[1], DEV)


def _dev_csr(m):
  from recoder_amd.als import AlsCSR
  return AlsCSR(sp.csr_matrix(m), DEV)


def _weights32(X, alpha=ALPHA, beta=BETA):
  """The three vectors as the fit is given them: float64 powers rounded once (the comparator's own)."""
  return tuple(a.astype(np.float32) for a in rp3_util.weights_f64(X, alpha, beta))


def _gpu_fit(X, wts, K, ranges=None, fill=None):
  """(ids, w, count) as numpy from rk_rp3_fit over ``ranges`` (default: one call over every row)."""
  from recoder_amd import rp3
  uc, ic = _pair(X)
  n = X.shape[1]
  uw, rs, cs = (torch.from_numpy(a).to(DEV) for a in wts)
  fi, fw, fc = fill if fill is not None else (0, 0.0, 0)
  ids = torch.full((n, K), fi, dtype=torch.int32, device=DEV)
  w = torch.full((n, K), fw, dtype=torch.float32, device=DEV)
  count = torch.full((n,), fc, dtype=torch.int32, device=DEV)
  for lo, hi in (ranges if ranges is not None else [(0, n)]):
    rp3.fit_rows(uc, ic, uw, rs, cs, ids, w, count, lo, hi)
  return ids.cpu().numpy(), w.cpu().numpy(), count.cpu().numpy()


def _assert_bitwise(got, want, what=""):
  for g, t, name in zip(got, want, ("ids", "weights", "counts")):
    assert g.dtype == t.dtype and g.shape == t.shape
    same = g.view(np.uint32) == t.view(np.uint32) if g.dtype == np.float32 else g == t
    assert same.all(), "%s %s: %d entries differ, first at %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])


@functools.lru_cache(maxsize=None)
def _case(n):
  """(X, the three f32 vectors) of the random graphs: empty users, one item nobody holds and one every
  other user holds (n > 1)."""
  users = {1: 50, 37: 300, 41: 12, 7915: 3000}[n]
  dens = {1: 0.5, 37: 0.2, 41: 0.3, 7915: 0.004}[n]
  full, none = (n // 3, n // 2) if n > 1 else (None, None)
  if n == 41:
    full = None          # (few users and no common hub: most pairs share one user, so whole groups of W tie)
  X = rp3_util.graph_matrix(users, n, dens, seed=n + 3, empty=(0, users // 2), full=full, none=none)
  return X, _weights32(X)


@functools.lru_cache(maxsize=None)
def _restated(n, K):
  X, wts = _case(n)
  return rp3_util.fit_f32(X, *wts, K)


# ----------------------------------------------------------------------- fit
@pytest.mark.parametrize("n, K", [(1, 1), (37, 5), (37, 64), (41, 5), (7915, 100)])
def test_fit_is_the_f32_restatement_bit_for_bit(n, K):
  X, wts = _case(n)
  want = _restated(n, K)
  got = _gpu_fit(X, wts, K, fill=(7, 3.0, 9))
  _assert_bitwise(got, want, "n=%d K=%d" % (n, K))
  ids, w, count = got
  live = np.arange(K)[None, :] < count[:, None]
  assert np.all(ids[~live] == -1) and np.all(w[~live].view(np.uint32) == 0), "padding must be -1 / +0"
  assert np.all(np.diff(ids.astype(np.int64), axis=1)[live[:, 1:]] > 0), "ids ascending inside a row"
  assert np.all(ids[live] != np.nonzero(live)[0]), "the diagonal is never kept"
  if n > 1:
    assert count[n // 2] == 0, "an item nobody holds has no neighbours"
  if (n, K) == (37, 64):
    assert count.max() < K
  if n in (37, 41) and K == 5:
    # rows whose K-th value also occurs among the entries that were cut: the rule (lower ids win) at work
    _, allw, _ = rp3_util.fit_f32(X, *wts, n)
    tied = sum(1 for i in range(n) if count[i] == K and
               (allw[i] == w[i, :K].min()).sum() > (w[i, :K] == w[i, :K].min()).sum())
    print("n=%d: rows whose K-th value is tied across the boundary: %d" % (n, tied))
    assert n != 41 or tied >= 5
  # against float64 on the same three vectors: (m + 2) 2^-24 relative, m the users the pair shares
  W64 = rp3_util.dense_w_f64(X, *wts)
  B = sp.csr_matrix(X).astype(np.float64)
  C = (B.T @ B).tocsr()
  rows = np.nonzero(live)[0]
  cols = ids[live].astype(np.int64)
  if live.any():
    ref = np.asarray(W64[rows, cols]).ravel()
    m = np.asarray(C[rows, cols]).ravel()
    assert np.all(ref > 0) and np.all(m >= 1)
    rel = np.abs(w[live].astype(np.float64) - ref) / ref
    print("n=%d K=%d: max rel err %.3g, max rel err / ((m + 2) 2^-24) %.3f, max m %d"
          % (n, K, rel.max(), (rel / ((m + 2) * 2.0 ** -24)).max(), m.max()))
    assert np.all(rel <= (m + 2) * 2.0 ** -24)


def test_fit_workspace_path_bit_for_bit():
  """n above rk_rp3_lds_items(): the accumulators and the candidate lists live in the workspace."""
  from recoder_amd import _rp3_lib
  n = _rp3_lib.load().rk_rp3_lds_items() + 1000
  users, per, K = 400, 30, 20
  rng = np.random.RandomState(11)
  rows = np.repeat(np.arange(users), per)
  cols = np.concatenate([rng.choice(n, per, replace=False) for _ in range(users)])
  cols[rows % 4 == 1] %= 500                 # (a dense corner: rows with far more than K candidates)
  X = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(users, n))
  X.sum_duplicates()
  X.data[:] = 1.0
  X = X.tolil()
  X[7, :] = 0                                # an empty user
  X[:, 64] = 1                               # an item every other user holds
  X[7, 64] = 0
  X = X.tocsr()
  X.eliminate_zeros()
  X.sort_indices()
  wts = _weights32(X)
  want = rp3_util.fit_f32(X, *wts, K)          # (row by row: no n x n array)
  assert (want[2] == K).sum() > 100 and (want[2] == 0).sum() > 100
  got = _gpu_fit(X, wts, K, fill=(7, 3.0, 9))
  _assert_bitwise(got, want, "workspace path")
  again = _gpu_fit(X, wts, K)
  _assert_bitwise(again, got, "workspace path, second call")
  part = _gpu_fit(X, wts, K, ranges=[(5, 777), (777, n - 3)], fill=(-7, 9.0, -3))
  _assert_bitwise([a[5:n - 3] for a in part], [a[5:n - 3] for a in got], "workspace path, ranges")
  for a, f in zip(part, (-7, 9.0, -3)):
    assert np.all(a[:5] == f) and np.all(a[n - 3:] == f)


@pytest.mark.parametrize("n, K", [(37, 5), (7915, 100)])
def test_row_ranges_give_the_rows_of_the_full_call(n, K):
  X, wts = _case(n)
  full = _gpu_fit(X, wts, K)
  _assert_bitwise(_gpu_fit(X, wts, K), full, "second call")
  a, b = (3, 20) if n == 37 else (1001, 4097)
  split = _gpu_fit(X, wts, K, ranges=[(b, n), (0, a), (a, b)], fill=(-7, 9.0, -3))
  _assert_bitwise(split, full, "three ranges")
  part = _gpu_fit(X, wts, K, ranges=[(a, b), (b, b)], fill=(-7, 9.0, -3))
  _assert_bitwise([t[a:b] for t in part], [t[a:b] for t in full], "one range")
  for t, f in zip(part, (-7, 9.0, -3)):
    assert np.all(t[:a] == f) and np.all(t[b:] == f), "rows outside the range must be left untouched"


# -------------------------------------------------------------------- scores
def test_scores_are_the_ascending_fmaf_chain():
  from recoder_amd import rp3
  n, K = 7915, 100
  X, _ = _case(n)
  ids, w, count = _restated(n, K)
  tid, tw, tc = (torch.from_numpy(a).to(DEV) for a in (ids, w, count))
  long_row = sp.csr_matrix((np.asarray(X[5:12].sum(0)) > 0).astype(np.float32))      # (more than 64 entries: two fetches)
  plain = sp.vstack([sp.csr_matrix((1, n), dtype=np.float32), long_row, X[5:160]]).tocsr()
  plain.sort_indices()
  assert np.diff(plain.indptr)[0] == 0 and np.diff(plain.indptr)[1] > 64
  sub = plain.copy()
  sub.data = (sub.data * np.random.RandomState(0).choice([1.0, 0.5, 3.0, -2.0], sub.nnz)).astype(np.float32)
  csr = _dev_csr(sub)
  assert csr.data is not None
  got = rp3.scores(csr, tid, tw, tc).cpu().numpy()
  want = rp3_util.scores_f32(sub, ids, w, count)
  assert got.shape == want.shape == (plain.shape[0], n)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  assert np.all(got[0].view(np.uint32) == 0), "an empty user row gives all +0"
  # a strip gives bitwise the columns of the full call, whatever the batch position
  for lo, hi in ((0, 1), (1023, 1025), (37, 7915), (7914, 7915), (n // 3, n // 3 + 1), (4001, 6007)):
    part = rp3.scores(csr, tid, tw, tc, lo, hi).cpu().numpy()
    assert part.shape == (plain.shape[0], hi - lo)
    assert np.array_equal(part.view(np.uint32), got[:, lo:hi].view(np.uint32)), (lo, hi)
  rev = rp3.scores(_dev_csr(sub[::-1]), tid, tw, tc).cpu().numpy()
  assert np.array_equal(rev[::-1].view(np.uint32), got.view(np.uint32))
  # unit values: the NULL data path
  c1 = _dev_csr(plain)
  assert c1.data is None
  assert np.array_equal(rp3.scores(c1, tid, tw, tc).cpu().numpy().view(np.uint32),
                        rp3_util.scores_f32(plain, ids, w, count).view(np.uint32))
  # out with a leading dimension: columns past the strip are left alone
  out = torch.full((plain.shape[0], 2048), 5.0, device=DEV)
  rp3.scores(csr, tid, tw, tc, 10, 2011, out=out)
  out = out.cpu().numpy()
  assert np.array_equal(out[:, :2001].view(np.uint32), got[:, 10:2011].view(np.uint32)) and np.all(out[:, 2001:] == 5.0)


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel
  x, y = _slice()
  rec = Recoder(model=RandomWalkItemModel())
  info = rec.train_rp3beta(RecommendationDataset(x))
  return rec, info, x, y


@pytest.fixture(scope="module")
def restated():
  """(ids, w, count) of the f32 restatement on the slice at the defaults, and its f32 scores of every user."""
  x, _ = _slice()
  model = rp3_util.fit_f32(x, *_weights32(x), K_DEFAULT)
  return model, rp3_util.scores_f32(x, *model)


def _lists(rec, x, k, batch=500):
  from recoder_amd.data import UsersInteractions
  n_users = x.shape[0]
  return np.concatenate([rec.recommend_array(UsersInteractions(np.arange(lo, min(n_users, lo + batch)),
                                                               x[lo:lo + batch]), k)
                         for lo in range(0, n_users, batch)])


def test_train_rp3beta_info_and_tensors(fitted, restated):
  rec, info, x, _ = fitted
  (ids, w, count), _ = restated
  assert sorted(info) == ["alpha", "beta", "fit_ms", "kept", "n", "neighbours", "nnz"]
  assert info["n"] == x.shape[1] and info["nnz"] == x.nnz
  assert (info["alpha"], info["beta"], info["neighbours"]) == (ALPHA, BETA, K_DEFAULT)
  assert info["kept"] == int(count.astype(np.int64).sum()) and info["fit_ms"] > 0
  print("RP3beta fit on the slice: %.2f ms, %d entries kept" % (info["fit_ms"], info["kept"]))
  m = rec.model
  got = (m.item_neighbours.cpu().numpy(), m.item_weights.data.cpu().numpy(), m.neighbour_counts.cpu().numpy())
  _assert_bitwise(got, (ids, w, count), "slice")
  assert rec.rp3_info["kept"] == info["kept"]


def test_every_top20_list_is_the_restated_one(fitted, restated):
  rec, _, x, _ = fitted
  _, S32 = restated
  lists = _lists(rec, x, 20)
  assert lists.shape == (x.shape[0], 20)
  assert lists.min() >= 0 and lists.max() < x.shape[1]
  for u in range(x.shape[0]):
    seen = x.indices[x.indptr[u]:x.indptr[u + 1]]
    assert len(set(lists[u])) == 20 and not np.isin(lists[u], seen).any(), "a seen or repeated item"
  want = rp3_util.top_k(S32.copy(), x, 20)
  same = np.all(lists == want, axis=1)
  assert same.all(), "%d users' lists differ, first user %d" % ((~same).sum(), int(np.argmin(same)))
  rec.eval_strip_items = 1000
  try:
    strips = _lists(rec, x, 20)
  finally:
    del rec.eval_strip_items
  assert np.array_equal(strips, lists)


def test_metrics_on_the_slice_match_float64(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  rec, _, x, y = fitted
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  W64 = rp3_util.fit_f64(x, ALPHA, BETA, K_DEFAULT)
  S64 = np.asarray((x.astype(np.float64) @ W64).todense())
  want_r, want_n = rp3_util.metric_means(rp3_util.top_k(S64, x, 100), y)
  del S64
  pop = np.tile(rp3_util.degrees(x)[1].astype(np.float32), (x.shape[0], 1))
  pop_r, = rp3_util.metric_means(rp3_util.top_k(pop, x, 20), y, ks=((20, "recall"),))
  print("slice alpha=%g beta=%g K=%d: Recall@20 gpu %.6f f64 %.6f popularity %.6f; NDCG@100 gpu %.6f f64 %.6f"
        % (ALPHA, BETA, K_DEFAULT, got[str(Recall(k=20))], want_r, pop_r, got[str(NDCG(k=100))], want_n))
  assert abs(got[str(Recall(k=20))] - want_r) <= 1e-3
  assert abs(got[str(NDCG(k=100))] - want_n) <= 1e-3
  assert got[str(Recall(k=20))] > pop_r


def test_empty_history_gets_k_valid_items(fitted):
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  m = sp.vstack([sp.csr_matrix((1, x.shape[1]), dtype=np.float32), x[:3]]).tocsr()
  got = rec.recommend(UsersInteractions(np.arange(4), m), 20)
  assert len(got) == 4 and len(set(got[0])) == 20 and all(0 <= i < x.shape[1] for i in got[0])
  for u in range(1, 4):
    assert not np.isin(got[u], x[u - 1].indices).any()


# ------------------------------------------------------------------ plumbing
def test_checkpoint_round_trip(fitted, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "rp3"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == {"alpha": ALPHA, "beta": BETA, "neighbours": K_DEFAULT}
  assert sorted(st["model"]) == ["item_neighbours", "item_weights", "neighbour_counts"]
  rec2 = Recoder(model=RandomWalkItemModel(1.0, 0.0, 7))
  rec2.init_from_model_file(f)
  assert rec2.model.model_params() == rec.model.model_params()
  for name in ("item_neighbours", "item_weights", "neighbour_counts"):
    assert torch.equal(getattr(rec2.model, name), getattr(rec.model, name))
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))


def test_explicit_values_are_stored_and_a_refit_reshapes(tmp_path):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel
  X = rp3_util.graph_matrix(80, 70, 0.2, seed=3)
  ds = RecommendationDataset(X)
  rec = Recoder(model=RandomWalkItemModel())
  info = rec.train_rp3beta(ds, alpha=0.9, beta=0.1, neighbours=6)
  assert rec.model.model_params() == {"alpha": 0.9, "beta": 0.1, "neighbours": 6}
  assert (info["alpha"], info["beta"], info["neighbours"]) == (0.9, 0.1, 6)
  assert tuple(rec.model.item_weights.shape) == tuple(rec.model.item_neighbours.shape) == (70, 6)
  want = rp3_util.fit_f32(X, *_weights32(X, 0.9, 0.1), 6)
  m = rec.model
  _assert_bitwise((m.item_neighbours.cpu().numpy(), m.item_weights.data.cpu().numpy(),
                   m.neighbour_counts.cpu().numpy()), want, "explicit values")
  info = rec.train_rp3beta(ds, neighbours=9)       # (alpha and beta: the model's, i.e. the ones just stored)
  assert rec.model.model_params() == {"alpha": 0.9, "beta": 0.1, "neighbours": 9}
  assert tuple(rec.model.item_weights.shape) == tuple(rec.model.item_neighbours.shape) == (70, 9)
  want = rp3_util.fit_f32(X, *_weights32(X, 0.9, 0.1), 9)
  m = rec.model
  _assert_bitwise((m.item_neighbours.cpu().numpy(), m.item_weights.data.cpu().numpy(),
                   m.neighbour_counts.cpu().numpy()), want, "refit with another K")
  st = torch.load(rec.save_state(str(tmp_path / "rp3")), map_location="cpu", weights_only=False)
  assert tuple(st["model"]["item_weights"].shape) == (70, 9)
  with pytest.raises(ValueError, match="train_rp3beta"):
    rec.train(ds)


def test_inference_recommender_gives_the_same_metrics(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall, RecommenderEvaluator
  from recoder_amd.recommender import InferenceRecommender
  rec, _, x, y = fitted
  ds = RecommendationDataset(x[:2000], y[:2000])
  metrics = [Recall(k=20, normalize=True), NDCG(k=100)]
  a = rec.evaluate(ds, num_recommendations=100, metrics=metrics, batch_size=500)
  b = RecommenderEvaluator(InferenceRecommender(rec, 100), metrics).evaluate(ds, batch_size=500)
  for k in a:      # (each evaluation draws its own user order: the per-user values as multisets)
    np.testing.assert_array_equal(np.sort(np.asarray(a[k], np.float64)), np.sort(np.asarray(b[k], np.float64)))
    assert np.isfinite(np.asarray(a[k], np.float64)).sum() > 1000


def test_large_k_agrees_with_the_kernel_path(fitted):
  from recoder_amd import _lib
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  kmax = _lib.load().rk_topk_max_k()
  # (compared up to each user's first tie: torch.topk's order among equal scores is its own)
  inp = UsersInteractions(np.arange(40), x[:40])
  big = rec.recommend_array(inp, kmax + 1)
  assert big.shape == (40, kmax + 1)
  small = rec.recommend_array(inp, kmax)
  out, _ = rec.predict(inp)
  out = out.cpu().numpy()
  uptos = []
  for u in range(40):
    strict = np.diff(out[u, small[u]]) < 0
    upto = len(strict) if strict.all() else int(np.argmin(strict))
    uptos.append(upto)
    assert np.array_equal(big[u, :upto], small[u, :upto])
  assert np.median(uptos) >= 20


def test_predict_and_forward_equal_the_scores_kernel(fitted):
  from recoder_amd import rp3
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  m = rec.model
  users = np.arange(64)
  out, _ = rec.predict(UsersInteractions(users, x[users]))
  want = rp3.scores(_dev_csr(x[users]), m.item_neighbours, m.item_weights.data, m.neighbour_counts)
  assert out.shape == want.shape and torch.equal(out, want)
  dense = torch.from_numpy(np.asarray(x[users].todense(), np.float32)).to(DEV)
  assert torch.equal(m(dense), want)
  tt = torch.tensor([5, 3, 700, 11], device=DEV)
  ii = torch.arange(0, x.shape[1], 2, device=DEV)
  sub = m(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  ref = m.torch_forward(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  assert sub.shape == (64, 4)
  assert torch.allclose(sub, ref, rtol=0, atol=1e-5 * float(ref.abs().max()))
