"""GPU: ItemKNN (recoder_amd/itemknn.py, rk_rp3_item_fit of librecoder_rp3.so, ItemNeighbourhoodModel) against the
restatements of tests/itemknn_util.py -- the fit bit for bit against the f32 chains (ids, weights, counts; every
similarity; with and without values; both accumulator forms; column ranges), which way round a non-symmetric
similarity is stored, the argument checks, and a fit on the ML-20M slice through ``Recoder.train_itemknn`` with
what the fitted model plugs into (recommend, evaluate, checkpoints, predict).

The kernel tests hand rk_rp3_item_fit the comparator's OWN f32 values and vectors (float64, rounded once), as
tests/test_rp3.py does: what is compared is the kernel's arithmetic.  The driver's vectors are checked against
hand-computed ones in tests/test_itemknn_host.py, and end to end here on the slice, whose values are all 1.0 (the
sums of squares are exact counts).

The scores of the end-to-end lists: ``slim_util.scores_f32`` does [users, n] work per neighbour slot, minutes on
the slice at 200 neighbours, so every user's list is checked against ``itemknn_util.scores_binary_f32`` (the
same ascending chain, which for x = 1 is a chain of f32 adds), and that function against ``slim_util.scores_f32``
bit for bit on the first users."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import itemknn_util as iu
from tests import rp3_util, slim_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = (1, 5, 64, 100)
# name -> (similarity, feature weighting, shrink, (asymmetric alpha, tversky alpha, tversky beta), integer values 1..5)
COMBOS = {
    "cosine-0": ("cosine", "none", 0.0, (), False),
    "cosine-10": ("cosine", "none", 10.0, (), False),
    "cosine-bm25": ("cosine", "bm25", 10.0, (), True),
    "asymmetric-0.3": ("asymmetric", "none", 10.0, (0.3,), False),
    "jaccard-0": ("jaccard", "none", 0.0, (), False),
    "tversky-0.3-0.7": ("tversky", "none", 2.0, (0.5, 0.3, 0.7), False),
}
FILL = (7, 3.0, 9)


def _slice():
  z = np.load(iu.SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def _dev_csr(m):
  from recoder_amd.als import AlsCSR
  return AlsCSR(sp.csr_matrix(m), DEV)


def _assert_bitwise(got, want, what=""):
  for g, t, name in zip(got, want, ("ids", "weights", "counts")):
    assert g.dtype == t.dtype and g.shape == t.shape
    same = g.view(np.uint32) == t.view(np.uint32) if g.dtype == np.float32 else g == t
    assert same.all(), "%s %s: %d entries differ, first at %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])


def _inputs(X, combo):
  """(A32, form, own f32, oth f32, g, shrink, binary) as the kernel is given them: the comparator's own."""
  similarity, weighting, shrink, extra, _ = COMBOS[combo] if isinstance(combo, str) else combo
  A64 = iu.weighted_f64(X, weighting)
  A32 = sp.csr_matrix((A64.data.astype(np.float32), A64.indices, A64.indptr), shape=A64.shape)
  form, own, oth, g, binary = iu.vectors_f64(A32, similarity, *extra)
  binary = binary or bool(np.all(A32.data == 1.0))
  return A32, form, own.astype(np.float32), oth.astype(np.float32), float(np.float32(g)), shrink, binary


def _gpu_fit(inputs, K, ranges=None, fill=None):
  """(ids, w, count) as numpy from rk_rp3_item_fit over ``ranges`` (default: one call over every column)."""
  from recoder_amd import als, itemknn
  A, form, own, oth, g, shrink, binary = inputs
  n = A.shape[1]
  uc, ic = als.csr_pair(A, A.shape[0], n, DEV)
  ud = td = None
  if not binary:
    At = A.T.tocsr()
    At.sort_indices()
    ud, td = torch.from_numpy(A.data.copy()).to(DEV), torch.from_numpy(At.data.copy()).to(DEV)
  fi, fw, fc = fill if fill is not None else (0, 0.0, 0)
  ids = torch.full((n, K), fi, dtype=torch.int32, device=DEV)
  w = torch.full((n, K), fw, dtype=torch.float32, device=DEV)
  count = torch.full((n,), fc, dtype=torch.int32, device=DEV)
  own, oth = torch.from_numpy(own).to(DEV), torch.from_numpy(oth).to(DEV)
  for lo, hi in (ranges if ranges is not None else [(0, n)]):
    itemknn.fit_columns(uc, ic, ud, td, own, oth, form, g, shrink, ids, w, count, lo, hi)
  return ids.cpu().numpy(), w.cpu().numpy(), count.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _matrix(n, values):
  """The random graphs of tests/test_rp3.py: empty users, one item nobody holds and one every other user holds
  (n > 1); ``values``: integer values 1..5 instead of 1.0."""
  users = {1: 50, 37: 300, 41: 12, 7915: 3000}[n]
  dens = {1: 0.5, 37: 0.2, 41: 0.3, 7915: 0.004}[n]
  full, none = (n // 3, n // 2) if n > 1 else (None, None)
  if n == 41:
    full = None          # (few users and no common hub: most pairs share one user, so whole groups of sims tie)
  X = rp3_util.graph_matrix(users, n, dens, seed=n + 3, empty=(0, users // 2), full=full, none=none)
  if values:
    X.data = np.random.RandomState(n).randint(1, 6, X.nnz).astype(np.float32)
  return X


@functools.lru_cache(maxsize=None)
def _case(n, combo):
  return _inputs(_matrix(n, COMBOS[combo][4]), combo)


@functools.lru_cache(maxsize=None)
def _ranked(n, combo):
  A, form, own, oth, g, shrink, binary = _case(n, combo)
  return iu.ranked_f32(A, form, own, oth, g, shrink, max(KS), binary)


# ----------------------------------------------------------------------- fit
CASES = [(37, c) for c in COMBOS] + [(n, c) for n in (1, 41, 7915) for c in ("cosine-10", "jaccard-0")]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n, combo", CASES)
def test_fit_is_the_f32_restatement_bit_for_bit(n, combo, K):
  inputs = _case(n, combo)
  assert inputs[6] == (combo != "cosine-bm25"), "only the weighted case takes the values path"
  want = iu.cut_ranked(_ranked(n, combo), K)
  got = _gpu_fit(inputs, K, fill=FILL)
  _assert_bitwise(got, want, "n=%d %s K=%d" % (n, combo, K))
  ids, w, count = got
  live = np.arange(K)[None, :] < count[:, None]
  assert np.all(ids[~live] == -1) and np.all(w[~live].view(np.uint32) == 0), "padding must be -1 / +0"
  assert np.all(np.diff(ids.astype(np.int64), axis=1)[live[:, 1:]] > 0), "ids ascending inside a column"
  assert np.all(ids[live] != np.nonzero(live)[0]), "the diagonal is never kept"
  assert np.all(w[live] > 0)
  if n > 1:
    assert count[n // 2] == 0 and not np.any(ids[live] == n // 2), "an item nobody holds is nobody's neighbour"
    assert count.max() == min(K, int(max(len(c[0]) for c in _ranked(n, combo))))
  else:
    assert count[0] == 0
  if n == 41 and K == 5:
    # columns whose K-th value also occurs among the entries that were cut: the rule (lower ids win) at work
    tied = sum(1 for top, sim in _ranked(n, combo) if len(sim) > K and sim[K] == sim[K - 1])
    print("n=41 %s: columns whose K-th value is tied across the boundary: %d" % (combo, tied))
    assert tied >= 5


def test_fit_workspace_form_bit_for_bit():
  """n above rk_rp3_lds_items(): the accumulators and the candidate lists live in the workspace, a column's
  first touch is read from the -0 fill; with values (fmaf chains) and without (jaccard)."""
  from recoder_amd import itemknn
  n = itemknn.LDS_ITEMS + 5
  users, per, K = 300, 40, 16
  rng = np.random.RandomState(11)
  rows = np.repeat(np.arange(users), per)
  cols = np.concatenate([rng.choice(n, per, replace=False) for _ in range(users)])
  cols[rows % 4 == 1] %= 500                 # (a dense corner: columns with far more than K candidates)
  X = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(users, n))
  X.sum_duplicates()
  X.data[:] = 1.0
  X = X.tolil()
  X[7, :] = 0                                # an empty user
  X[:, 64] = 1                               # an item every other user holds
  X[7, 64] = 0
  X[:, n - 1] = 0
  X[3, n - 1] = 1                            # the last column, past the last full granule of 64
  X = X.tocsr()
  X.eliminate_zeros()
  X.sort_indices()
  V = X.copy()
  V.data = rng.randint(1, 6, X.nnz).astype(np.float32)
  for M, combo in ((V, ("cosine", "none", 10.0, (), True)), (X, ("jaccard", "none", 0.0, (), False))):
    inputs = _inputs(M, combo)
    assert inputs[6] == (combo[0] == "jaccard")
    want = iu.fit_f32(*inputs[:6], K, inputs[6])          # (column by column: no n x n array)
    assert (want[2] == K).sum() > 100 and (want[2] == 0).sum() > 100 and want[2][n - 1] > 0
    got = _gpu_fit(inputs, K, fill=FILL)
    _assert_bitwise(got, want, "workspace form, %s" % combo[0])
    _assert_bitwise(_gpu_fit(inputs, K), got, "workspace form, second call")
    part = _gpu_fit(inputs, K, ranges=[(777, n - 3), (5, 777)], fill=(-7, 9.0, -3))
    _assert_bitwise([a[5:n - 3] for a in part], [a[5:n - 3] for a in got], "workspace form, ranges")
    for a, f in zip(part, (-7, 9.0, -3)):
      assert np.all(a[:5] == f) and np.all(a[n - 3:] == f)


@pytest.mark.parametrize("n, combo", [(37, "cosine-bm25"), (37, "tversky-0.3-0.7"), (7915, "cosine-10")])
def test_column_ranges_give_the_columns_of_the_full_call(n, combo):
  inputs, K = _case(n, combo), 5
  full = _gpu_fit(inputs, K)
  _assert_bitwise(full, iu.cut_ranked(_ranked(n, combo), K), "full call")
  split = _gpu_fit(inputs, K, ranges=[(0, 7), (7, 8), (8, n)], fill=(-7, 9.0, -3))
  _assert_bitwise(split, full, "three ranges")
  back = _gpu_fit(inputs, K, ranges=[(8, n), (7, 8), (0, 7)], fill=(-7, 9.0, -3))
  _assert_bitwise(back, full, "three ranges, in another order")
  for lo, hi in ((0, 7), (7, 8), (8, n)):
    part = _gpu_fit(inputs, K, ranges=[(lo, hi), (hi, hi)], fill=(-7, 9.0, -3))
    _assert_bitwise([t[lo:hi] for t in part], [t[lo:hi] for t in full], "one range")
    for t, f in zip(part, (-7, 9.0, -3)):
      assert np.all(t[:lo] == f) and np.all(t[hi:] == f), "columns outside the range must be left untouched"


def test_a_non_symmetric_similarity_is_the_right_way_round():
  """asymmetric, alpha = 0.3: ``dense_weights()[i, j]`` is sim(i, j) = s / (|a_j|^1.4 |a_i|^0.6 + shrink) of
  float64, not sim(j, i).  The matrix is binary, so s is an exact count in f32 and what separates the two is
  the rounding of the two vectors, of the product, the sum and the quotient: 5 * 2^-24 = 3e-7 < 1e-6."""
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel
  X = _matrix(37, False)
  rec = Recoder(model=ItemNeighbourhoodModel(36, 10.0, "asymmetric", "none", asymmetric_alpha=0.3))
  rec.train_itemknn(RecommendationDataset(X))
  W = rec.model.dense_weights(torch.float64).cpu().numpy()
  A = iu.weighted_f64(X, "none")
  W64 = np.asarray(iu.sims_f64(A, *iu.vectors_f64(A, "asymmetric", 0.3)[:4], 10.0, False).todense())
  assert np.array_equal(W > 0, W64 > 0) and (W64 > 0).sum() > 1000
  live = W64 > 0
  rel = np.abs(W - W64)[live] / W64[live]
  wrong = np.abs(W.T - W64)[live] / W64[live]
  print("asymmetric 0.3: max rel err against sim(i, j) %.3g; against sim(j, i) median %.3g"
        % (rel.max(), np.median(wrong)))
  assert rel.max() <= 1e-6
  assert np.median(wrong) > 1e-3, "the case must tell the two orientations apart"


def test_argument_errors_return_a_message_and_launch_nothing():
  from recoder_amd import _rp3_lib, als
  from recoder_amd._lib import ptr
  lib = _rp3_lib.load()
  A, form, own, oth, g, shrink, _ = _case(37, "cosine-bm25")
  uc, ic = als.csr_pair(A, A.shape[0], 37, DEV)
  K = 5
  ids = torch.full((37, K), 7, dtype=torch.int32, device=DEV)
  w = torch.full((37, K), 3.0, device=DEV)
  count = torch.full((37,), 9, dtype=torch.int32, device=DEV)
  own, oth = torch.from_numpy(own).to(DEV), torch.from_numpy(oth).to(DEV)
  ws = torch.empty(lib.rk_rp3_item_workspace_bytes(37), dtype=torch.uint8, device=DEV)

  def call(t_data=ptr(ic.data), u_data=ptr(uc.data), form=0, g=0.0, shrink=1.0, K=K, lo=0, hi=37, ws_bytes=ws.numel()):
    return lib.rk_rp3_item_fit(ptr(ic.indptr), ptr(ic.indices), t_data, ptr(uc.indptr), ptr(uc.indices), u_data,
                               A.shape[0], 37, ptr(own), ptr(oth), form, g, shrink, K, lo, hi, ptr(ids), ptr(w),
                               ptr(count), ptr(ws), ws_bytes, None)
  assert uc.data is not None and ic.data is not None
  for kw, msg in ((dict(t_data=None), b"t_data and u_data"), (dict(u_data=None), b"t_data and u_data"),
                  (dict(form=2), b"form must be 0"), (dict(form=-1), b"form must be 0"),
                  (dict(shrink=-1.0), b"shrink must be finite and >= 0"),
                  (dict(shrink=float("inf")), b"shrink must be finite and >= 0"),
                  (dict(shrink=float("nan")), b"shrink must be finite and >= 0"),
                  (dict(g=float("nan")), b"g must be finite"), (dict(g=float("-inf")), b"g must be finite"),
                  (dict(K=0), b"K outside"), (dict(K=lib.rk_rp3_max_neighbours() + 1), b"K outside"),
                  (dict(lo=5, hi=4), b"bad column range"), (dict(hi=38), b"bad column range"),
                  (dict(ws_bytes=255), b"workspace too small")):
    assert call(**kw) < 0, kw
    err = lib.rk_rp3_last_error()
    assert err.startswith(b"rk_rp3_item_fit: ") and msg in err, (kw, err)
  torch.cuda.synchronize()
  assert bool((ids == 7).all()) and bool((w == 3.0).all()) and bool((count == 9).all()), "nothing was launched"
  assert call(lo=4, hi=4) == 0                   # (an empty range is no error and no launch)
  torch.cuda.synchronize()
  assert bool((count == 9).all())


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel
  x, y = _slice()
  rec = Recoder(model=ItemNeighbourhoodModel())
  info = rec.train_itemknn(RecommendationDataset(x))
  return rec, info, x, y


@pytest.fixture(scope="module")
def restated():
  """(ids, w, count) of the f32 restatement on the slice at the defaults, and its f32 scores of every user."""
  from recoder_amd.nn import ItemNeighbourhoodModel
  x, _ = _slice()
  p = ItemNeighbourhoodModel().model_params()
  assert np.all(x.data == 1.0)
  inputs = _inputs(x, (p["similarity"], p["feature_weighting"], p["shrink"], (), False))
  model = iu.fit_f32(*inputs[:6], p["neighbours"], inputs[6])
  return model, iu.scores_binary_f32(x, *model)


def _lists(rec, x, k, batch=500):
  from recoder_amd.data import UsersInteractions
  n_users = x.shape[0]
  return np.concatenate([rec.recommend_array(UsersInteractions(np.arange(lo, min(n_users, lo + batch)),
                                                               x[lo:lo + batch]), k)
                         for lo in range(0, n_users, batch)])


def _model_arrays(m):
  return m.item_neighbours.cpu().numpy(), m.item_weights.data.cpu().numpy(), m.neighbour_counts.cpu().numpy()


def test_train_itemknn_info_and_tensors(fitted, restated):
  rec, info, x, _ = fitted
  (ids, w, count), _ = restated
  p = rec.model.model_params()
  assert sorted(info) == ["feature_weighting", "fit_ms", "kept", "n", "neighbours", "nnz", "shrink", "similarity"]
  assert info["n"] == x.shape[1] and info["nnz"] == x.nnz
  assert all(info[k] == p[k] for k in ("neighbours", "shrink", "similarity", "feature_weighting"))
  assert info["kept"] == int(count.astype(np.int64).sum()) and info["fit_ms"] > 0
  print("ItemKNN fit on the slice: %.2f ms, %d entries kept" % (info["fit_ms"], info["kept"]))
  _assert_bitwise(_model_arrays(rec.model), (ids, w, count), "slice")
  assert rec.itemknn_info["kept"] == info["kept"]


def test_every_top20_list_is_the_restated_one(fitted, restated):
  rec, _, x, _ = fitted
  model, S32 = restated
  first = slim_util.scores_f32(x[:24], *model)
  assert np.array_equal(first.view(np.uint32), S32[:24].view(np.uint32)) and (first != 0).mean() > 0.05
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


def test_metrics_on_the_slice_match_float64_and_beat_popularity(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  rec, _, x, y = fitted
  p = rec.model.model_params()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  W64 = iu.fit_f64(x, p["neighbours"], p["shrink"], p["similarity"], p["feature_weighting"])
  want_r, want_n = iu.quality(x, y, W64)
  pop_r, = rp3_util.metric_means(iu.popularity_lists(x, 20), y, ks=((20, "recall"),))
  print("slice %s / %s, shrink %g, K=%d: Recall@20 gpu %.6f f64 %.6f popularity %.6f; NDCG@100 gpu %.6f f64 %.6f"
        % (p["similarity"], p["feature_weighting"], p["shrink"], p["neighbours"], got[str(Recall(k=20))], want_r,
           pop_r, got[str(NDCG(k=100))], want_n))
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


def test_checkpoint_round_trip(fitted, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "itemknn"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == rec.model.model_params() == ItemNeighbourhoodModel().model_params()
  assert sorted(st["model"]) == ["item_neighbours", "item_weights", "neighbour_counts"]
  rec2 = Recoder(model=ItemNeighbourhoodModel(7, 1.0, "dice"))
  rec2.init_from_model_file(f)
  assert rec2.model.model_params() == rec.model.model_params()
  for name in ("item_neighbours", "item_weights", "neighbour_counts"):
    assert torch.equal(getattr(rec2.model, name), getattr(rec.model, name))
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))


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


def test_predict_and_forward_equal_the_scores_kernel(fitted):
  from recoder_amd import itemknn
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  m = rec.model
  users = np.arange(64)
  out, _ = rec.predict(UsersInteractions(users, x[users]))
  want = itemknn.scores(_dev_csr(x[users]), m.item_neighbours, m.item_weights.data, m.neighbour_counts)
  assert out.shape == want.shape and torch.equal(out, want) and bool((want != 0).any())
  dense = torch.from_numpy(np.asarray(x[users].todense(), np.float32)).to(DEV)
  assert torch.equal(m(dense), want)
  tt = torch.tensor([5, 3, 700, 11], device=DEV)
  ii = torch.arange(0, x.shape[1], 2, device=DEV)
  sub = m(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  ref = m.torch_forward(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  assert sub.shape == (64, 4)
  assert torch.allclose(sub, ref, rtol=0, atol=1e-5 * float(ref.abs().max()))


def test_explicit_values_fit_and_serve_and_a_refit_reshapes(tmp_path):
  """Through the driver, with stored values 1..5 and tfidf: the driver's weighted values are the comparator's bit
  for bit, its two vectors (float64 sums of squares in another order) within one f32 ulp, and the fitted tensors
  the f32 restatement of the driver's own inputs bit for bit."""
  from recoder_amd import als, itemknn
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel
  X = rp3_util.graph_matrix(80, 70, 0.2, seed=3)
  X.data = np.random.RandomState(9).randint(1, 6, X.nnz).astype(np.float32)
  ds = RecommendationDataset(X)
  rec = Recoder(model=ItemNeighbourhoodModel())
  info = rec.train_itemknn(ds, neighbours=6, shrink=2.0, similarity="asymmetric", feature_weighting="tfidf")
  want_p = dict(ItemNeighbourhoodModel().model_params(), neighbours=6, shrink=2.0, similarity="asymmetric",
                feature_weighting="tfidf")
  assert rec.model.model_params() == want_p
  assert (info["neighbours"], info["shrink"], info["similarity"], info["feature_weighting"]) == \
      (6, 2.0, "asymmetric", "tfidf")
  assert tuple(rec.model.item_weights.shape) == tuple(rec.model.item_neighbours.shape) == (70, 6)

  def restate(K):
    ud, td, form, own, oth, g = itemknn.host_inputs(als.csr_pair(X, 80, 70, DEV), "asymmetric", "tfidf", 0.5)
    A64 = iu.weighted_f64(X, "tfidf")
    assert np.array_equal(ud, A64.data.astype(np.float32))
    A32 = sp.csr_matrix((ud, X.indices, X.indptr), shape=X.shape)
    At = A32.T.tocsr()
    At.sort_indices()
    assert np.array_equal(td, At.data)
    ref = iu.vectors_f64(A32, "asymmetric", 0.5)
    assert form == ref[0] == 0 and np.allclose(own, ref[1], rtol=2.0 ** -23, atol=0)
    assert np.allclose(oth, ref[2], rtol=2.0 ** -23, atol=0)
    return iu.fit_f32(A32, form, own, oth, g, 2.0, K, False)
  _assert_bitwise(_model_arrays(rec.model), restate(6), "explicit values")
  assert int(rec.model.neighbour_counts.sum()) > 200
  lists = rec.recommend_array(UsersInteractions(np.arange(80), X), 10)
  S = slim_util.scores_f32(X, *_model_arrays(rec.model))
  assert np.array_equal(lists, rp3_util.top_k(S, X, 10))
  info = rec.train_itemknn(ds, neighbours=9)       # (the other settings: the model's, i.e. the ones just stored)
  assert rec.model.model_params() == dict(want_p, neighbours=9)
  assert tuple(rec.model.item_weights.shape) == tuple(rec.model.item_neighbours.shape) == (70, 9)
  _assert_bitwise(_model_arrays(rec.model), restate(9), "refit with another K")
  st = torch.load(rec.save_state(str(tmp_path / "itemknn")), map_location="cpu", weights_only=False)
  assert tuple(st["model"]["item_weights"].shape) == (70, 9) and st["model_params"]["neighbours"] == 9
  with pytest.raises(ValueError, match="train_itemknn"):
    rec.train(ds)
  bad = X.copy()
  bad.data[0] = -1.0
  with pytest.raises(ValueError, match="finite interaction values >= 0"):
    rec.train_itemknn(RecommendationDataset(bad))
