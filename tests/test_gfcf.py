"""GPU: GF-CF (recoder_amd/gfcf.py, rk_ease_lowrank_add in librecoder_ease.so, GraphFilterModel) against the
float64 restatement of tests/gfcf_util.py -- the rank-k update kernel, a fit on small graphs, the subspace the
randomized SVD finds on a matrix with a clear gap, and on the ML-20M slice what the fitted model plugs into
(predict, evaluate, checkpoints).

Tolerances.  The kernel: ``gfcf_util.lowrank_bound`` (derived there: k + 3 roundings, doubled).  A fit adds
``gfcf_util.gram_bound`` for the Gram's chain.  The subspace statistic max|V V^T - V64 V64^T| may be M_SUB = 4
times that of the float32 numpy restatement of the same randomized SVD with the same Omega: the margin the
EASE inverse tests give f32 LAPACK.  Measured on an MI355X: DESIGN section 4, "GF-CF".  The quality margin is
twice the five-seed spread of the float64 randomized restatement's Recall@20 on the slice, measured on the CPU:
the ``gfcf_quality_spread`` record of profiles/gfcf_quality.jsonl (tools/gfcf_bench.py --cpu-grid)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import gfcf_util as gu, rp3_util, svd_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
M_SUB = 4.0
# profiles/gfcf_quality.jsonl, record "gfcf_quality_spread" (rank 128, alpha 3, q = 6, seeds 0..4): the exact
# eigenvectors give Recall@20 0.141444, the five randomized draws 0.138621 .. 0.141485
EXACT_RECALL20, SEED_SPREAD = 0.141444, 0.002864
QUALITY_MARGIN = 2 * SEED_SPREAD


def _t(a):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _pair(m):
  from recoder_amd import als
  return als.csr_pair(m, m.shape[0], m.shape[1], DEV)


# -------------------------------------------------------------------- kernel
def _problem(n, k, seed=0):
  """Random A, V and scales with some scales exactly 0 (f32 values, so the float64 reference sees the same
  inputs)."""
  rng = np.random.RandomState(1000 * n + k + seed)
  A = rng.randn(n, n).astype(np.float32)
  V = rng.randn(n, k).astype(np.float32)
  a = (rng.rand(n) + 0.5).astype(np.float32) * rng.choice([-1.0, 1.0], n).astype(np.float32)
  b = (rng.rand(n) + 0.5).astype(np.float32)
  a[rng.rand(n) < 0.15] = 0.0
  b[rng.rand(n) < 0.15] = 0.0
  if n > 2:
    a[1], b[2] = 0.0, 0.0
  return A, V, a, b


def _run(A, V, a, b, alpha, lda=None, ldv=None, ranges=None, pad=-7.0):
  """The kernel on device copies with the given leading dimensions; returns the whole [n, lda] buffer."""
  from recoder_amd import gfcf
  n, k = V.shape
  lda, ldv = lda or n, ldv or k
  Ab = torch.full((n, lda), pad, device=DEV)
  Ab[:, :n] = _t(A)
  Vb = torch.full((n, ldv), 3.0, device=DEV)      # (the padding of V must not be read)
  Vb[:, :k] = _t(V)
  for lo, hi in (ranges or [(0, n)]):
    gfcf.lowrank_add(Ab[:, :n], Vb[:, :k], _t(a), _t(b), alpha, lo, hi)
  return Ab.cpu().numpy()


@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 256])
@pytest.mark.parametrize("n", [1, 31, 127, 128, 129, 257])
def test_lowrank_add_against_float64(n, k):
  A, V, a, b = _problem(n, k)
  alpha = 0.7
  lda = n + 3 if n in (31, 129, 257) else n
  ldv = k + 5 if k in (3, 65, 256) else k
  got = _run(A, V, a, b, alpha, lda, ldv)
  A64, V64 = A.astype(np.float64), V.astype(np.float64)
  want = A64 + alpha * a.astype(np.float64)[:, None] * (V64 @ V64.T) * b.astype(np.float64)[None, :]
  bound = gu.lowrank_bound(A, V, a, b, alpha)
  err = np.abs(got[:, :n] - want)
  print("lowrank_add n=%d k=%d: max err / bound = %.3g" % (n, k, float((err / bound).max())))
  assert np.all(err <= bound)
  assert np.all(got[:, n:] == -7.0), "columns at or past n were touched"
  # a zero scale adds nothing: the row / column keeps its bits
  zr, zc = a == 0, b == 0
  assert np.array_equal(got[:, :n][zr], A[zr]) and np.array_equal(got[:, :n][:, zc], A[:, zc])


def test_lowrank_add_is_bitwise_repeatable_and_splits_by_rows():
  n, k = 129, 65
  A, V, a, b = _problem(n, k, seed=1)
  full = _run(A, V, a, b, -1.3, lda=n + 3, ldv=k + 5)
  again = _run(A, V, a, b, -1.3, lda=n + 3, ldv=k + 5)
  assert np.array_equal(full.view(np.uint32), again.view(np.uint32))
  parts = _run(A, V, a, b, -1.3, lda=n + 3, ldv=k + 5, ranges=[(0, 40), (40, 129)])
  assert np.array_equal(parts.view(np.uint32), full.view(np.uint32))
  # the leading dimensions play no part in the values
  plain = _run(A, V, a, b, -1.3)
  assert np.array_equal(plain.view(np.uint32), full[:, :n].view(np.uint32))
  # a range leaves the rows outside it alone
  some = _run(A, V, a, b, -1.3, ranges=[(40, 41)])
  assert np.array_equal(some[40].view(np.uint32), plain[40].view(np.uint32))
  assert np.array_equal(np.delete(some, 40, 0), np.delete(A, 40, 0))
  # sentinels in the padding columns survive, NaN included
  nan = _run(A, V, a, b, -1.3, lda=n + 3, pad=float("nan"))
  assert np.isnan(nan[:, n:]).all() and np.array_equal(nan[:, :n].view(np.uint32), plain.view(np.uint32))


def test_alpha_zero_leaves_the_matrix_as_it_is():
  A, V, a, b = _problem(129, 64, seed=2)
  assert np.array_equal(_run(A, V, a, b, 0.0), A)


def test_lowrank_add_is_not_symmetric_in_its_scales():
  """An asymmetric case with integer data, exact in f32: rows scale by a, columns by b, not the reverse."""
  n, k = 70, 3
  rng = np.random.RandomState(3)
  V = rng.randint(-3, 4, (n, k)).astype(np.float32)
  a = rng.randint(1, 5, n).astype(np.float32)
  b = rng.randint(1, 9, n).astype(np.float32) * 0.5
  A = rng.randint(-9, 10, (n, n)).astype(np.float32)
  want = A + 2.0 * a[:, None] * (V @ V.T) * b[None, :]
  assert np.array_equal(_run(A, V, a, b, 2.0), want)


# ----------------------------------------------------------------------- fit
@pytest.mark.parametrize("seed,alpha", [(1, 0.3), (2, 3.0)])
def test_fit_on_a_small_graph(seed, alpha):
  from recoder_amd import gfcf
  X = rp3_util.graph_matrix(60, 40, 0.15, seed, empty=(0,), full=3, none=7)
  W, info = gfcf.fit(_pair(X), 8, alpha, oversample=16, num_power_iterations=6, omega=svd_util.omega(40, 24, seed))
  assert (info["n"], info["nnz"], info["rank"], info["alpha"], info["l"]) == (40, X.nnz, 8, alpha, 24)
  assert all(info[k] > 0 for k in ("gram_ms", "svd_ms", "filter_ms")) and len(info["singular_values"]) == 8
  assert abs(info["singular_values"][0] - 1.0) <= 1e-5          # (sigma_1 of a normalised graph is 1)
  V = info["V"].cpu().numpy()
  W = W.cpu().numpy()
  want = gu.weights_f64(X, 8, alpha, V=V)
  _, di, dh = gu.scales_f64(X)
  bound = gu.lowrank_bound(gu.gram_f64(X), V, di, dh, alpha) + gu.gram_bound(X)
  err = np.abs(W - want)
  live = bound > 0
  print("fit seed=%d: max err / bound = %.3g" % (seed, float((err[live] / bound[live]).max())))
  assert np.all(err <= bound)
  # the item nobody holds: an exact zero row and column (and a zero row of V)
  assert not W[7].any() and not W[:, 7].any() and not V[7].any()
  assert W[3, 5] != W[5, 3], "W is not symmetric"
  # the stored values play no part in the fit
  Xv = X.copy()
  Xv.data[:] = np.random.RandomState(0).rand(X.nnz).astype(np.float32) + 0.5
  W2, _ = gfcf.fit(_pair(Xv), 8, alpha, oversample=16, num_power_iterations=6, omega=svd_util.omega(40, 24, seed))
  assert np.array_equal(W2.cpu().numpy(), W)


def test_subspace_on_a_matrix_with_a_gap():
  from recoder_amd import gfcf
  X = svd_util.planted()
  sigma, E = gu.top_eigenvectors(gu.gram_f64(X), 9)
  assert sigma[7] > 0.7 and sigma[8] < 0.3, "the planted matrix no longer separates sigma_8 from sigma_9"
  P64 = E[:, :8] @ E[:, :8].T
  om = svd_util.omega(X.shape[1], 24, 5)
  _, info = gfcf.fit(_pair(X), 8, 1.0, oversample=16, num_power_iterations=6, omega=om)
  V = info["V"].cpu().numpy().astype(np.float64)
  V32 = svd_util.rsvd(gu.normalised(X), 8, 16, 6, om, np.float32)[1].astype(np.float64)
  got, ref = np.abs(V @ V.T - P64).max(), np.abs(V32 @ V32.T - P64).max()
  print("subspace: max|VV^T - V64V64^T| gpu %.3g, float32 restatement %.3g, ratio %.2f" % (got, ref, got / ref))
  assert got <= M_SUB * ref
  assert np.abs(np.asarray(info["singular_values"]) - sigma[:8]).max() <= 1e-5


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  x, y = gu.load_slice()
  rec = Recoder(model=GraphFilterModel())
  info = rec.train_gfcf(RecommendationDataset(x))
  return rec, info, x, y


def test_train_gfcf_info(fitted):
  rec, info, x, _ = fitted
  assert (info["n"], info["nnz"], info["rank"], info["alpha"], info["l"]) == (x.shape[1], x.nnz, 128, 3.0, 144)
  assert all(info[k] > 0 for k in ("gram_ms", "svd_ms", "filter_ms")) and "V" not in info
  assert rec.gfcf_info["V"].shape == (x.shape[1], 128) and rec.gfcf_info["V"].is_cuda
  assert rec.model.model_params() == {"rank": 128, "alpha": 3.0}
  print("GF-CF fit on the slice: gram %.2f ms, svd %.2f ms, filter %.3f ms, ritz residual %.3g"
        % (info["gram_ms"], info["svd_ms"], info["filter_ms"], info["ritz_residual"]))


def test_predict_stays_within_the_f32_bound_of_float64(fitted):
  """|score - score64| <= sum_j |x_uj| bound_W[j, i] + d_u 2^-23 sum_j |x_uj W_ji|: the weights' bound (kernel +
  Gram) carried through the product, plus the scores' own fmaf chain over the user's d_u entries (d_u
  roundings of 2^-24, doubled as everywhere here), W64 built from the device's V."""
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  V = rec.gfcf_info["V"].cpu().numpy()
  W64 = gu.weights_f64(x, 128, 3.0, V=V)
  _, di, dh = gu.scales_f64(x)
  bw = gu.lowrank_bound(gu.gram_f64(x), V, di, dh, 3.0) + gu.gram_bound(x)
  users = np.arange(500)
  out, _ = rec.predict(UsersInteractions(users, x[users]))
  got = out.cpu().numpy().astype(np.float64)
  xs = abs(x[users]).astype(np.float64)
  want = np.asarray(x[users].astype(np.float64) @ W64)
  d = np.diff(x[users].indptr)[:, None]
  bound = np.asarray(xs @ bw) + d * 2.0 ** -23 * np.asarray(xs @ np.abs(W64))
  err = np.abs(got - want)
  print("predict: max err / bound = %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
  assert got.shape == want.shape and np.all(err <= bound)


def test_recall_on_the_slice(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  rec, _, x, y = fitted
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  print("slice rank=128 alpha=3: Recall@20 gpu %.6f (float64, exact eigenvectors %.6f); NDCG@100 gpu %.6f"
        % (got[str(Recall(k=20))], EXACT_RECALL20, got[str(NDCG(k=100))]))
  assert got[str(Recall(k=20))] >= EXACT_RECALL20 - QUALITY_MARGIN


def test_checkpoint_round_trip(fitted, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "gfcf"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == {"rank": 128, "alpha": 3.0} and list(st["model"]) == ["item_weights"]
  rec2 = Recoder(model=GraphFilterModel(rank=3, alpha=0.1))
  rec2.init_from_model_file(f)
  assert (rec2.model.rank, rec2.model.alpha) == (128, 3.0)
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))
  assert torch.equal(rec.model.item_weights.data, rec2.model.item_weights.data)


def test_inference_recommender_serves_the_model(fitted):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.recommender import InferenceRecommender
  rec, _, x, _ = fitted
  inp = UsersInteractions(np.arange(50), x[:50])
  lists = InferenceRecommender(rec, 20).recommend(inp)
  want = rec.recommend(inp, 20)
  assert len(lists) == 50 and all(list(a) == list(b) for a, b in zip(lists, want))
  for u in range(50):
    assert not np.isin(want[u], x[u].indices).any()


def test_explicit_rank_and_alpha_are_stored_and_a_refit_reuses_the_buffer():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  X = rp3_util.graph_matrix(80, 60, 0.2, 4, empty=(0,), full=3, none=7)
  rec = Recoder(model=GraphFilterModel())
  info = rec.train_gfcf(RecommendationDataset(X), rank=8, alpha=0.5)
  assert (rec.model.rank, rec.model.alpha, info["rank"], info["alpha"]) == (8, 0.5, 8, 0.5)
  assert rec.model.model_params() == {"rank": 8, "alpha": 0.5}
  where = rec.model.item_weights.data_ptr()
  W8 = rec.model.item_weights.data.clone()
  info = rec.train_gfcf(RecommendationDataset(X), rank=12)
  assert (rec.model.rank, rec.model.alpha, info["rank"], info["l"]) == (12, 0.5, 12, 28)
  assert rec.model.item_weights.data_ptr() == where and rec.gfcf_info["V"].shape == (60, 12)
  W12 = rec.model.item_weights.data.cpu().numpy()
  assert not np.array_equal(W12, W8.cpu().numpy())
  V = rec.gfcf_info["V"].cpu().numpy()
  _, di, dh = gu.scales_f64(X)
  bound = gu.lowrank_bound(gu.gram_f64(X), V, di, dh, 0.5) + gu.gram_bound(X)
  assert np.all(np.abs(W12 - gu.weights_f64(X, 12, 0.5, V=V)) <= bound)
  # the same seed gives the same bits
  rec.train_gfcf(RecommendationDataset(X))
  assert np.array_equal(rec.model.item_weights.data.cpu().numpy(), W12)
  with pytest.raises(ValueError, match="train_gfcf"):
    rec.train(RecommendationDataset(X))
