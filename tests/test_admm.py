"""GPU: ADMM-SLIM (recoder_amd/admm.py, rk_ease_gemm and rk_ease_admm_update in librecoder_ease.so, AdmmSlimModel)
against the restatements of tests/admm_util.py -- the dense product, the element-wise update bit for bit, a fit at
n = 257, and on the ML-20M slice the fit through ``Recoder`` and what the fitted model plugs into.

Tolerances.  The product: ``(k + 4) 2^-24 (|alpha| (|A| |B|)_ij + |beta| |E_ij|)``, the bound of any summation order
plus the epilogue's two roundings.  The update: bits; its row sums ``(n + 4) 2^-24`` of the sum of the terms.  The fit
at n = 257: 8 times the error, to the same float64 result, of the f32 numpy restatement of the same loop (LAPACK's
f32 inverse, BLAS sgemm): both are f32 chains of length n that differ in order; entries whose float64 |V| lies within
the f32 restatement's own error of theta may fall either side of the threshold and are left out (at most 1 %).  On
the slice: the records of tests/golden/admm_slice.json (tools/admm_bench.py --cpu-grid)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import admm_util as au, ease_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(ease_util.SLICE), "admm_slice.json")


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(a, pad, fill=-7.0):
  """A device buffer [rows, cols + pad] filled with a sentinel, ``a`` in its first columns; (buffer, the view)."""
  buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
  buf[:, :a.shape[1]] = _t(a)
  return buf, buf[:, :a.shape[1]]


def _pair(m):
  from recoder_amd import als
  return als.csr_pair(m, m.shape[0], m.shape[1], DEV)


# ---------------------------------------------------------------------- gemm
SIZES = (1, 31, 127, 128, 129, 257)


def _gemm_case(m, n, k, mode, rng, alpha=-1.75, beta=0.625):
  """One product into a padded D; returns (got [m, n], D's padding, A, B, E)."""
  from recoder_amd import admm
  A, B, E = rng.randn(m, k).astype(np.float32), rng.randn(k, n).astype(np.float32), rng.randn(m, n).astype(np.float32)
  _, Av = _padded(A, 3)
  _, Bv = _padded(B, 5)
  Db, Dv = _padded(E if mode == "D" else np.full((m, n), 9.0, np.float32), 2)
  Eb, Ev = _padded(E, 7)
  admm.gemm(Av, Bv, Dv, alpha, beta, E={"null": None, "D": Dv, "sep": Ev}[mode])
  if mode == "sep":
    assert np.array_equal(Eb.cpu().numpy()[:, :n], E) and np.all(Eb.cpu().numpy()[:, n:] == -7.0), "E was written"
  Dh = Db.cpu().numpy()
  return Dh[:, :n], Dh[:, n:], A, B, E


@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 257])
def test_gemm_against_float64(k):
  rng = np.random.RandomState(100 + k)
  alpha, beta = -1.75, 0.625
  worst = 0.0
  for a, m in enumerate(SIZES):
    for b, n in enumerate(SIZES):
      for mode in ("null", "D", "sep"):
        got, pad, A, B, E = _gemm_case(m, n, k, mode, rng, alpha, beta)
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        want = alpha * (A64 @ B64)
        bound = abs(alpha) * (np.abs(A64) @ np.abs(B64))
        if mode != "null":
          want = want + beta * E.astype(np.float64)
          bound = bound + abs(beta) * np.abs(E).astype(np.float64)
        bound = (k + 4) * U24 * bound
        err = np.abs(got - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (m, n, k, mode)
        assert np.all(pad == -7.0), "the padding of D was written"
  print("gemm k=%d: max err / bound = %.3g" % (k, worst))


@pytest.mark.parametrize("m,n,k", [(257, 129, 65), (129, 257, 257), (31, 1, 3)])
def test_gemm_row_ranges_and_repeats_give_the_same_bits(m, n, k):
  from recoder_amd import admm
  rng = np.random.RandomState(m + n + k)
  A, B, E = _t(rng.randn(m, k)), _t(rng.randn(k, n)), _t(rng.randn(m, n))
  full = admm.gemm(A, B, torch.empty(m, n, device=DEV), 0.5, -2.0, E=E).cpu().numpy()
  again = admm.gemm(A, B, torch.empty(m, n, device=DEV), 0.5, -2.0, E=E).cpu().numpy()
  assert np.array_equal(_bits(full), _bits(again))
  for lo, hi in ((0, 1), (m // 3, m // 3 + 130 if m > 200 else m), (m - 1, m), (5, 5)):
    hi = min(hi, m)
    out = torch.full((m, n), 3.0, device=DEV)
    admm.gemm(A, B, out, 0.5, -2.0, E=E, row_lo=lo, row_hi=hi)
    out = out.cpu().numpy()
    assert np.array_equal(_bits(out[lo:hi]), _bits(full[lo:hi])), (lo, hi)
    assert np.all(out[:lo] == 3.0) and np.all(out[hi:] == 3.0), "rows outside the range were written"
  # one column of a wider product: an element does not depend on its tile
  j = n // 2
  col = admm.gemm(A, B[:, j:j + 1].contiguous(), torch.empty(m, 1, device=DEV), 0.5, -2.0,
                  E=E[:, j:j + 1].contiguous()).cpu().numpy()
  assert np.array_equal(_bits(col[:, 0]), _bits(full[:, j]))


def test_gemm_is_the_ascending_fmaf_chain():
  """The header's order, restated with ease_util.fmaf: the chain from +0 over t ascending, alpha * dot, fma(beta, E, .)."""
  from recoder_amd import admm
  rng = np.random.RandomState(5)
  m, n, k = 33, 40, 37
  A, B, E = (rng.randn(*s).astype(np.float32) for s in ((m, k), (k, n), (m, n)))
  acc = np.zeros((m, n), np.float32)
  for t in range(k):
    acc = ease_util.fmaf(A[:, t:t + 1], B[t:t + 1, :], acc)
  p = np.float32(1.3) * acc
  want = ease_util.fmaf(np.float32(-0.7), E, p)
  got = admm.gemm(_t(A), _t(B), torch.empty(m, n, device=DEV), 1.3, -0.7, E=_t(E)).cpu().numpy()
  assert np.array_equal(_bits(got), _bits(want))
  got = admm.gemm(_t(A), _t(B), torch.empty(m, n, device=DEV), 1.3).cpu().numpy()
  assert np.array_equal(_bits(got), _bits(p))


# -------------------------------------------------------------------- update
@pytest.mark.parametrize("n", [1, 33, 129])
@pytest.mark.parametrize("nonneg", [False, True])
@pytest.mark.parametrize("theta", [0.0, 0.3])
def test_update_bit_for_bit(n, nonneg, theta):
  from recoder_amd import admm
  rng = np.random.RandomState(n + 2 * nonneg)
  T, C, U = (rng.randn(n, n).astype(np.float32) for _ in range(3))      # (non-zero diagonals: the call zeroes them)
  P = (rng.randn(n, n) * 0.1 + np.eye(n) * (1 + rng.rand(n))).astype(np.float32)
  for lo, hi in ((0, n), (n // 3, n - n // 4)):
    wC, wU, wM, wg, wp, wd, wn = au.update_f32(T, P, C, U, theta, nonneg, lo, hi)
    dC, dU, dM = _t(C), _t(U), torch.zeros(n, n, device=DEV)
    g, rp, rd = (torch.full((n,), -5.0, device=DEV) for _ in range(3))
    rn = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    admm.admm_update(_t(T), _t(P), dC, dU, dM, theta, nonneg, g, rp, rd, rn, lo, hi)
    if lo == hi:
      continue
    for name, got, want in (("C", dC, wC), ("U", dU, wU), ("M", dM, wM), ("gamma", g, wg)):
      assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (name, lo, hi)
    for a in (dC, dU, dM):
      d = np.diag(a.cpu().numpy())[lo:hi]
      assert not d.any() and not np.signbit(d).any(), "a diagonal is not +0"
    rp, rd, rn = rp.cpu().numpy(), rd.cpu().numpy(), rn.cpu().numpy()
    out = np.r_[0:lo, hi:n]
    assert np.all(rp[out] == -5.0) and np.all(rd[out] == -5.0) and np.all(rn[out] == -5), "rows outside the range"
    assert np.array_equal(rn[lo:hi], wn)
    assert np.all(np.abs(rp[lo:hi] - wp) <= (n + 4) * U24 * wp) and np.all(np.abs(rd[lo:hi] - wd) <= (n + 4) * U24 * wd)
    if theta == 0.0 and not nonneg and n > 1:
      off = ~np.eye(n, dtype=bool)[lo:hi]
      assert not dU.cpu().numpy()[lo:hi][off].any(), "theta = 0: C_new = V and U = 0"


# ------------------------------------------------------------- fit at n = 257
L1, L2, RHO, ITERS = 2.0, 50.0, 100.0, 30


@pytest.fixture(scope="module")
def small():
  return au.zipf_matrix(600, 257, seed=0)


@pytest.mark.parametrize("nonneg", [False, True])
def test_fit_against_the_float64_loop(small, nonneg):
  from recoder_amd import admm
  C64, i64 = au.fit(small, L1, L2, RHO, ITERS, nonneg)
  C32, _ = au.fit(small, L1, L2, RHO, ITERS, nonneg, dtype=np.float32)
  C, info = admm.fit(_pair(small), L1, L2, RHO, ITERS, nonneg)
  C = C.cpu().numpy()
  scale = np.abs(C64).max()
  e32_abs = np.abs(C32 - C64).max()
  V = i64["V"] if nonneg else np.abs(i64["V"])
  keep = np.abs(V - L1 / RHO) > e32_abs
  left_out = 1.0 - keep.mean()
  e32, egpu = e32_abs / scale, np.abs(C - C64)[keep].max() / scale
  print("fit n=257 nonneg %s: kernels %.3g, f32 numpy %.3g (ratio %.2f), left out %.4f %%"
        % (nonneg, egpu, e32, egpu / e32, 100 * left_out))
  assert left_out <= 0.01
  assert egpu <= 8 * e32
  d = np.diag(C)
  assert not d.any() and not np.signbit(d).any()
  if nonneg:
    assert C.min() == 0.0
  assert info["iterations"] == ITERS and len(info["primal_residual"]) == len(info["dual_residual"]) == ITERS
  # (Frobenius norms over n^2 entries, each within the budget above: n times it, twice for a difference of two)
  floor = 2 * 257 * 8 * e32_abs
  np.testing.assert_allclose(info["primal_residual"], i64["primal_residual"], rtol=1e-4, atol=floor)
  np.testing.assert_allclose(info["dual_residual"], i64["dual_residual"], rtol=1e-4, atol=RHO * floor)
  assert abs(info["density"] - i64["density"]) <= 0.01 * i64["density"] + left_out
  # a second fit gives the same bits
  C2, _ = admm.fit(_pair(small), L1, L2, RHO, ITERS, nonneg)
  assert np.array_equal(_bits(C2.cpu().numpy()), _bits(C))


def test_a_non_positive_pivot_is_eases_value_error():
  from recoder_amd import admm
  X = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, -1.0]], np.float32))
  X.data[:] = [np.nan, 1.0]
  with pytest.raises(ValueError, match="not positive definite"):
    admm.fit(_pair(X), 0.0, 1.0, 1.0, 2, False)


# ---------------------------------------------------------------- on the slice
def _slice():
  z = np.load(ease_util.SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


@pytest.fixture(scope="module")
def golden():
  return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  x, y = _slice()
  rec = Recoder(model=AdmmSlimModel())
  info = rec.train_admm_slim(RecommendationDataset(x))
  return rec, info, x, y


def _evaluate(rec, x, y):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  return got[str(Recall(k=20))], got[str(NDCG(k=100))]


def test_the_golden_record_is_the_models_default_cell(golden):
  from recoder_amd.nn import AdmmSlimModel
  assert AdmmSlimModel().model_params() == golden["default"]["params"]


def test_defaults_on_the_slice(fitted, golden):
  rec, info, x, y = fitted
  m = rec.model
  assert info["n"] == x.shape[1] and info["nnz"] == x.nnz and info["iterations"] == m.num_iterations
  assert (info["l1_reg"], info["l2_reg"], info["rho"], info["nonneg"]) == (m.l1_reg, m.l2_reg, m.rho, m.nonneg)
  assert all(info[k] > 0 for k in ("gram_ms", "inverse_ms", "admm_ms"))
  primal, dual = info["primal_residual"], info["dual_residual"]
  assert len(primal) == len(dual) == m.num_iterations
  assert primal[-1] < primal[-6] < primal[-11] and dual[-1] < dual[-6] < dual[-11]
  print("ADMM-SLIM on the slice: gram %.2f ms, inverse %.2f ms, %d iterations %.1f ms; primal %.3g, dual %.3g, "
        "density %.5f (golden %.5f)" % (info["gram_ms"], info["inverse_ms"], m.num_iterations, info["admm_ms"],
                                        primal[-1], dual[-1], info["density"], golden["default"]["density"]))
  C = m.item_weights.data
  assert not bool(torch.diagonal(C).any())
  if m.nonneg:
    assert float(C.min()) == 0.0
  assert abs(float((C != 0).double().mean()) - info["density"]) < 1e-12
  assert abs(info["density"] - golden["default"]["density"]) <= 0.02 * golden["default"]["density"]
  r20, n100 = _evaluate(rec, x, y)
  print("slice at the defaults: Recall@20 gpu %.6f f64 %.6f; NDCG@100 gpu %.6f f64 %.6f"
        % (r20, golden["default"]["recall20"], n100, golden["default"]["ndcg100"]))
  assert abs(r20 - golden["default"]["recall20"]) <= 1e-3
  assert abs(n100 - golden["default"]["ndcg100"]) <= 1e-3


def test_without_l1_the_fit_meets_the_kernels_ease(golden):
  """l1 = 0, nonneg False at the recorded (l2, rho, iterations): item_weights against train_ease(reg = l2) from the
  same kernels, within the float64 loop's truncation distance there plus the f32 budget of tests/test_ease.py's
  weights (both recorded by tools/admm_bench.py --cpu-grid)."""
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel, ShallowAutoencoder
  x, _ = _slice()
  g = golden["ease_limit"]
  rec = Recoder(model=AdmmSlimModel())
  rec.train_admm_slim(RecommendationDataset(x), l1_reg=0.0, l2_reg=g["l2_reg"], rho=g["rho"],
                      num_iterations=g["num_iterations"], nonneg=False)
  ease = Recoder(model=ShallowAutoencoder(g["l2_reg"]))
  ease.train_ease(RecommendationDataset(x))
  dist = float((rec.model.item_weights.data - ease.model.item_weights.data).abs().max())
  print("l1 = 0 on the slice: max|C - B_ease| %.3g; truncation %.3g + f32 budget %.3g"
        % (dist, g["truncation_distance"], g["ease_weights_budget"]))
  assert dist <= g["truncation_distance"] + g["ease_weights_budget"]


def test_checkpoint_round_trip(fitted, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "admm"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == rec.model.model_params() and list(st["model"]) == ["item_weights"]
  rec2 = Recoder(model=AdmmSlimModel(l1_reg=9.0, l2_reg=9.0, rho=9.0, num_iterations=9, nonneg=False))
  rec2.init_from_model_file(f)
  assert rec2.model.model_params() == rec.model.model_params()
  inp = UsersInteractions(np.arange(300), x[:300])
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


def test_strips_give_the_same_lists(fitted):
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  inp = UsersInteractions(np.arange(200), x[:200])
  want = rec.recommend_array(inp, 20)
  rec.eval_strip_items = 3000
  try:
    got = rec.recommend_array(inp, 20)
  finally:
    del rec.eval_strip_items
  assert np.array_equal(got, want)


def test_a_refit_reuses_the_buffer_and_stores_explicit_hyperparameters(small):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  rec = Recoder(model=AdmmSlimModel())
  ds = RecommendationDataset(small)
  info = rec.train_admm_slim(ds, l1_reg=L1, l2_reg=L2, rho=RHO, num_iterations=ITERS, nonneg=False)
  want = {"l1_reg": L1, "l2_reg": L2, "rho": RHO, "num_iterations": ITERS, "nonneg": False}
  assert rec.model.model_params() == want and {k: info[k] for k in ("l1_reg", "l2_reg", "rho", "nonneg")} == \
      {k: want[k] for k in ("l1_reg", "l2_reg", "rho", "nonneg")} and info["iterations"] == ITERS
  where, first = rec.model.item_weights.data_ptr(), rec.model.item_weights.data.clone()
  info = rec.train_admm_slim(ds, nonneg=True)
  assert rec.model.item_weights.data_ptr() == where and rec.model.nonneg is True and rec.model.rho == RHO
  assert info == rec.admm_info and info["nonneg"] is True
  assert float(rec.model.item_weights.data.min()) == 0.0 and float(first.min()) < 0.0
  with pytest.raises(ValueError, match="train_admm_slim"):
    rec.train(ds)
