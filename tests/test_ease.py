"""GPU: EASE (recoder_amd/ease.py, librecoder_ease.so, ShallowAutoencoder) against the float64
restatement of tests/ease_util.py -- the Gram, the SPD inverse, finalize, the scores, a fit on the
ML-20M slice and what the fitted model plugs into (recommend, evaluate, checkpoints, predict).

The inverse's bound: e(P) = max|P - P64| / max|P64| and the float64 residual max|A P - I| of the GPU
result may be at most M_INV times those of np.linalg.inv(A.astype(float32)), computed here.  M_INV
is 4 (an unpivoted blocked elimination has larger constants than LAPACK's pivoted LU).  Measured on an
MI355X (e ratio / residual ratio): n <= 64: 1.00 / 1.00; n = 65: 1.58 / 1.60; 127: 3.64 / 2.02;
128: 2.02 / 1.81; 129: 3.97 / 2.47; 257: 2.65 / 1.77; the slice at reg = 10: 2.08 / 1.70, at reg = 500:
1.93 / 1.93.  (Without the compensated update the slice gave 26.7 and 28.6: DESIGN section 4.)"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import als_util, ease_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
M_INV = 4.0


def _t(a):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _slice():
  z = np.load(ease_util.SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def _pair(m):
  from recoder_amd import als
  return als.csr_pair(m, m.shape[0], m.shape[1], DEV)


def _dev_csr(m):
  from recoder_amd.als import AlsCSR
  return AlsCSR(sp.csr_matrix(m), DEV)


# ---------------------------------------------------------------------- gram
def _gram_matrix(n, values, seed):
  """Random CSR with empty rows, an item nobody touched (when n > 1) and one item every user touched."""
  rows = {1: 50, 37: 300, 7915: 3000}[n]
  dens = {1: 0.5, 37: 0.2, 7915: 0.004}[n]
  m = als_util.random_csr(rows, n, dens, seed=seed, values=values, empty_rows=(0, rows // 2)).tolil()
  rng = np.random.RandomState(seed + 1)
  full, none = (n // 3, n // 2) if n > 1 else (0, None)
  for r in range(rows):
    if r in (0, rows // 2):
      continue
    m[r, full] = 1.0 if values == "binary" else float(np.round(rng.rand() * 4, 1) + 0.5)
  m = m.tocsr()
  if none is not None:
    m = m.tolil()
    m[:, none] = 0
    m = m.tocsr()
  m.eliminate_zeros()
  m.sort_indices()
  return m.astype(np.float32), none


@pytest.mark.parametrize("n", [1, 37, 7915])
@pytest.mark.parametrize("values", ["binary", "counts"])
def test_gram_against_float64(n, values):
  from recoder_amd import ease
  m, none = _gram_matrix(n, values, seed=n + 3)
  reg = 500.0 if values == "binary" else 3.5
  uc, ic = _pair(m)
  assert (uc.data is None) == (values == "binary")
  G = ease.gram(uc, ic, reg).cpu().numpy()
  G2 = ease.gram(uc, ic, reg).cpu().numpy()
  want = ease_util.gram(m, reg)
  if values == "binary":
    # every entry is an integer below 2^24: the f32 chain is exact
    assert want.max() < 2 ** 24
    assert np.array_equal(G, want.astype(np.float32))
  else:
    a = abs(m).astype(np.float64)
    bound = 1e-6 * np.sqrt(m.shape[0]) * np.asarray((a.T @ a).todense()) + 1e-6 * reg * np.eye(n)
    err = np.abs(G - want)
    print("gram n=%d: max err / bound = %.3g" % (n, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound)
  assert np.array_equal(G, G.T), "A not bitwise symmetric"
  assert np.array_equal(G, G2), "not bitwise repeatable (the header promises it for every value)"
  if none is not None:
    assert G[none, none] == np.float32(reg) and not G[none, :none].any() and not G[none, none + 1:].any()


def test_gram_into_a_wider_buffer():
  from recoder_amd import _ease_lib, ease
  from recoder_amd.device import current_stream
  m, _ = _gram_matrix(37, "binary", seed=9)
  uc, ic = _pair(m)
  buf = torch.full((37, 48), -7.0, device=DEV)
  lib = _ease_lib.load()
  _ease_lib.check(lib.rk_ease_gram(ic.indptr.data_ptr(), ic.indices.data_ptr(), None, uc.indptr.data_ptr(),
                                   uc.indices.data_ptr(), None, m.shape[0], 37, 2.0, buf.data_ptr(), 48,
                                   current_stream()), "rk_ease_gram")
  buf = buf.cpu().numpy()
  assert np.array_equal(buf[:, :37], ease_util.gram(m, 2.0).astype(np.float32)) and np.all(buf[:, 37:] == -7.0)
  assert np.array_equal(ease.gram(uc, ic, 2.0).cpu().numpy(), buf[:, :37])


# ------------------------------------------------------------------- inverse
def _check_inverse(A32, label):
  from recoder_amd import ease
  A64 = A32.astype(np.float64)
  P64 = np.linalg.inv(A64)
  P32 = np.linalg.inv(A32)
  P = ease.spd_inverse(_t(A32).clone()).cpu().numpy()
  e_gpu, e_ref = ease_util.rel_err(P, P64), ease_util.rel_err(P32, P64)
  r_gpu, r_ref = ease_util.residual(A64, P), ease_util.residual(A64, P32)
  print("inverse %s: e_gpu %.3g e_lapack32 %.3g ratio %.2f; residual gpu %.3g lapack32 %.3g ratio %.2f"
        % (label, e_gpu, e_ref, e_gpu / e_ref, r_gpu, r_ref, r_gpu / r_ref))
  assert np.all(np.isfinite(P))
  assert e_gpu <= M_INV * e_ref
  assert r_gpu <= M_INV * r_ref
  return P


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257])
def test_inverse_small_spd(n):
  rng = np.random.RandomState(n)
  F = rng.randn(2 * n + 3, n)
  A32 = (F.T @ F + 0.5 * np.eye(n)).astype(np.float32)
  A32 = np.maximum(A32, A32.T)                 # (bitwise symmetric input)
  _check_inverse(A32, "n=%d" % n)


def test_inverse_with_a_leading_dimension():
  from recoder_amd import _ease_lib, ease
  from recoder_amd.device import current_stream
  n, ld = 70, 96
  rng = np.random.RandomState(5)
  F = rng.randn(200, n)
  A32 = (F.T @ F + np.eye(n)).astype(np.float32)
  buf = torch.full((n, ld), 9.0, device=DEV)
  buf[:, :n] = _t(A32)
  lib = _ease_lib.load()
  ws = torch.empty(lib.rk_ease_spd_inverse_workspace_bytes(n), dtype=torch.uint8, device=DEV)
  status = torch.ones(1, dtype=torch.int32, device=DEV)
  _ease_lib.check(lib.rk_ease_spd_inverse(buf.data_ptr(), n, ld, ws.data_ptr(), ws.numel(), status.data_ptr(),
                                          current_stream()), "rk_ease_spd_inverse")
  assert int(status.item()) == 0
  got = buf.cpu().numpy()
  assert np.all(got[:, n:] == 9.0)
  assert np.array_equal(got[:, :n], ease.spd_inverse(_t(A32).clone()).cpu().numpy())


@pytest.fixture(scope="module")
def slice_fits():
  """{reg: (A32, P64, e(P_lapack32))} on the ML-20M slice, computed once."""
  x, _ = _slice()
  out = {}
  for reg in (10.0, 500.0):
    A64 = ease_util.gram(x, reg)
    A32 = A64.astype(np.float32)
    assert np.array_equal(A32.astype(np.float64), A64)
    out[reg] = A32
  return out


@pytest.mark.parametrize("reg", [10.0, 500.0])
def test_inverse_on_the_slice(slice_fits, reg):
  _check_inverse(slice_fits[reg], "slice reg=%g" % reg)


def test_zero_pivot_raises_value_error():
  from recoder_amd import ease
  m, none = _gram_matrix(37, "binary", seed=4)
  A = ease_util.gram(m, 0.0).astype(np.float32)
  assert not A[none].any() and not A[:, none].any()
  with pytest.raises(ValueError, match="positive definite"):
    ease.spd_inverse(_t(A).clone())


def test_the_process_is_usable_after_a_zero_pivot():
  from recoder_amd import ease
  A = np.diag(np.float32([2.0, 4.0, 8.0]))
  assert np.array_equal(ease.spd_inverse(_t(A).clone()).cpu().numpy(), np.diag(np.float32([0.5, 0.25, 0.125])))


# ------------------------------------------------------------------ finalize
@pytest.mark.parametrize("in_place", [True, False])
def test_finalize_is_the_f32_formula_bit_for_bit(in_place):
  from recoder_amd import ease
  x, _ = _slice()
  _, P64 = ease_util.fit(x[:, :900], 10.0)
  P32 = P64.astype(np.float32)
  want = ease_util.finalize_f32(P32)
  Pt = _t(P32).clone()
  out = None if in_place else torch.full_like(Pt, 3.0)
  B, diag = ease.finalize(Pt, out)
  assert (B.data_ptr() == Pt.data_ptr()) == in_place
  B = B.cpu().numpy()
  assert np.array_equal(B.view(np.uint32), want.view(np.uint32))
  assert np.all(np.diag(B).view(np.uint32) == 0), "the diagonal must be +0"
  assert np.array_equal(diag.cpu().numpy(), np.diag(P32))
  if not in_place:
    assert np.array_equal(Pt.cpu().numpy(), P32)


# -------------------------------------------------------------------- scores
def test_scores_are_the_ascending_fmaf_chain():
  from recoder_amd import ease
  x, _ = _slice()
  lens = np.diff(x.indptr)
  assert lens.max() == 274
  # users with 0, 1 and 274 items (the slice's longest row; it has no user with fewer than two, so the
  # first two rows are an empty one and the first entry of the longest) and two ordinary ones
  longest = x[int(np.argmax(lens))]
  one = sp.csr_matrix((longest.data[:1], longest.indices[:1], [0, 1]), shape=longest.shape)
  plain = sp.vstack([sp.csr_matrix(longest.shape, dtype=np.float32), one, longest, x[7], x[1]]).tocsr()
  assert list(np.diff(plain.indptr)[:3]) == [0, 1, 274]
  sub = plain.copy()
  sub.data = (sub.data * np.random.RandomState(0).choice([1.0, 0.5, 3.0, -2.0], sub.nnz)).astype(np.float32)
  W = np.random.RandomState(1).randn(x.shape[1], 2100).astype(np.float32)
  Wt = _t(W)
  csr = _dev_csr(sub)
  got = ease.scores(csr, Wt).cpu().numpy()
  want = ease_util.scores_chain_f32(sub, W)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  assert not got[0].any()
  # a strip gives bitwise the columns of the full call, whatever the batch position
  for lo, hi in ((0, 1), (1023, 1025), (37, 2100), (2099, 2100)):
    part = ease.scores(csr, Wt, lo, hi).cpu().numpy()
    assert np.array_equal(part.view(np.uint32), got[:, lo:hi].view(np.uint32))
  rev = ease.scores(_dev_csr(sub[::-1]), Wt).cpu().numpy()
  assert np.array_equal(rev[::-1].view(np.uint32), got.view(np.uint32))
  # unit values: the NULL data path
  ones = plain
  c1 = _dev_csr(ones)
  assert c1.data is None
  assert np.array_equal(ease.scores(c1, Wt).cpu().numpy().view(np.uint32),
                        ease_util.scores_chain_f32(ones, W).view(np.uint32))
  # out with a leading dimension: columns past the strip are left alone
  out = torch.full((plain.shape[0], 64), 5.0, device=DEV)
  ease.scores(csr, Wt, 10, 47, out=out)
  out = out.cpu().numpy()
  assert np.array_equal(out[:, :37], got[:, 10:47]) and np.all(out[:, 37:] == 5.0)


# ---------------------------------------------------------------- end to end
REG = 500.0


@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  x, y = _slice()
  rec = Recoder(model=ShallowAutoencoder(REG))
  info = rec.train_ease(RecommendationDataset(x))
  return rec, info, x, y


@pytest.fixture(scope="module")
def restated():
  """(B64, float64 scores, e(P_lapack32)) on the slice at REG."""
  x, _ = _slice()
  A64 = ease_util.gram(x, REG)
  P64 = np.linalg.inv(A64)
  e_ref = ease_util.rel_err(np.linalg.inv(A64.astype(np.float32)), P64)
  B64 = ease_util.weights(P64)
  return B64, ease_util.scores(x, B64), e_ref


def _weights_budget(A64, P64, B64):
  """The inverse's budget carried to B = -P / diag(P), to first order: |dB_ij| <= |dP_ij| / p_jj +
  |B_ij| |dp_jj| / p_jj with |dP| <= M_INV e(P_lapack32) max|P|; doubled for the higher-order terms and
  the divide's own rounding."""
  e_ref = ease_util.rel_err(np.linalg.inv(A64.astype(np.float32)), P64)
  return 2 * M_INV * e_ref * np.abs(P64).max() / np.diag(P64).min() * (1 + np.abs(B64).max())


def _metric_means(lists, y, ks=((20, "recall"), (100, "ndcg"))):
  from recoder_amd import metrics as M
  out = []
  for k, kind in ks:
    vals = []
    for u in range(y.shape[0]):
      t = y.indices[y.indptr[u]:y.indptr[u + 1]]
      if len(t):
        vals.append(M.recall(lists[u], t, k) if kind == "recall" else M.ndcg(lists[u], t, k))
    out.append(float(np.mean(vals)))
  return out


def test_train_ease_info_and_weights(fitted, restated):
  rec, info, x, _ = fitted
  assert info["n"] == x.shape[1] and info["nnz"] == x.nnz and info["reg"] == REG
  assert all(info[k] > 0 for k in ("gram_ms", "inverse_ms", "finalize_ms")) and "diag" not in info
  print("EASE fit on the slice: gram %.2f ms, inverse %.2f ms, finalize %.3f ms"
        % (info["gram_ms"], info["inverse_ms"], info["finalize_ms"]))
  B = rec.model.item_weights.data.cpu().numpy()
  B64, _, e_ref = restated
  assert not np.diag(B).any()
  A64 = ease_util.gram(x, REG)
  budget = _weights_budget(A64, np.linalg.inv(A64), B64)
  print("max|B - B64| %.3g (budget %.3g), max|B64| %.3g" % (np.abs(B - B64).max(), budget, np.abs(B64).max()))
  assert np.abs(B - B64).max() <= budget
  assert np.array_equal(rec.ease_info["diag"].shape, (x.shape[1],))


def test_metrics_on_the_slice_match_float64(fitted, restated):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  rec, _, x, y = fitted
  _, S64, _ = restated
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  want_r, want_n = _metric_means(ease_util.top_k(S64, x, 100), y)
  print("slice reg=%g: Recall@20 gpu %.6f f64 %.6f; NDCG@100 gpu %.6f f64 %.6f"
        % (REG, got[str(Recall(k=20))], want_r, got[str(NDCG(k=100))], want_n))
  assert abs(got[str(Recall(k=20))] - want_r) <= 1e-3
  assert abs(got[str(NDCG(k=100))] - want_n) <= 1e-3


def test_every_top20_list_is_valid_under_float64(fitted, restated):
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  B64, S64, e_ref = restated
  n_users = x.shape[0]
  lists = np.concatenate([rec.recommend_array(UsersInteractions(np.arange(lo, min(n_users, lo + 500)),
                                                                x[lo:lo + 500]), 20)
                          for lo in range(0, n_users, 500)])
  assert lists.shape == (n_users, 20)
  absx, absB = abs(x).astype(np.float64), np.abs(B64)
  l1 = np.asarray(absx.sum(1)).ravel()
  d = np.diff(x.indptr)
  tau = M_INV * e_ref * absB.max() * l1 + d * 2.0 ** -23 * np.asarray(absx @ absB).max(1)
  masked = S64.copy()
  worst_slack = -np.inf
  for u in range(n_users):
    seen = x.indices[x.indptr[u]:x.indptr[u + 1]]
    assert len(set(lists[u])) == 20 and not np.isin(lists[u], seen).any(), "a seen or repeated item"
    assert lists[u].min() >= 0 and lists[u].max() < x.shape[1]
    masked[u, seen] = -np.inf
    kth = np.partition(masked[u], -20)[-20]
    slack = kth - S64[u, lists[u]].min() - 2 * tau[u]
    worst_slack = max(worst_slack, slack)
    assert slack <= 0, "user %d: the list's worst float64 score is %.3g below the 20th best, budget %.3g" \
        % (u, kth - S64[u, lists[u]].min(), 2 * tau[u])
  same = np.mean([np.array_equal(a, b) for a, b in zip(lists, ease_util.top_k(S64, x, 20))])
  print("top-20 lists identical to float64: %.2f %%; worst slack %.3g" % (100 * same, worst_slack))


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
  from recoder_amd.nn import ShallowAutoencoder
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "ease"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == {"reg": REG} and list(st["model"]) == ["item_weights"]
  rec2 = Recoder(model=ShallowAutoencoder(1.0))
  rec2.init_from_model_file(f)
  assert rec2.model.reg == REG
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))


def test_explicit_reg_is_stored_in_the_model():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  m = als_util.random_csr(80, 70, 0.2, seed=3, values="counts")
  rec = Recoder(model=ShallowAutoencoder(500.0))
  info = rec.train_ease(RecommendationDataset(m), reg=2.5)
  assert rec.model.reg == 2.5 and info["reg"] == 2.5 and rec.model.model_params() == {"reg": 2.5}
  B64, P64 = ease_util.fit(m, 2.5)
  err = np.abs(rec.model.item_weights.data.cpu().numpy() - B64).max()
  assert err <= _weights_budget(ease_util.gram(m, 2.5), P64, B64)
  with pytest.raises(ValueError, match="train_ease"):
    rec.train(RecommendationDataset(m))


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


def test_large_k_falls_back_and_agrees_with_the_kernel_path(fitted):
  from recoder_amd import _lib
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  kmax = _lib.load().rk_topk_max_k()
  inp = UsersInteractions(np.arange(40), x[:40])
  big = rec.recommend_array(inp, kmax + 1)
  assert big.shape == (40, kmax + 1)
  assert np.array_equal(big[:, :kmax], rec.recommend_array(inp, kmax))


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


def test_predict_and_forward_equal_the_scores_kernel(fitted):
  from recoder_amd import ease
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  users = np.arange(64)
  out, _ = rec.predict(UsersInteractions(users, x[users]))
  want = ease.scores(_dev_csr(x[users]), rec.model.item_weights.data)
  assert out.shape == want.shape and torch.equal(out, want)
  dense = torch.from_numpy(np.asarray(x[users].todense(), np.float32)).to(DEV)
  assert torch.equal(rec.model(dense), want)
  tt = torch.tensor([5, 3, 700, 11], device=DEV)
  ii = torch.arange(0, x.shape[1], 2, device=DEV)
  sub = rec.model(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  ref = rec.model.torch_forward(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  assert sub.shape == (64, 4)
  assert torch.allclose(sub, ref, rtol=0, atol=1e-5 * float(ref.abs().max()))
