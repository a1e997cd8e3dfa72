"""GPU: PureSVD (recoder_amd/svd.py, librecoder_svd.so, Recoder.train_svd) against the numpy restatement
of tests/svd_util.py -- the sparse product, the Gaussian, the rotation, the orthonormalisation, the fit
with an injected Omega on a planted matrix and on the ML-20M slice, and what the fitted model plugs into.

Where a device result is held to a multiple of the float32 restatement's own error the multiple is
M_F32 = 4: the device works at the same precision in a different summation order (the margin the EASE
tests give the device against float32 LAPACK, for the same reason)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg
import torch

from tests import als_util, svd_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
M_F32 = 4.0
FLOOR = 1e-6


def _t(a):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _pair(m):
  from recoder_amd import als
  return als.csr_pair(m, m.shape[0], m.shape[1], DEV)


# ----------------------------------------------------------------------- spmm
def _spmm_matrix(values):
  """700 x 6000: ordinary rows of about 60 entries, empty rows, one row of 5000 entries (the 16-wave
  path), one row just below the long-row threshold and one just on or above it; column 11 is touched by 600
  rows, so the transposed matrix has a long row too."""
  from recoder_amd import svd
  m = als_util.random_csr(700, 6000, 0.01, seed=5, values=values, empty_rows=(0, 350, 699)).tolil()
  rng = np.random.RandomState(6)

  def val(n):
    return np.ones(n) if values == "binary" else np.round(rng.rand(n) * 4, 1) + 0.5
  for r, n in ((3, 5002), (4, svd.LONG_ROW - 1), (5, svd.LONG_ROW + 2)):
    cols = np.sort(rng.choice(6000, n, replace=False))
    m.rows[r] = [int(c) for c in cols]
    m.data[r] = [float(v) for v in val(n)]
  m = m.tocsr()
  touch = np.setdiff1d(np.arange(20, 620), [350])
  col = sp.csr_matrix((val(len(touch)), (touch, np.full(len(touch), 11))), shape=m.shape)
  keep = m.copy().tolil()
  keep[:, 11] = 0
  keep[:, 13] = 0                                   # (nobody touches column 13: an empty row of the transpose)
  m = (keep.tocsr() + col).tocsr().astype(np.float32)
  m.eliminate_zeros()
  m.sort_indices()
  d = np.diff(m.indptr)
  # (rows 3 to 5 may have lost their entries in columns 11 and 13)
  assert d[0] == d[350] == d[699] == 0 and d[3] >= 5000
  assert svd.LONG_ROW - 3 <= d[4] < svd.LONG_ROW <= d[5] <= svd.LONG_ROW + 2
  assert np.diff(m.T.tocsr().indptr)[11] >= svd.LONG_ROW
  return m


@pytest.mark.parametrize("l", [1, 20, 80, 216, 512])
@pytest.mark.parametrize("values", ["binary", "counts"])
def test_spmm_against_float64(values, l):
  from recoder_amd import svd
  m = _spmm_matrix(values)
  uc, ic = _pair(m)
  assert (uc.data is None) == (values == "binary")
  rng = np.random.RandomState(l)
  for csr, host in ((uc, m), (ic, m.T.tocsr())):
    F = rng.randn(host.shape[1], l).astype(np.float32)
    Ft = _t(F).reshape(host.shape[1], l)
    got_t = svd.spmm(csr, Ft)
    got = got_t.cpu().numpy()
    h64 = host.astype(np.float64)
    want = np.asarray(h64 @ F.astype(np.float64))
    d = np.maximum(np.diff(host.indptr), 1)
    bound = 1e-6 * np.sqrt(d)[:, None] * np.asarray(abs(h64) @ np.abs(F).astype(np.float64)) + 1e-30
    err = np.abs(got - want)
    print("spmm %s l=%d %s: max err / bound = %.3g" % (values, l, host.shape, float((err / bound).max())))
    assert np.all(err <= bound)
    empty = np.diff(host.indptr) == 0
    assert empty.any() and not got[empty].any()
    # bitwise repeatable; a row range gives bitwise the rows of the full call and touches nothing else
    assert torch.equal(svd.spmm(csr, Ft), got_t)
    buf = torch.full_like(got_t, -7.0)
    lo, hi = 2, min(host.shape[0] - 1, 401)
    svd.spmm(csr, Ft, out=buf, row_lo=lo, row_hi=hi)
    assert torch.equal(buf[lo:hi], got_t[lo:hi]) and bool((buf[:lo] == -7.0).all()) and bool((buf[hi:] == -7.0).all())
    # operands with odd leading dimensions (the 4-byte path): the same bits
    Fw = torch.zeros(host.shape[1], l + 3, device=DEV)
    Fw[:, :l] = Ft
    outw = torch.full((host.shape[0], l + 1), 9.0, device=DEV)
    svd.spmm(csr, Fw[:, :l], out=outw[:, :l])
    assert torch.equal(outw[:, :l], got_t) and bool((outw[:, l:] == 9.0).all())


# ------------------------------------------------------------------- gaussian
def test_gaussian_is_seeded_and_standard_normal():
  from recoder_amd import svd
  a = svd.gaussian(5000, 200, 7)
  assert torch.equal(a, svd.gaussian(5000, 200, 7))
  b = svd.gaussian(5000, 200, 8)
  assert float((a == b).float().mean()) < 1e-3
  # keyed on (seed, row, column): neither the leading dimension nor the number of rows matters
  wide = torch.full((300, 256), 3.0, device=DEV)
  svd.gaussian(300, 200, 7, out=wide[:, :200])
  assert torch.equal(wide[:, :200], a[:300]) and bool((wide[:, 200:] == 3.0).all())
  x = a.double().cpu().numpy().ravel()
  n = x.size
  assert n == 10 ** 6 and np.all(np.isfinite(x))
  print("gaussian: mean %.3g (5 se %.3g), var - 1 %.3g (5 se %.3g)"
        % (x.mean(), 5 / np.sqrt(n), x.var() - 1, 5 * np.sqrt(2 / n)))
  assert abs(x.mean()) <= 5 / np.sqrt(n)
  assert abs(x.var() - 1) <= 5 * np.sqrt(2 / n)
  c = np.corrcoef(a[:, 0].cpu().numpy(), a[:, 1].cpu().numpy())[0, 1]
  assert abs(c) <= 5 / np.sqrt(5000)


# --------------------------------------------------------------------- rotate
@pytest.mark.parametrize("rows,l,l2", [(1003, 20, 20), (1003, 80, 80), (1003, 216, 216), (1003, 24, 8),
                                       (517, 216, 200), (130, 512, 512), (65, 1, 1), (64, 300, 260), (1, 33, 257)])
def test_rotate_against_float64(rows, l, l2):
  from recoder_amd import svd
  rng = np.random.RandomState(rows + l + l2)
  Y = rng.randn(rows, l).astype(np.float32)
  M = rng.randn(l, l2).astype(np.float32)          # (not symmetric: a swapped index would show)
  Yt, Mt = _t(Y).reshape(rows, l), _t(M).reshape(l, l2)
  got_t = svd.rotate(Yt, Mt)
  got = got_t.cpu().numpy()
  want = Y.astype(np.float64) @ M.astype(np.float64)
  bound = 1e-6 * np.sqrt(l) * (np.abs(Y).astype(np.float64) @ np.abs(M).astype(np.float64)) + 1e-30
  err = np.abs(got - want)
  print("rotate %dx%dx%d: max err / bound = %.3g" % (rows, l, l2, float((err / bound).max())))
  assert np.all(err <= bound)
  assert torch.equal(svd.rotate(Yt, Mt), got_t), "not bitwise repeatable"
  wide = torch.full((rows, l2 + 5), 2.0, device=DEV)
  svd.rotate(Yt, Mt, out=wide[:, :l2])
  assert torch.equal(wide[:, :l2], got_t) and bool((wide[:, l2:] == 2.0).all())
  # every output is one k-ascending fmaf chain: the identity gives Y back bit for bit
  if l == l2:
    assert torch.equal(svd.rotate(Yt, torch.eye(l, device=DEV)), Yt)


# ------------------------------------------------------------- orthonormalize
@pytest.mark.parametrize("l", [20, 80, 129, 216])
def test_orthonormalize_against_the_float32_restatement(l):
  from recoder_amd import svd
  rng = np.random.RandomState(l)
  rows = 3000
  mix = rng.randn(l, l) + 2.0 * np.eye(l)
  Y = (rng.randn(rows, l) @ mix).astype(np.float32)
  Q32 = svd_util.orth(Y.copy()).astype(np.float64)
  Q = svd.orthonormalize(_t(Y).reshape(rows, l).clone()).cpu().numpy().astype(np.float64)
  e_gpu = np.abs(Q.T @ Q - np.eye(l)).max()
  e_ref = np.abs(Q32.T @ Q32 - np.eye(l)).max()
  print("orthonormalize l=%d (cond %.1f): max|Q^T Q - I| gpu %.3g, float32 restatement %.3g, ratio %.2f"
        % (l, np.linalg.cond(Y.astype(np.float64)), e_gpu, e_ref, e_gpu / e_ref))
  assert e_gpu <= M_F32 * e_ref
  # the same column space, the same orientation: Q = Y R^-1 with R upper triangular, positive diagonal
  R = Q.T @ Y.astype(np.float64)
  assert np.abs(np.tril(R, -1)).max() <= 1e-4 * np.abs(R).max() and np.all(np.diag(R) > 0)


def test_chol_inverse_reports_a_breakdown_and_keeps_the_first():
  from recoder_amd import svd
  G = np.diag(np.float32([4.0, 0.0, 9.0, -1.0]))
  status = torch.zeros(1, dtype=torch.int32, device=DEV)
  Rinv = svd.chol_inverse(_t(G), status).cpu().numpy()
  assert int(status.item()) == 2                      # pivot 1, reported as k + 1
  assert np.array_equal(Rinv, np.diag(np.float32([0.5, 1.0, 1.0 / 3.0, 1.0])))
  svd.chol_inverse(_t(np.eye(3)), status)
  assert int(status.item()) == 2, "the status word is the caller's to clear"
  with pytest.raises(RuntimeError, match="numerical rank"):
    svd.orthonormalize(_t(np.ones((50, 3))).clone())


# ------------------------------------------------------------------------ fit
def _fit(A, h, oversample, q, om):
  from recoder_amd import svd
  uc, ic = _pair(A)
  U = torch.empty(A.shape[0], h, device=DEV)
  V = torch.empty(A.shape[1], h, device=DEV)
  info = svd.fit(U, V, uc, ic, oversample, q, 0, omega=om)
  return (np.asarray(info["singular_values"]), V.cpu().numpy(), U.cpu().numpy()), info


def _check_against_restatements(A, got, r64, r32, label):
  s_gpu, s_ref = svd_util.stats(A, got, r64), svd_util.stats(A, r32, r64)
  print("fit %s: gpu %s; float32 restatement %s" % (label, {k: "%.3g" % v for k, v in s_gpu.items()},
                                                    {k: "%.3g" % v for k, v in s_ref.items()}))
  for k in ("e_sigma", "e_orth", "e_sub"):
    assert s_gpu[k] <= M_F32 * max(s_ref[k], FLOOR), k
  assert s_gpu["e_U"] <= 1e-5


def test_fit_on_the_planted_matrix():
  A = svd_util.planted()
  om = svd_util.omega(A.shape[1], 24, 0)
  got, info = _fit(A, 8, 16, 4, om)
  assert info["h"] == 8 and info["l"] == 24 and info["nnz"] == A.nnz
  r64, r32 = (svd_util.rsvd(A, 8, 16, 4, om, dt) for dt in (np.float64, np.float32))
  _check_against_restatements(A, got, r64, r32, "planted")
  want = np.sort(scipy.sparse.linalg.svds(A.astype(np.float64), k=8, return_singular_vectors=False))[::-1]
  rel = np.abs(got[0] - want) / want
  print("planted: max relative sigma error against svds %.3g, ritz residual %.3g" % (rel.max(), info["ritz_residual"]))
  assert rel.max() <= 1e-5


@pytest.mark.parametrize("h,q", [(4, 6), (64, 6)])
def test_fit_on_the_slice(h, q):
  x, y = svd_util.load_slice()
  om = svd_util.omega(x.shape[1], h + 16, 0)
  got, info = _fit(x, h, 16, q, om)
  r64, r32 = (svd_util.rsvd(x, h, 16, q, om, dt) for dt in (np.float64, np.float32))
  _check_against_restatements(x, got, r64, r32, "slice h=%d q=%d" % (h, q))
  l_gpu = svd_util.top_k(svd_util.scores(got), x, 20)
  l_64 = svd_util.top_k(svd_util.scores(r64), x, 20)
  differ = svd_util.top20_differ(l_gpu, l_64)
  rec_gpu, rec_64, pop = svd_util.recall_at(l_gpu, y), svd_util.recall_at(l_64, y), svd_util.popularity_recall(x, y)
  print("slice h=%d q=%d: top-20 differ %.4f %%, Recall@20 gpu %.6f float64 %.6f popularity %.6f; "
        "spmm %.3f ms, orth %.3f ms, eig %.3f ms, ritz residual %.3g"
        % (h, q, 100 * differ, rec_gpu, rec_64, pop, info["spmm_ms"], info["orth_ms"], info["eig_ms"],
           info["ritz_residual"]))
  assert differ <= 5e-3
  assert abs(rec_gpu - rec_64) <= 1e-3
  if h == 4:
    # (rank matters on this sparse slice: at h = 64 the float64 restatement itself gives 0.0715 against
    # popularity's 0.1079, so the comparison with popularity is made at the rank that carries it)
    assert rec_gpu > pop


# ---------------------------------------------------------------- end to end
H = 4


def _recoder(h=H):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", loss_params={"confidence": 10.0}, optimizer_type="adam")


def _tables(rec):
  m = rec.model
  return (m.user_embedding_layer.weight.detach().cpu().numpy(), m.item_embedding_layer.weight.detach().cpu().numpy(),
          m.bias.detach().cpu().numpy())


@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  x, y = svd_util.load_slice()
  rec = _recoder()
  info = rec.train_svd(RecommendationDataset(x), seed=3)
  return rec, info, x, y


def test_train_svd_info_and_tables(fitted):
  rec, info, x, _ = fitted
  assert set(info) == {"h", "l", "nnz", "singular_values", "spmm_ms", "orth_ms", "eig_ms", "ritz_residual"}
  assert info == rec.svd_info
  assert info["h"] == H and info["l"] == H + 16 and info["nnz"] == x.nnz
  s = np.asarray(info["singular_values"])
  assert s.shape == (H,) and np.all(np.diff(s) < 0) and s[-1] > 0
  assert info["spmm_ms"] > 0 and info["orth_ms"] > 0 and info["eig_ms"] > 0
  U, V, b = _tables(rec)
  assert U.shape == (x.shape[0], H) and V.shape == (x.shape[1], H)
  assert b.shape == (x.shape[1],) and not b.any()
  V64 = V.astype(np.float64)
  assert np.abs(V64.T @ V64 - np.eye(H)).max() <= 1e-5
  assert np.linalg.norm(U - x.astype(np.float64) @ V64) <= 1e-5 * np.linalg.norm(U)
  want = np.sort(scipy.sparse.linalg.svds(x.astype(np.float64), k=H, return_singular_vectors=False))[::-1]
  print("train_svd on the slice: sigma %s (svds %s), ritz residual %.3g; spmm %.3f ms, orth %.3f ms, eig %.3f ms"
        % (np.round(s, 3), np.round(want, 3), info["ritz_residual"], info["spmm_ms"], info["orth_ms"], info["eig_ms"]))
  assert np.all(s <= want * (1 + 1e-5)), "Ritz values never exceed the singular values"


def test_train_svd_is_bitwise_repeatable_for_a_seed(fitted):
  from recoder_amd.data import RecommendationDataset
  rec, info, x, _ = fitted
  rec2 = _recoder()
  info2 = rec2.train_svd(RecommendationDataset(x), seed=3)
  for a, b in zip(_tables(rec), _tables(rec2)):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
  assert info2["singular_values"] == info["singular_values"]
  rec3 = _recoder()
  rec3.train_svd(RecommendationDataset(x), seed=4)
  assert not np.array_equal(_tables(rec3)[1], _tables(rec)[1])


def test_ritz_residual_falls_with_power_iterations(fitted):
  from recoder_amd.data import RecommendationDataset
  rec, info, x, _ = fitted
  rec0 = _recoder()
  info0 = rec0.train_svd(RecommendationDataset(x), num_power_iterations=0, seed=3)
  print("ritz residual: q = 0 %.3g, q = 6 %.3g" % (info0["ritz_residual"], info["ritz_residual"]))
  assert info["ritz_residual"] < info0["ritz_residual"]


def test_recommend_is_the_masked_top_k_of_the_tables(fitted):
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = fitted
  users = np.arange(1000)
  lists = rec.recommend_array(UsersInteractions(users, x[users]), 20)
  U, V, _ = _tables(rec)
  S = U[users].astype(np.float64) @ V.astype(np.float64).T
  want = svd_util.top_k(S, x[users], 20)
  same = float(np.mean([np.array_equal(a, b) for a, b in zip(lists, want)]))
  print("recommend: %.2f %% of 1000 lists identical to the float64 top-20 of U V^T" % (100 * same))
  masked = S.copy()
  for i, u in enumerate(users):
    seen = x.indices[x.indptr[u]:x.indptr[u + 1]]
    assert len(set(lists[i])) == 20 and not np.isin(lists[i], seen).any()
    masked[i, seen] = -np.inf
    # (the device scores in f32-class arithmetic: an item may trade places with one whose float64 score is
    # within that rounding of it)
    tol = 1e-5 * float(np.abs(U[u]).astype(np.float64) @ np.abs(V).max(axis=0))
    kth = np.partition(masked[i], -20)[-20]
    assert S[i, lists[i]].min() >= kth - tol
  assert same >= 0.9


def test_checkpoint_round_trip(fitted, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "svd"))
  rec2 = Recoder(model=MatrixFactorization(64))
  rec2.init_from_model_file(f)
  assert rec2.model.embedding_size == H
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))


def test_evaluate_beats_popularity(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import Recall
  rec, _, x, y = fitted
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=20, metrics=[Recall(k=20, normalize=True)],
                     batch_size=500)
  got = float(np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)))
  pop = svd_util.popularity_recall(x, y)
  print("train_svd (device RNG, h=4, q=6): Recall@20 %.4f, popularity %.4f" % (got, pop))
  assert got > pop


def test_adam_als_and_similarity_take_the_tables():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.embedding import ExactEmbeddingsIndex
  x, _ = svd_util.load_slice()
  rec = _recoder(32)
  rec.train_svd(RecommendationDataset(x), num_power_iterations=2, seed=1)
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
  before = _tables(rec)[1].copy()
  hist = rec.train_als(RecommendationDataset(x), num_iterations=1, reg=100.0, cg_steps=3)
  assert len(hist) == 1 and np.isfinite(hist[0])
  assert not np.array_equal(_tables(rec)[1], before)
  rec.train(RecommendationDataset(x), batch_size=500, lr=1e-3, num_epochs=1, negative_sampling=True)
  assert np.all(np.isfinite(rec.last_epoch_losses)) and len(rec.last_epoch_losses) == 20


def test_a_rank_deficient_matrix_raises():
  from recoder_amd.data import RecommendationDataset
  a = np.zeros((60, 50), np.float32)
  a[:30, :20] = 1.0
  a[30:, 20:] = 1.0
  assert np.linalg.matrix_rank(a) == 2
  rec = _recoder(4)
  with pytest.raises(RuntimeError, match="numerical rank is below embedding size \\+ oversample = 8"):
    rec.train_svd(RecommendationDataset(sp.csr_matrix(a)), oversample=4)
  # the process is usable afterwards
  rec2 = _recoder(2)
  info = rec2.train_svd(RecommendationDataset(sp.csr_matrix(np.eye(40, dtype=np.float32) + a[:40, :40])), oversample=2)
  assert len(info["singular_values"]) == 2
