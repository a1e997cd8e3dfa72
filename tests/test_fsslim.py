"""GPU: fsSLIM (rk_slim_fit_sparse of librecoder_slim.so, ``candidates=M`` of recoder_amd/slim.py and
``Recoder.train_slim``) against the restatements of tests/fsslim_util.py and tests/slim_util.py: bit for bit on
matrices whose products and sums are exact in f32 (binary, values in {0.5, 1, 2}), by the optimality conditions on
values that are not, and end to end on the ML-20M slice against tests/golden/fsslim_slice.json."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import fsslim_util as fu, slim_util
from tests.test_slim import _assert_bitwise, _dev_csr, _slice

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWEEPS, TOL, L1, L2 = 50, 1e-5, 1.0, 5.0
FILL = (7, 3.0, 9, -5, -6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsslim_slice.json")


@functools.lru_cache(maxsize=None)
def matrix(kind):
  """binary 300 x 97 and 500 x 130; "valued": the first with values in {0.5, 1, 2}; "uniform": values in (0, 2).
  Item 3 nobody holds, user 1 holds every item but 3, user 0 is empty."""
  users, n = (500, 130) if kind == "b130" else (300, 97)
  rng = np.random.RandomState(users + n)
  m = (rng.rand(users, n) < 0.12).astype(np.float32)
  m[1, :] = 1.0
  m[:, 3] = 0.0
  m[0, :] = 0.0
  if kind == "valued":
    m *= rng.choice(np.array([0.5, 1.0, 2.0], np.float32), m.shape)
  if kind == "uniform":
    m *= rng.uniform(0.05, 1.95, m.shape).astype(np.float32)
  X = sp.csr_matrix(m)
  X.sort_indices()
  return X


@functools.lru_cache(maxsize=None)
def edge_matrix():
  """1 100 users x 40 items: item 0 every user holds (a user list of 1 100: 18 pieces of 64 users, the last one
  short), user 0 holds every item but 5 and 6, item 5 nobody holds; the test gives item 6 one holder."""
  rng = np.random.RandomState(5)
  m = (rng.rand(1100, 40) < 0.1).astype(np.float32)
  m[:, 0] = 1.0
  m[0, :] = 1.0
  m[:, 5] = 0.0
  m[:, 6] = 0.0
  X = sp.csr_matrix(m)
  X.sort_indices()
  return X


def grams(X):
  G64 = slim_util.gram_f64(X)
  return G64.astype(np.float32), G64


def inv_of(G64, l2=L2):
  return slim_util.inv_denom_f64(G64, l2).astype(np.float32)


def gpu_sparse(X, cand, cnt, inv, l1, K, ranges=None, fill=None, max_sweeps=SWEEPS):
  """(ids, w, count, sweeps, support, screened) as numpy from rk_slim_fit_sparse over ``ranges``."""
  from recoder_amd import slim
  X = sp.csr_matrix(X)
  n = X.shape[1]
  ucsr, icsr = _dev_csr(X), _dev_csr(sp.csr_matrix(X.T))
  f = fill if fill is not None else (0, 0.0, 0, 0, 0)
  ids = torch.full((n, K), f[0], dtype=torch.int32, device=DEV)
  w = torch.full((n, K), f[1], dtype=torch.float32, device=DEV)
  count, sweeps, support = (torch.full((n,), v, dtype=torch.int32, device=DEV) for v in f[2:])
  screened = torch.full((n,), -9, dtype=torch.int32, device=DEV)
  c, k = torch.from_numpy(np.ascontiguousarray(cand)).to(DEV), torch.from_numpy(cnt).to(DEV)
  iv = torch.from_numpy(inv).to(DEV)
  for lo, hi in (ranges if ranges is not None else [(0, n)]):
    slim.fit_columns_sparse(ucsr, icsr, c, k, iv, l1, ids, w, count, sweeps, support, max_sweeps, TOL, lo, hi,
                            screened=screened)
  return tuple(t.cpu().numpy() for t in (ids, w, count, sweeps, support, screened))


# ------------------------------------------------------------------- kernel
@pytest.mark.parametrize("kind", ["b97", "b130", "valued"])
def test_full_candidates_equal_the_dense_kernel_and_cd_f32(kind):
  from recoder_amd import ease, slim
  X = matrix(kind)
  n = X.shape[1]
  G32, G64 = grams(X)
  K = 16
  inv = inv_of(G64)
  cand, cnt = fu.all_candidates(n)
  got = gpu_sparse(X, cand, cnt, inv, L1, K, fill=FILL)
  want = slim_util.cd_f32(G32, inv, L1, K, SWEEPS, TOL)
  _assert_bitwise(got[:5], want, kind + " against cd_f32")
  assert want[4].max() > K and want[2][3] == 0, "the cut must bind; the item nobody holds has an empty column"
  ucsr, icsr = _dev_csr(X), _dev_csr(sp.csr_matrix(X.T))
  G = ease.gram(ucsr, icsr, 0.0)
  assert np.array_equal(G.cpu().numpy(), G32)
  ids = torch.empty(n, K, dtype=torch.int32, device=DEV)
  w = torch.empty(n, K, dtype=torch.float32, device=DEV)
  count, sweeps, support = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
  slim.fit_columns(G, torch.from_numpy(inv).to(DEV), L1, ids, w, count, sweeps, support, SWEEPS, TOL)
  _assert_bitwise(got[:5], tuple(t.cpu().numpy() for t in (ids, w, count, sweeps, support)), kind + " against rk_slim_fit")
  assert np.array_equal(got[5], [len(slim_util.candidates(G64, j, L1)) for j in range(n)])


def _lds():
  from recoder_amd import _slim_lib, slim
  lds = _slim_lib.load().rk_slim_sparse_lds_candidates()
  assert lds == slim.SPARSE_LDS_CANDIDATES
  return lds


RESTRICTED = [("b97", 1), ("b97", 8), ("b97", 63), ("b97", 64), ("b97", 65), ("valued", 8), ("valued", 65),
              ("b130", "lds"), ("b130", "lds+1")]


@pytest.mark.parametrize("kind, M", RESTRICTED)
def test_restricted_candidates_equal_the_masked_restatement(kind, M):
  """The lists go to the kernel directly.  At l1 = 0 every candidate passes the screen, so the columns on either
  side of rk_slim_sparse_lds_candidates() run over that many candidates."""
  from recoder_amd import _slim_lib, slim
  lds = _lds()
  M = {"lds": lds, "lds+1": lds + 1}.get(M, M)
  l1 = 0.0 if kind == "b130" else L1
  X = matrix(kind)
  G32, G64 = grams(X)
  inv = inv_of(G64)
  cand, cnt = fu.select(X, M)
  assert cnt.max() == M and cnt[3] == 0
  K = 12
  got = gpu_sparse(X, cand, cnt, inv, l1, K, fill=FILL)
  want = fu.cd_f32(G32, inv, cand, cnt, l1, K, SWEEPS, TOL)
  _assert_bitwise(got[:5], want, "%s M=%d" % (kind, M))
  assert np.array_equal(got[5], fu.screened(G64, cand, cnt, l1))
  if kind == "b130":
    assert got[5].max() == M, "a column must run over all M candidates"
    assert _slim_lib.load().rk_slim_fit_sparse_workspace_bytes(M) == slim.sparse_workspace_bytes(M)
    assert (slim.sparse_workspace_bytes(M) > 256) == (M > lds)
  if M >= 63:
    assert want[4].max() > K, "the cut must bind"


@pytest.mark.parametrize("M", [20, 65])
def test_non_dyadic_values_equal_the_ascending_chains_bit_for_bit(M):
  """Values in (0, 2): the sums round, so the bits depend on the order of every chain of L and q.  The restatement
  makes each entry by the header's ascending fmaf chain over the users (``fu.local_chain_f32``); a walk in another
  order, or a product summed another way, gives other bits."""
  X = matrix("uniform")
  G32, G64 = grams(X)
  inv = inv_of(G64)
  cand, cnt = fu.select(X, M)
  XXt = fu.chains(X)
  # (the data must be able to tell: the chain differs from the rounded float64 Gram somewhere)
  items, jl, sub = fu.local_chain_f32(XXt, 7, cand[7, :cnt[7]])
  assert (sub != fu.local(G32, 7, cand[7, :cnt[7]])[2])[np.arange(len(items)) != jl].any()
  got = gpu_sparse(X, cand, cnt, inv, 0.5, 12, fill=FILL)
  want = fu.cd_f32(XXt, inv, cand, cnt, 0.5, 12, SWEEPS, TOL)
  _assert_bitwise(got[:5], want, "uniform values, M=%d" % M)
  assert want[4].max() > 12 and want[3].max() > 2


def test_cut_ties_go_to_the_lower_ids():
  """tests/test_slim.py's tie construction through the sparse kernel: item 0 is held by every user, items 1..70 by
  disjoint groups of three users (items 40 and 66 by four), so the candidates of column 0 never meet, every weight is
  (G_0k - l1) * inv_denom[k] with two distinct values, and the cut falls inside the tie."""
  n, l1, l2 = 80, 1.0, 2.0
  size = {k: 4 if k in (40, 66) else 3 for k in range(1, 71)}
  D = np.zeros((sum(size.values()), n), np.float32)
  D[:, 0] = 1.0
  u = 0
  for k, c in size.items():
    D[u:u + c, k] = 1.0
    u += c
  X = sp.csr_matrix(D)
  G32, G64 = grams(X)
  inv = inv_of(G64, l2)
  cand, cnt = fu.all_candidates(n)
  for K, kept in ((5, [1, 2, 3, 40, 66]), (66, list(range(1, 67))), (1, [40])):
    got = gpu_sparse(X, cand, cnt, inv, l1, K, fill=FILL)
    _assert_bitwise(got[:5], slim_util.cd_f32(G32, inv, l1, K, SWEEPS, TOL), "ties, K=%d" % K)
    assert got[4][0] == 70 and list(got[0][0, :got[2][0]]) == kept
    assert len(set(got[1][0, :got[2][0]].tolist())) <= 2, "the kept weights tie"


def test_driver_candidates_are_the_restated_selection():
  from recoder_amd import als, slim
  for kind, M, sim, shrink in (("b97", 8, "cosine", 0.0), ("valued", 20, "cosine", 3.0), ("b130", 105, "cosine", 0.0)):
    X = matrix(kind)
    pair = als.csr_pair(X, X.shape[0], X.shape[1], DEV)
    ids, count, _ = slim.candidate_lists(pair, M, sim, shrink)
    want_ids, want_count = fu.select(X, M, sim, shrink)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(count.cpu().numpy(), want_count)
    live = np.arange(M)[None, :] < want_count[:, None]
    assert np.all(np.diff(want_ids.astype(np.int64), axis=1)[live[:, 1:]] > 0)
    # the diagonal the driver makes is the Gram's
    assert np.array_equal(slim.diagonal(pair[1]), np.diag(grams(X)[0]))


def test_column_ranges_canaries_and_repeatability():
  X = matrix("b130")
  n = X.shape[1]
  G32, G64 = grams(X)
  inv = inv_of(G64)
  cand, cnt = fu.select(X, 105)
  whole = gpu_sparse(X, cand, cnt, inv, 0.0, 12, fill=FILL)
  again = gpu_sparse(X, cand, cnt, inv, 0.0, 12, fill=FILL)
  ragged = gpu_sparse(X, cand, cnt, inv, 0.0, 12, ranges=[(41, 130), (0, 7), (7, 41), (50, 50)], fill=FILL)
  _assert_bitwise(again, whole, "second run")
  _assert_bitwise(ragged, whole, "ragged ranges")
  part = gpu_sparse(X, cand, cnt, inv, 0.0, 12, ranges=[(7, 41)], fill=FILL)
  out = np.r_[0:7, 41:n]
  assert np.all(part[0][out] == FILL[0]) and np.all(part[1][out] == FILL[1])
  assert all(np.all(part[i][out] == FILL[i]) for i in (2, 3, 4)) and np.all(part[5][out] == -9)
  _assert_bitwise(tuple(a[7:41] for a in part), tuple(a[7:41] for a in whole), "the range itself")


def test_edge_rows():
  X = edge_matrix()
  n = X.shape[1]
  G32, G64 = grams(X)
  inv = inv_of(G64)
  assert G64[0, 0] == 1100 and G64[5, 5] == 0 and G64[6, 6] == 0
  # item 6 gets one holder: with item 0 and nothing else in common beyond that user, every q of its column is 1 <= l1
  Xl = X.tolil()
  Xl[7, :] = 0
  Xl[7, 0] = Xl[7, 6] = 1.0
  X = sp.csr_matrix(Xl)
  X.sort_indices()
  G32, G64 = grams(X)
  inv = inv_of(G64)
  assert G64[6].max() == 1 and G64[6, 0] == 1
  K = 4
  cand, cnt = fu.all_candidates(n)
  cnt[9] = 0                                            # (a column without candidates; the others have M of them)
  got = gpu_sparse(X, cand, cnt, inv, L1, K, fill=FILL)
  want = fu.cd_f32(G32, inv, cand, cnt, L1, K, SWEEPS, TOL)
  _assert_bitwise(got[:5], want, "edge rows")
  ids, w, count, sweeps, support, screened = got
  assert count[5] == 0 and sweeps[5] == 0 and screened[5] == 0, "an item nobody holds"
  assert count[6] == 0 and sweeps[6] == 0 and screened[6] == 0, "every candidate at or below l1"
  assert count[9] == 0 and sweeps[9] == 0 and np.all(ids[9] == -1) and not w[9].any(), "cand_count 0"
  assert screened[0] >= 30 and sweeps[0] >= 1, "the item every user holds"
  assert (support > K).sum() >= 5 and count.max() == K, "the cut binds"
  # the cut's tie order: the K largest by (w descending, id ascending), stored ascending
  full = fu.cd_f32(G32, inv, cand, cnt, L1, n, SWEEPS, TOL)
  for j in np.flatnonzero(support > K)[:5]:
    kid, kw = slim_util.cut(full[0][j, :full[2][j]], full[1][j, :full[2][j]], K)
    assert np.array_equal(ids[j], kid) and np.array_equal(w[j], kw)


def test_a_user_who_holds_every_item():
  """Every item has a holder and user 2 holds them all: every pair of items co-occurs, and that user's row is longer
  than a wave (70 items), so one user step takes two rounds of the lanes."""
  rng = np.random.RandomState(9)
  m = (rng.rand(150, 70) < 0.1).astype(np.float32)
  m[2, :] = 1.0
  X = sp.csr_matrix(m)
  assert X[2].nnz == 70 and (slim_util.gram_f64(X) > 0).all()
  G32, G64 = grams(X)
  inv = inv_of(G64)
  cand, cnt = fu.select(X, 30)
  got = gpu_sparse(X, cand, cnt, inv, L1, 8, fill=FILL)
  _assert_bitwise(got[:5], fu.cd_f32(G32, inv, cand, cnt, L1, 8, SWEEPS, TOL), "a user with every item")
  assert cnt.min() == 30 and got[5].max() > 8


# the KKT residual of the restatement's f32 model on the masked float64 Gram of matrix("uniform") at M = 20, measured
# on the CPU (``fu.cd_f32`` on the float64 Gram rounded to f32); the kernel is asserted at 4 x that, as
# tests/test_slim.py holds rk_slim_fit to 4 x what it measured for ``cd_f32``
UNIFORM_KKT = 3.566e-4


def test_non_dyadic_values_meet_the_optimality_conditions():
  X = matrix("uniform")
  n = X.shape[1]
  G32, G64 = grams(X)
  M, l1, l2 = 20, 0.5, 5.0
  cand, cnt = fu.select(X, M)
  got = gpu_sparse(X, cand, cnt, inv_of(G64, l2), l1, M, max_sweeps=200)
  assert np.array_equal(got[2], got[4]), "uncut"
  W = slim_util.dense(got[0], got[1].astype(np.float64), got[2])
  res = fu.kkt_residual(G64, cand, cnt, W, l1, l2, range(n))
  W64, _ = fu.cd_f64(G64, cand, cnt, l1, l2, 200, TOL)
  gap = float(np.abs(W - W64.toarray()).max())
  print("uniform values: KKT residual %.4g (measured for cd_f32: %.4g), max |W - W64| %.3g" % (res, UNIFORM_KKT, gap))
  assert res <= 4 * UNIFORM_KKT


def test_refusals_before_a_launch():
  from recoder_amd import _slim_lib
  from recoder_amd._lib import ptr
  lib = _slim_lib.load()
  X = matrix("b97")
  n = X.shape[1]
  ucsr, icsr = _dev_csr(X), _dev_csr(sp.csr_matrix(X.T))
  M, K = 8, 4
  cand = torch.full((n, 1024), -1, dtype=torch.int32, device=DEV)
  cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
  inv = torch.zeros(n, dtype=torch.float32, device=DEV)
  ids = torch.full((n, K), 7, dtype=torch.int32, device=DEV)
  w = torch.zeros(n, K, device=DEV)
  c3 = [torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(3)]
  ws = torch.empty(lib.rk_slim_fit_sparse_workspace_bytes(1024) + 512, dtype=torch.uint8, device=DEV)
  assert ws.data_ptr() % 256 == 0

  def call(M=M, lo=0, hi=n, ws_ptr=ptr(ws), ws_bytes=ws.numel()):
    return lib.rk_slim_fit_sparse(ptr(icsr.indptr), ptr(icsr.indices), None, ptr(ucsr.indptr), ptr(ucsr.indices), None,
                                  X.shape[0], n, ptr(cand), ptr(cnt), M, ptr(inv), 1.0, K, 5, 1e-5, lo, hi, ptr(ids),
                                  ptr(w), ptr(c3[0]), ptr(c3[1]), ptr(c3[2]), None, ws_ptr, ws_bytes, None)
  for kw, text in ((dict(M=0), "M outside"), (dict(M=1025), "M outside"), (dict(ws_ptr=ptr(ws) + 4), "aligned"),
                   (dict(M=200, ws_bytes=256), "workspace too small"), (dict(lo=5, hi=4), "column range")):
    assert call(**kw) < 0
    assert text in lib.rk_slim_last_error().decode(), kw
  assert lib.rk_slim_fit_sparse_workspace_bytes(0) < 0 and lib.rk_slim_fit_sparse_workspace_bytes(1025) < 0
  torch.cuda.synchronize()
  assert bool((ids == 7).all()), "a refused call launches nothing"
  assert call() == 0 and call(lo=4, hi=4) == 0
  torch.cuda.synchronize()
  assert bool((ids == -1).all())


# ---------------------------------------------------------------- end to end
def test_train_slim_with_candidates_on_the_slice(tmp_path):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.metrics import Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  with open(GOLDEN) as f:
    golden = json.load(f)
  p = golden["params"]
  x, y = _slice()
  n = x.shape[1]
  rec = Recoder(model=SparseLinearModel(p["l1_reg"], p["l2_reg"], p["neighbours"]))
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  info = rec.train_slim(RecommendationDataset(x), max_sweeps=p["max_sweeps"], tol=p["tol"],
                        candidates=p["candidates"], candidate_similarity=p["candidate_similarity"],
                        candidate_shrink=p["candidate_shrink"])
  peak = torch.cuda.max_memory_allocated() - base
  print("fsSLIM on the slice: %s; peak %d bytes (n x n x 4 = %d)" % (info, peak, n * n * 4))
  assert peak < n * n * 4
  assert {"candidates", "candidate_ms", "mean_candidates", "fit_ms", "kept"} <= set(info)
  assert info["candidates"] == 100 and info["candidate_ms"] > 0
  assert abs(info["mean_candidates"] - golden["f32"]["mean_candidates"]) < 1e-9
  assert abs(info["kept"] / (n * n) - golden["f32"]["density"]) < 1e-12
  assert rec.model.model_params()["candidates"] == 100
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100, metrics=[Recall(k=20, normalize=True)],
                     batch_size=500)
  r20 = float(np.nanmean(np.asarray(next(iter(res.values())), np.float64)))
  diff = abs(golden["recall20_f32_minus_f64"])
  tol = 2 * diff if diff > 0 else 5e-7                   # (measured 0: the kernels restate cd_f32, six digits)
  print("Recall@20 %.6f, cd_f32 restatement %.6f, tolerance %.3g" % (r20, golden["f32"]["recall20"], tol))
  assert abs(r20 - golden["f32"]["recall20"]) <= tol
  users = np.arange(40)
  inp = UsersInteractions(users, x[users])
  top = np.asarray(rec.recommend_array(inp, 20))
  assert top.shape == (40, 20)
  path = rec.save_state(str(tmp_path / "fsslim"))
  rec2 = Recoder(model=SparseLinearModel())
  rec2.init_from_model_file(path)
  assert rec2.model.model_params() == rec.model.model_params()
  assert np.array_equal(np.asarray(rec2.recommend_array(inp, 20)), top)
