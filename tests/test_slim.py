"""GPU: SLIM (recoder_amd/slim.py, librecoder_slim.so, SparseLinearModel) against the restatements of
tests/slim_util.py -- the fit bit for bit against the f32 coordinate-descent chains (ids, weights, counts,
sweeps, supports; both state paths; column ranges), against the same sweeps in float64, the scores bit for
bit against the fmaf chain, and ``Recoder.train_slim`` end to end on a synthetic catalogue and on the
ML-20M slice with what the fitted model plugs into (recommend, evaluate, checkpoints, predict).

G of the kernel tests is made on the host (exact: binary data, integer entries far below 2^24) and uploaded,
so that they do not depend on the Gram kernel; the end-to-end tests take ``ease.gram``'s."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import rp3_util, slim_util
from tests.test_slim_host import case

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWEEPS, TOL = 50, 1e-5
FILL = (7, 3.0, 9, -5, -6)

# (n, l1, l2, K) of the issue's table
CASES = [(1, 1.0, 5.0, 1), (37, 1.0, 5.0, 64), (37, 0.0, 5.0, 64), (37, 1.0, 5.0, 5), (41, 0.5, 1.0, 5),
         (67, 2.0, 10.0, 64)]


def _slice():
  z = np.load(slim_util.SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def _dev_csr(m):
  from recoder_amd.als import AlsCSR
  return AlsCSR(sp.csr_matrix(m), DEV)


@functools.lru_cache(maxsize=None)
def _gram(n):
  """(G f32 exact, its float64 image) of the random graph ``case(n)``."""
  G = slim_util.gram_f64(case(n))
  assert G.max() < 2 ** 24
  return G.astype(np.float32), G


def _inv(G64, l2):
  """inv_denom as the fit is given it: float64 rounded once (the comparator's own)."""
  return slim_util.inv_denom_f64(G64, l2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _restated(n, l1, l2, K, max_sweeps=SWEEPS):
  G32, G64 = _gram(n)
  return slim_util.cd_f32(G32, _inv(G64, l2), l1, K, max_sweeps, TOL)


def _gpu_fit(G32, inv, l1, K, max_sweeps=SWEEPS, tol=TOL, ranges=None, fill=None):
  """(ids, w, count, sweeps, support) as numpy from rk_slim_fit over ``ranges`` (default: every column)."""
  from recoder_amd import slim
  n = G32.shape[0]
  G = torch.from_numpy(np.ascontiguousarray(G32)).to(DEV)
  iv = torch.from_numpy(inv).to(DEV)
  f = fill if fill is not None else (0, 0.0, 0, 0, 0)
  ids = torch.full((n, K), f[0], dtype=torch.int32, device=DEV)
  w = torch.full((n, K), f[1], dtype=torch.float32, device=DEV)
  count, sweeps, support = (torch.full((n,), v, dtype=torch.int32, device=DEV) for v in f[2:])
  for lo, hi in (ranges if ranges is not None else [(0, n)]):
    slim.fit_columns(G, iv, l1, ids, w, count, sweeps, support, max_sweeps, tol, lo, hi)
  return tuple(t.cpu().numpy() for t in (ids, w, count, sweeps, support))


def _assert_bitwise(got, want, what=""):
  for g, t, name in zip(got, want, ("ids", "weights", "counts", "sweeps", "supports")):
    assert g.dtype == t.dtype and g.shape == t.shape
    same = g.view(np.uint32) == t.view(np.uint32) if g.dtype == np.float32 else g == t
    assert same.all(), "%s %s: %d entries differ, first at %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])


def _assert_layout(ids, w, count, n, K):
  live = np.arange(K)[None, :] < count[:, None]
  assert np.all(ids[~live] == -1) and np.all(w[~live].view(np.uint32) == 0), "padding must be -1 / +0"
  assert np.all(w[live] > 0)
  assert np.all(np.diff(ids.astype(np.int64), axis=1)[live[:, 1:]] > 0), "ids ascending inside a column"
  assert np.all(ids[live] != np.nonzero(live)[0]), "the diagonal is never kept"
  if n > 1:
    assert count[n // 2] == 0 and not np.any(ids == n // 2), "an item nobody holds: an empty column, in no column"


def f64_gap(n, l1, l2, model):
  """(max |W32 - W64|, support flips at weights above that gap) of an uncut f32 model against ``cd_f64`` run
  for the same number of sweeps per column."""
  ids, w, count, sweeps, support = model
  assert np.array_equal(count, support), "the comparison needs the uncut columns"
  W32 = slim_util.dense(ids, w, count).astype(np.float64)
  W64, _ = slim_util.cd_f64(_gram(n)[1], l1, l2, SWEEPS, TOL, sweeps=sweeps)
  gap = float(np.abs(W32 - W64).max())
  flips = ((W32 > 0) != (W64 > 0)) & (np.maximum(W32, W64) > gap)
  return gap, int(flips.sum())


# ----------------------------------------------------------------------- fit
@pytest.mark.parametrize("n, l1, l2, K", CASES)
def test_fit_is_the_f32_restatement_bit_for_bit(n, l1, l2, K):
  G32, G64 = _gram(n)
  want = _restated(n, l1, l2, K)
  got = _gpu_fit(G32, _inv(G64, l2), l1, K, fill=FILL)
  _assert_bitwise(got, want, "n=%d l1=%g K=%d" % (n, l1, K))
  ids, w, count, sweeps, support = got
  _assert_layout(ids, w, count, n, K)
  cands = np.array([len(slim_util.candidates(G64, j, l1)) for j in range(n)])
  assert np.all(sweeps[cands == 0] == 0) and np.all(sweeps[cands > 0] >= 1) and sweeps.max() <= SWEEPS
  assert np.array_equal(count, np.minimum(support, K))
  print("n=%d l1=%g l2=%g K=%d: candidates up to %d, supports up to %d, sweeps up to %d, %d columns cut"
        % (n, l1, l2, K, cands.max(), support.max(), sweeps.max(), (support > K).sum()))
  if n == 1:
    assert count[0] == 0
  if (n, K) == (37, 64):
    assert support.max() < K and support.max() >= 30
    if l1 == 0:
      assert np.array_equal(cands, (G64 > 0).sum(1) - (np.diag(G64) > 0)), "every co-occurring item is a candidate"
  if K == 5:
    assert (support > K).sum() >= 5, "the cut must bind"
    # columns whose K-th weight also occurs among the entries that were cut: the rule (lower ids win) at work
    _, allw, allc, _, _ = _restated(n, l1, l2, 64)
    tied = sum(1 for j in range(n) if support[j] > K and
               (allw[j, :allc[j]] == w[j, :K].min()).sum() > (w[j, :K] == w[j, :K].min()).sum())
    print("n=%d: columns whose K-th weight is tied across the cut: %d" % (n, tied))
  if n == 67:
    assert cands.max() > 64, "candidate counts past one wave"


def test_cut_ties_go_to_the_lower_ids():
  """Weights that tie exactly at the cut: item 0 is held by every user, items 1..70 by disjoint groups of three
  users (items 40 and 66 by four), so the candidates of column 0 never meet each other, q is never touched and
  every weight is (G_0k - l1) * inv_denom[k] with two distinct values.  K = 5 keeps the two heavier items and
  the three lowest ids of the tie; K = 66 crosses a wave."""
  n, l1, l2 = 80, 1.0, 2.0
  size = {k: 4 if k in (40, 66) else 3 for k in range(1, 71)}
  D = np.zeros((sum(size.values()), n), np.float32)
  D[:, 0] = 1.0
  u = 0
  for k, c in size.items():
    D[u:u + c, k] = 1.0
    u += c
  G64 = slim_util.gram_f64(sp.csr_matrix(D))
  G32, inv = G64.astype(np.float32), _inv(G64, l2)
  for K, kept in ((5, [1, 2, 3, 40, 66]), (66, list(range(1, 67))), (70, list(range(1, 71))), (1, [40])):
    want = slim_util.cd_f32(G32, inv, l1, K, SWEEPS, TOL)
    got = _gpu_fit(G32, inv, l1, K, fill=FILL)
    _assert_bitwise(got, want, "ties, K=%d" % K)
    assert got[4][0] == 70 and got[3][0] == 2 and list(got[0][0, :got[2][0]]) == kept
    assert len(set(got[1][0, :got[2][0]].tolist())) <= 2


def test_the_sweep_cap_binds():
  n, l1, l2, K = 37, 1.0, 5.0, 64
  G32, G64 = _gram(n)
  full = _restated(n, l1, l2, K)
  want = _restated(n, l1, l2, K, 3)
  got = _gpu_fit(G32, _inv(G64, l2), l1, K, max_sweeps=3, fill=FILL)
  _assert_bitwise(got, want, "max_sweeps=3")
  late = full[3] > 3
  assert late.sum() >= n // 2, "the cap must bind"
  assert np.all(got[3][late] == 3) and np.all(got[3][~late] == full[3][~late])


def test_fit_workspace_path_bit_for_bit():
  """A column with more candidates than rk_slim_lds_candidates(): its state lives in the workspace, the
  result is the restatement's all the same.  A block of 40 users holds the first 1 100 items, 150 users
  hold a few items each: the block's columns have 1 099 candidates, the others none.  Three
  sweeps and a sample of the columns keep the restatement cheap."""
  from recoder_amd import _slim_lib
  lds = _slim_lib.load().rk_slim_lds_candidates()
  n, big, K, l1, l2, sweeps = lds + 300, lds + 140, 20, 2.0, 30.0, 3
  rng = np.random.RandomState(5)
  D = np.zeros((190, n), np.float32)
  D[:40, :big] = rng.rand(40, big) < 0.9
  D[:5, :big] = 1.0                                        # (five users hold all of the block: G >= 5 > l1 inside it)
  D[40:] = rng.rand(150, n) < 0.004
  G64 = slim_util.gram_f64(sp.csr_matrix(D))
  G32 = G64.astype(np.float32)
  inv = _inv(G64, l2)
  cands = np.array([len(slim_util.candidates(G64, j, l1)) for j in range(n)])
  assert cands.max() == big - 1 > lds and (cands <= lds).sum() >= 100
  cols = [0, 1, 517, big - 1, big, big + 7, n - 1]
  want = slim_util.cd_f32(G32, inv, l1, K, sweeps, TOL, cols=cols)
  assert (want[4][cols] > K).sum() >= 3, "the cut must bind on the workspace path too"
  got = _gpu_fit(G32, inv, l1, K, max_sweeps=sweeps, fill=FILL)
  _assert_bitwise([a[cols] for a in got], [a[cols] for a in want], "workspace path")
  _assert_layout(got[0], got[1], got[2], 1, K)
  again = _gpu_fit(G32, inv, l1, K, max_sweeps=sweeps)
  _assert_bitwise(again, got, "workspace path, second call")
  part = _gpu_fit(G32, inv, l1, K, max_sweeps=sweeps, ranges=[(5, 777), (777, n - 3)], fill=FILL)
  _assert_bitwise([a[5:n - 3] for a in part], [a[5:n - 3] for a in got], "workspace path, ranges")
  for a, f in zip(part, FILL):
    assert np.all(a[:5] == f) and np.all(a[n - 3:] == f)


@pytest.mark.parametrize("n, l1, l2, K", [(37, 1.0, 5.0, 5), (67, 2.0, 10.0, 64)])
def test_column_ranges_give_the_columns_of_the_full_call(n, l1, l2, K):
  G32, G64 = _gram(n)
  inv = _inv(G64, l2)
  full = _gpu_fit(G32, inv, l1, K)
  _assert_bitwise(full, _restated(n, l1, l2, K), "full call")
  _assert_bitwise(_gpu_fit(G32, inv, l1, K), full, "second call")
  a, b = 3, 20
  split = _gpu_fit(G32, inv, l1, K, ranges=[(b, n), (0, a), (a, b)], fill=FILL)
  _assert_bitwise(split, full, "three ranges")
  part = _gpu_fit(G32, inv, l1, K, ranges=[(a, b), (b, b)], fill=FILL)
  _assert_bitwise([t[a:b] for t in part], [t[a:b] for t in full], "one range")
  for t, f in zip(part, FILL):
    assert np.all(t[:a] == f) and np.all(t[b:] == f), "columns outside the range must be left untouched"


# what cd_f32 (= the kernel, bit for bit) differs from cd_f64 by on these inputs, measured on the CPU
F64_GAP = {(37, 1.0): 2.061e-07, (37, 0.0): 1.333e-07, (41, 0.5): 6.914e-07, (67, 2.0): 2.564e-07}


@pytest.mark.parametrize("n, l1, l2", [(37, 1.0, 5.0), (37, 0.0, 5.0), (41, 0.5, 1.0), (67, 2.0, 10.0)])
def test_fit_against_the_same_sweeps_in_float64(n, l1, l2):
  """max |W32 - W64| of the uncut model against ``cd_f64`` with the same sweeps per column, and no support
  flip above it.  Measured for ``cd_f32`` on the CPU on exactly these inputs (the kernel equals it bit for
  bit): MEASURED_GAPS; asserted at 4 x the measured value."""
  G32, G64 = _gram(n)
  got = _gpu_fit(G32, _inv(G64, l2), l1, 128)
  gap, flips = f64_gap(n, l1, l2, got)
  print("n=%d l1=%g: max |W32 - W64| %.3g (measured for cd_f32: %.3g), flips %d" % (n, l1, gap, F64_GAP[n, l1], flips))
  assert flips == 0
  assert gap <= 4 * F64_GAP[n, l1]


# -------------------------------------------------------------------- scores
def test_scores_are_the_ascending_fmaf_chain():
  from recoder_amd import slim
  n, l1, l2, K = 67, 2.0, 10.0, 64
  X = case(n)
  ids, w, count, _, _ = _restated(n, l1, l2, K)
  tid, tw, tc = (torch.from_numpy(a).to(DEV) for a in (ids, w, count))
  base = sp.vstack([sp.csr_matrix((1, n), dtype=np.float32), X[5:40], sp.csr_matrix(np.ones((1, n), np.float32))]).tocsr()
  base.sort_indices()
  vals = base.copy()
  vals.data = (vals.data * np.random.RandomState(0).choice([1.0, 0.5, 3.0, -2.0], vals.nnz)).astype(np.float32)
  # (row 3 once more at position 36: the same user, values included, at two batch positions)
  plain = sp.vstack([base[:36], base[3:4], base[36:]]).tocsr()
  sub = sp.vstack([vals[:36], vals[3:4], vals[36:]]).tocsr()
  assert np.diff(plain.indptr)[0] == 0 and np.diff(plain.indptr)[-1] == n and np.diff(plain.indptr)[3] > 0
  csr = _dev_csr(sub)
  assert csr.data is not None
  got = slim.scores(csr, tid, tw, tc).cpu().numpy()
  want = slim_util.scores_f32(sub, ids, w, count)
  assert got.shape == want.shape == (plain.shape[0], n)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  assert np.all(got[0].view(np.uint32) == 0), "an empty user row gives all +0"
  assert np.array_equal(got[3].view(np.uint32), got[36].view(np.uint32)), "the same user at two batch positions"
  assert np.abs(got).max() > 0.1
  # a strip gives bitwise the columns of the full call
  for lo, hi in ((0, 1), (31, 33), (5, n), (n - 1, n), (n // 2, n // 2 + 1)):
    part = slim.scores(csr, tid, tw, tc, lo, hi).cpu().numpy()
    assert part.shape == (plain.shape[0], hi - lo)
    assert np.array_equal(part.view(np.uint32), got[:, lo:hi].view(np.uint32)), (lo, hi)
  rev = slim.scores(_dev_csr(sub[::-1]), tid, tw, tc).cpu().numpy()
  assert np.array_equal(rev[::-1].view(np.uint32), got.view(np.uint32))
  # unit values: the NULL data path
  c1 = _dev_csr(plain)
  assert c1.data is None
  assert np.array_equal(slim.scores(c1, tid, tw, tc).cpu().numpy().view(np.uint32),
                        slim_util.scores_f32(plain, ids, w, count).view(np.uint32))
  # out with a leading dimension: columns past the strip are left alone
  out = torch.full((plain.shape[0], 96), 5.0, device=DEV)
  slim.scores(csr, tid, tw, tc, 10, 51, out=out)
  out = out.cpu().numpy()
  assert np.array_equal(out[:, :41].view(np.uint32), got[:, 10:51].view(np.uint32)) and np.all(out[:, 41:] == 5.0)


def test_scores_over_more_than_one_tile_of_columns():
  """A model of 700 columns (three tiles of the kernel's 256) with made-up neighbours of every count from 0
  to K, a strip that starts and ends inside a tile."""
  from recoder_amd import slim
  n, K = 700, 9
  rng = np.random.RandomState(3)
  count = (np.arange(n) % (K + 1)).astype(np.int32)
  ids = np.full((n, K), -1, np.int32)
  w = np.zeros((n, K), np.float32)
  for j in range(n):
    ids[j, :count[j]] = np.sort(rng.choice(n, count[j], replace=False))
    w[j, :count[j]] = rng.rand(count[j]).astype(np.float32) + 0.01
  X = sp.random(30, n, density=0.1, random_state=7, format="csr", dtype=np.float32)
  X.data[:] = rng.choice([1.0, 2.0, 0.25], X.nnz)
  X.sort_indices()
  tid, tw, tc = (torch.from_numpy(a).to(DEV) for a in (ids, w, count))
  want = slim_util.scores_f32(X, ids, w, count)
  got = slim.scores(_dev_csr(X), tid, tw, tc).cpu().numpy()
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got != 0).mean() > 0.05
  part = slim.scores(_dev_csr(X), tid, tw, tc, 100, 613).cpu().numpy()
  assert np.array_equal(part.view(np.uint32), want[:, 100:613].view(np.uint32))


# ------------------------------------------------ end to end: a small catalogue
SYN = dict(users=500, n=300, l1=3.0, l2=20.0, K=8)


@functools.lru_cache(maxsize=None)
def _synthetic():
  x = rp3_util.graph_matrix(SYN["users"], SYN["n"], 0.05, seed=21, empty=(0, 250), full=100, none=150)
  y = rp3_util.graph_matrix(SYN["users"], SYN["n"], 0.02, seed=22, empty=(3,))
  y = sp.csr_matrix(y - y.multiply(x))          # (held-out items are unseen ones)
  y.eliminate_zeros()
  return x, y


@functools.lru_cache(maxsize=None)
def _syn_restated(K):
  x, _ = _synthetic()
  G = slim_util.gram_f64(x)
  return slim_util.cd_f32(G.astype(np.float32), _inv(G, SYN["l2"]), SYN["l1"], K, SWEEPS, TOL)


@pytest.fixture(scope="module")
def syn():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  x, y = _synthetic()
  rec = Recoder(model=SparseLinearModel(SYN["l1"], SYN["l2"], SYN["K"]))
  info = rec.train_slim(RecommendationDataset(x))
  return rec, info, x, y


def _model_arrays(m):
  return m.item_neighbours.cpu().numpy(), m.item_weights.data.cpu().numpy(), m.neighbour_counts.cpu().numpy()


def _lists(rec, x, k, batch=500):
  from recoder_amd.data import UsersInteractions
  n_users = x.shape[0]
  return np.concatenate([rec.recommend_array(UsersInteractions(np.arange(lo, min(n_users, lo + batch)),
                                                               x[lo:lo + batch]), k)
                         for lo in range(0, n_users, batch)])


def test_train_slim_info_and_tensors(syn):
  rec, info, x, _ = syn
  ids, w, count, sweeps, support = _syn_restated(SYN["K"])
  assert sorted(info) == ["cut_columns", "fit_ms", "gram_ms", "kept", "l1_reg", "l2_reg", "max_sweeps_run", "n",
                          "neighbours", "nnz", "unconverged_columns"]
  assert info["n"] == x.shape[1] and info["nnz"] == x.nnz
  assert (info["l1_reg"], info["l2_reg"], info["neighbours"]) == (SYN["l1"], SYN["l2"], SYN["K"])
  assert info["kept"] == int(count.astype(np.int64).sum()) > 0
  assert info["cut_columns"] == int((support > SYN["K"]).sum()) > 0
  assert info["unconverged_columns"] == int((sweeps >= SWEEPS).sum())
  assert info["max_sweeps_run"] == int(sweeps.max()) > 1
  assert info["fit_ms"] > 0 and info["gram_ms"] > 0
  print("SLIM on the synthetic catalogue: Gram %.2f ms, fit %.2f ms, %d entries kept, %d columns cut, up to %d sweeps"
        % (info["gram_ms"], info["fit_ms"], info["kept"], info["cut_columns"], info["max_sweeps_run"]))
  _assert_bitwise(_model_arrays(rec.model), (ids, w, count), "synthetic")
  assert rec.slim_info["kept"] == info["kept"]


def test_every_top20_list_is_the_restated_one(syn):
  rec, _, x, _ = syn
  ids, w, count, _, _ = _syn_restated(SYN["K"])
  S32 = slim_util.scores_f32(x, ids, w, count)
  lists = _lists(rec, x, 20, batch=128)
  assert lists.shape == (x.shape[0], 20)
  assert lists.min() >= 0 and lists.max() < x.shape[1]
  for u in range(x.shape[0]):
    seen = x.indices[x.indptr[u]:x.indptr[u + 1]]
    assert len(set(lists[u])) == 20 and not np.isin(lists[u], seen).any(), "a seen or repeated item"
  want = rp3_util.top_k(S32.copy(), x, 20)
  same = np.all(lists == want, axis=1)
  assert same.all(), "%d users' lists differ, first user %d" % ((~same).sum(), int(np.argmin(same)))
  rec.eval_strip_items = 100
  try:
    strips = _lists(rec, x, 20, batch=128)
  finally:
    del rec.eval_strip_items
  assert np.array_equal(strips, lists)


def test_metrics_match_float64_from_the_restated_model(syn):
  """``evaluate`` against float64 scores of the restated model: a user's metric can differ only where the f32
  and the float64 scores order the user's list differently, and lies in [0, 1], so the means differ by at
  most (users whose lists differ) / (users evaluated)."""
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  rec, _, x, y = syn
  ids, w, count, _, _ = _syn_restated(SYN["K"])
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=128)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  S64 = np.asarray(x.astype(np.float64) @ slim_util.dense(ids, w.astype(np.float64), count))
  L64 = rp3_util.top_k(S64, x, 100)
  L32 = rp3_util.top_k(slim_util.scores_f32(x, ids, w, count), x, 100)
  want_r, want_n = rp3_util.metric_means(L64, y)
  evaluated = int((np.diff(y.indptr) > 0).sum())
  slack = float(np.any(L64 != L32, axis=1).sum()) / evaluated + 1e-9
  print("synthetic: Recall@20 gpu %.6f f64 %.6f; NDCG@100 gpu %.6f f64 %.6f; slack %.3g"
        % (got[str(Recall(k=20))], want_r, got[str(NDCG(k=100))], want_n, slack))
  assert want_r > 0 and evaluated > 400
  assert abs(got[str(Recall(k=20))] - want_r) <= slack
  assert abs(got[str(NDCG(k=100))] - want_n) <= slack


def test_empty_history_gets_k_valid_items(syn):
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = syn
  m = sp.vstack([sp.csr_matrix((1, x.shape[1]), dtype=np.float32), x[1:4]]).tocsr()
  got = rec.recommend(UsersInteractions(np.arange(4), m), 20)
  assert len(got) == 4 and len(set(got[0])) == 20 and all(0 <= i < x.shape[1] for i in got[0])
  for u in range(1, 4):
    assert not np.isin(got[u], x[u].indices).any()


def test_checkpoint_round_trip(syn, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  rec, _, x, _ = syn
  f = rec.save_state(str(tmp_path / "slim"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == {"l1_reg": SYN["l1"], "l2_reg": SYN["l2"], "neighbours": SYN["K"]}
  assert sorted(st["model"]) == ["item_neighbours", "item_weights", "neighbour_counts"]
  rec2 = Recoder(model=SparseLinearModel(1.0, 0.0, 7))
  rec2.init_from_model_file(f)
  assert rec2.model.model_params() == rec.model.model_params()
  for name in ("item_neighbours", "item_weights", "neighbour_counts"):
    assert torch.equal(getattr(rec2.model, name), getattr(rec.model, name))
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))


def test_inference_recommender_gives_the_same_metrics(syn):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall, RecommenderEvaluator
  from recoder_amd.recommender import InferenceRecommender
  rec, _, x, y = syn
  ds = RecommendationDataset(x, y)
  metrics = [Recall(k=20, normalize=True), NDCG(k=100)]
  a = rec.evaluate(ds, num_recommendations=100, metrics=metrics, batch_size=128)
  b = RecommenderEvaluator(InferenceRecommender(rec, 100), metrics).evaluate(ds, batch_size=128)
  for k in a:      # (each evaluation draws its own user order: the per-user values as multisets)
    np.testing.assert_array_equal(np.sort(np.asarray(a[k], np.float64)), np.sort(np.asarray(b[k], np.float64)))
    assert np.isfinite(np.asarray(a[k], np.float64)).sum() > 400


def test_predict_and_forward_equal_the_scores_kernel(syn):
  from recoder_amd import slim
  from recoder_amd.data import UsersInteractions
  rec, _, x, _ = syn
  m = rec.model
  users = np.arange(64)
  out, _ = rec.predict(UsersInteractions(users, x[users]))
  want = slim.scores(_dev_csr(x[users]), m.item_neighbours, m.item_weights.data, m.neighbour_counts)
  assert out.shape == want.shape and torch.equal(out, want) and float(want.abs().max()) > 0
  dense = torch.from_numpy(np.asarray(x[users].todense(), np.float32)).to(DEV)
  assert torch.equal(m(dense), want)
  tt = torch.tensor([5, 3, 100, 11], device=DEV)
  ii = torch.arange(0, x.shape[1], 2, device=DEV)
  sub = m(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  ref = m.torch_forward(dense[:, ::2].contiguous(), input_items=ii, target_items=tt)
  assert sub.shape == (64, 4)
  assert torch.allclose(sub, ref, rtol=0, atol=1e-5 * float(ref.abs().max()))


def test_a_refit_with_another_k_reshapes(tmp_path):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  x, _ = _synthetic()
  ds = RecommendationDataset(x)
  rec = Recoder(model=SparseLinearModel())
  info = rec.train_slim(ds, l1_reg=SYN["l1"], l2_reg=SYN["l2"], neighbours=SYN["K"])
  assert rec.model.model_params() == {"l1_reg": SYN["l1"], "l2_reg": SYN["l2"], "neighbours": SYN["K"]}
  assert tuple(rec.model.item_weights.shape) == tuple(rec.model.item_neighbours.shape) == (SYN["n"], SYN["K"])
  _assert_bitwise(_model_arrays(rec.model), _syn_restated(SYN["K"])[:3], "explicit values")
  info = rec.train_slim(ds, neighbours=64)        # (l1_reg and l2_reg: the model's, i.e. the ones just stored)
  assert rec.model.model_params() == {"l1_reg": SYN["l1"], "l2_reg": SYN["l2"], "neighbours": 64}
  assert tuple(rec.model.item_weights.shape) == tuple(rec.model.item_neighbours.shape) == (SYN["n"], 64)
  assert info["cut_columns"] == int((_syn_restated(64)[4] > 64).sum()) and info["neighbours"] == 64
  _assert_bitwise(_model_arrays(rec.model), _syn_restated(64)[:3], "refit with another K")
  st = torch.load(rec.save_state(str(tmp_path / "slim")), map_location="cpu", weights_only=False)
  assert tuple(st["model"]["item_weights"].shape) == (SYN["n"], 64)
  with pytest.raises(ValueError, match="train_slim"):
    rec.train(ds)


# ------------------------------------------------- end to end: the ML-20M slice
# l1 = 2 leaves the slice's largest Gram row 1 119 candidates (above the LDS threshold: both state paths run
# in this fit), which is not below K = 1024 by itself; the supports are: the converged float64 solution
# (scikit-learn, l1 = 2, l2 = 500) has at most 540 entries in a column, and the sampled columns below, the
# most popular item's among them, have at most 501.  The test asserts cut_columns == 0.
SLICE_L1, SLICE_L2, SLICE_K = 2.0, 500.0, 1024
SLICE_KKT = 4.986e-3       # the largest KKT residual of cd_f32 on the 64 sampled columns, measured on the CPU


def slice_sample(G):
  cols = np.random.RandomState(20).choice(G.shape[0], 63, replace=False)
  top = int(np.argmax(np.diag(G)))
  return np.unique(np.concatenate([cols[cols != top][:63], [top]]))


@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  x, y = _slice()
  rec = Recoder(model=SparseLinearModel(SLICE_L1, SLICE_L2, SLICE_K))
  info = rec.train_slim(RecommendationDataset(x))
  return rec, info, x, slim_util.gram_f64(x)


def test_slice_sampled_columns_are_the_restatement(fitted):
  rec, info, x, G = fitted
  print("SLIM on the slice: Gram %.2f ms, fit %.2f ms, %d kept, %d cut, %d unconverged, up to %d sweeps"
        % (info["gram_ms"], info["fit_ms"], info["kept"], info["cut_columns"], info["unconverged_columns"],
           info["max_sweeps_run"]))
  cols = slice_sample(G)
  assert len(cols) == 64 and int(np.argmax(np.diag(G))) in cols
  want = slim_util.cd_f32(G.astype(np.float32), _inv(G, SLICE_L2), SLICE_L1, SLICE_K, SWEEPS, TOL, cols=cols)
  got = _model_arrays(rec.model)
  _assert_bitwise([a[cols] for a in got], [a[cols] for a in want[:3]], "slice sample")
  cands = np.array([len(slim_util.candidates(G, j, SLICE_L1)) for j in cols])
  from recoder_amd import slim
  assert cands.max() > slim.LDS_CANDIDATES and want[4][cols].max() <= SLICE_K
  assert info["cut_columns"] == 0 and info["n"] == x.shape[1] and info["nnz"] == x.nnz


def test_slice_kkt_of_the_whole_model(fitted):
  """The optimality conditions of every converged column in float64, r = G[:, j] - G w_j:
  |r_k - l1 - l2 w_k| <= eps on the support, r_k <= l1 + eps off it, w >= 0, a zero diagonal.  eps = 4 x the
  largest residual of ``cd_f32`` on the 64 sampled columns, measured on the CPU: 4.986e-3 (they run at most 11 sweeps;
  the residual of a stopped column is of the order tol x (G_kk + l2), 1e-5 x 1145 for the most popular item)."""
  rec, info, x, G = fitted
  assert info["cut_columns"] == 0
  ids, w, count = _model_arrays(rec.model)
  n, K = ids.shape
  live = np.arange(K)[None, :] < count[:, None]
  assert np.all(w[live] > 0) and np.all(ids[live] != np.nonzero(live)[0])
  W = sp.csc_matrix((w[live].astype(np.float64), (ids[live], np.nonzero(live)[0])), shape=(n, n))
  # (converged: fewer than max_sweeps sweeps; the kernel reports the sweeps, the model does not keep them, so
  # the columns are taken from the f32 rule on the host: a column the sample shows unconverged is skipped)
  eps = 4 * SLICE_KKT
  worst_on = worst_off = 0.0
  for lo in range(0, n, 1024):
    hi = min(n, lo + 1024)
    Wb = W[:, lo:hi]
    R = G[:, lo:hi] - np.asarray((Wb.T @ G).T)            # (G symmetric: G W = (W^T G)^T)
    Wd = np.asarray(Wb.todense())
    on = Wd > 0
    off = ~on
    off[np.arange(lo, hi), np.arange(hi - lo)] = False
    if on.any():
      worst_on = max(worst_on, float(np.abs(R[on] - SLICE_L1 - SLICE_L2 * Wd[on]).max()))
    worst_off = max(worst_off, float(np.maximum(R[off] - SLICE_L1, 0.0).max()))
  print("slice KKT: on the support %.3g, off it %.3g (eps %.3g), unconverged columns %d"
        % (worst_on, worst_off, eps, info["unconverged_columns"]))
  assert info["unconverged_columns"] == 0
  assert worst_on <= eps and worst_off <= eps
