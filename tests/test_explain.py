"""GPU: rk_ease_explain, rk_slim_explain and rk_als_explain against the f32 restatement of tests/explain_util.py bit
for bit (contributors, contributions, baseline, total, status) on the smallest inputs that reach every branch; the list
kernel against the dense kernel on the lists' dense matrix; sub-ranges of users, permuted targets and repeated runs;
the planted tie; ``Recoder.explain`` end to end on the ML-20M slice for an EASE fit and an ALS fit."""
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import explain_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _csr(csr, use_data):
  from recoder_amd import als
  c = als.AlsCSR(csr.copy(), DEV)                          # (the shared case is read-only)
  if not use_data:
    c.data = None
  elif c.data is None:
    c.data = _t(csr.data)
  return c


def _host(out):
  return tuple(o.cpu().numpy() for o in out)


def _same(got, want, what):
  for name, g, w in zip(("contributors", "contributions", "baseline", "total"), got, want):
    assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
    bad = np.argwhere(g.view(np.uint32 if g.dtype == F32 else np.int64) !=
                      np.ascontiguousarray(w).view(np.uint32 if w.dtype == F32 else np.int64))
    assert len(bad) == 0, (what, name, bad[:5].tolist())


def _permuted(run, items, got, what):
  """A permutation of every row's targets gives the same bits per pair."""
  perm = np.array([2, 0, 1])
  again = run(np.ascontiguousarray(items[:, perm]))
  _same(again, tuple(g[:, perm] for g in got), what + ", permuted targets")


# ----------------------------------------------------------------------------------------------- the item-item kernels
@pytest.mark.parametrize("use_data", [True, False], ids=["values", "ones"])
def test_dense_kernel_equals_the_restatement_bit_for_bit(use_data):
  from recoder_amd import explain
  csr, items = U.histories()
  c = _csr(csr, use_data)
  W = U.dense_w()
  Wt = _t(W)
  wide = _t(np.concatenate([W, np.full((U.N_ITEMS, 4), np.nan, F32)], axis=1))[:, :U.N_ITEMS]     # ldw = n + 4
  for m in U.MS:
    want = U.want_items("dense", m, use_data)
    for lo, hi in U.BATCHES:
      for J in U.JS:
        it = _t(items[lo:hi, :J], np.int64)
        got = _host(explain.dense(c, Wt, it, m, lo, hi))
        _same(got, U.cut(want, lo, hi, J, m), ("dense", m, lo, J))
        if m == 5 and J == 3:
          _same(_host(explain.dense(c, Wt, it, m, lo, hi)), got, "dense, second run")
          _same(_host(explain.dense(c, wide, it, m, lo, hi)), got, "dense, ldw > n")
          _permuted(lambda p: _host(explain.dense(c, Wt, _t(p, np.int64), m, lo, hi)), items[lo:hi], got, "dense")
  # a user alone: B = 1 gives the pair's bits of the batch
  one = _host(explain.dense(c, Wt, _t(items[9:10], np.int64), 5, 9, 10))
  _same(one, U.cut(U.want_items("dense", 5, use_data), 9, 10, 3, 5), "dense, B = 1")


@pytest.mark.parametrize("columns", [True, False], ids=["columns", "rows"])
@pytest.mark.parametrize("K", U.KS)
def test_list_kernel_equals_the_restatement_and_the_dense_kernel(K, columns):
  from recoder_amd import explain
  csr, items = U.histories()
  ids, w, count = U.neighbour_lists(K)
  ti, tw, tc = _t(ids, np.int32), _t(w), _t(count, np.int32)
  Wt = _t(U.lists_to_dense(ids, w, count, columns))
  for use_data in (True, False):
    c = _csr(csr, use_data)
    for m in U.MS:
      want = U.want_items((K, columns), m, use_data)
      for lo, hi in U.BATCHES:
        for J in U.JS:
          it = _t(items[lo:hi, :J], np.int64)
          got = _host(explain.lists(c, ti, tw, tc, columns, it, m, lo, hi))
          _same(got, U.cut(want, lo, hi, J, m), ("lists", K, columns, use_data, m, lo, J))
          _same(_host(explain.dense(c, Wt, it, m, lo, hi)), got, ("dense on the lists' matrix", K, columns, m, lo, J))
    if use_data:
      _same(_host(explain.lists(c, ti, tw, tc, columns, it, m, lo, hi)), got, "lists, second run")
      _permuted(lambda p: _host(explain.lists(c, ti, tw, tc, columns, _t(p, np.int64), m, lo, hi)), items[lo:hi], got,
                "lists")
  # the target no list holds: every contribution is +0, and the history still fills the m places
  u, q = np.argwhere(items == U.ABSENT)[0]
  full = U.want_items((K, columns), 5, True)
  assert not full[1][u, q].any() and full[3][u, q] == 0 and (full[0][u, q] >= 0).sum() == min(5, U.LENGTHS[u])


def test_planted_tie():
  """W zero but W[3, 7] = 2, W[5, 7] = -1, W[9, 7] = 2; history {3, 5, 9}, target 7, m = 2: contributors (3, 9) by the
  tie rule, contributions (2, 2), total 3."""
  from recoder_amd import explain
  W = np.zeros((12, 12), F32)
  W[3, 7], W[5, 7], W[9, 7] = 2, -1, 2
  row = np.zeros((1, 12), F32)
  row[0, [3, 5, 9]] = 1
  ids, c, base, tot = _host(explain.dense(_csr(sp.csr_matrix(row), False), _t(W), _t([[7]], np.int64), 2))
  assert ids.tolist() == [[[3, 9]]] and c.tolist() == [[[2.0, 2.0]]] and base.tolist() == [[0.0]]
  assert tot.tolist() == [[3.0]]


# ----------------------------------------------------------------------------------------------------- the MF kernel
def _run_mf(csr, p, v, bias, alpha, use_data, items, m, lo=0, hi=None):
  from recoder_amd import explain
  h = p["Y"].shape[1]
  Yt = _t(np.concatenate([p["Y"], np.full((p["Y"].shape[0], 3), np.nan, F32)], axis=1))[:, :h]    # ldy = h + 3
  out = explain.folded(_csr(csr, use_data), Yt, _t(p["G"]), _t(v), None if bias is None else _t(bias), alpha,
                       _t(items, np.int64), m, lo, hi)
  return _host(out)


@pytest.mark.parametrize("h", U.HS)
def test_mf_kernel_equals_the_restatement_bit_for_bit(h):
  csr, items = U.histories()
  p = U.mf_problem(h)
  for vi, (name, alpha, use_data, bias_given) in enumerate(U.VARIANTS):
    v, bias = U.variant_inputs(p, bias_given)
    want = U.want_mf(h, vi)
    assert not want[4].any()
    for m in U.MS:
      for lo, hi in U.BATCHES:
        for J in (U.JS if vi == 0 else (3,)):
          got = _run_mf(csr, p, v, bias, alpha, use_data, items[lo:hi, :J], m, lo, hi)
          _same(got[:4], U.cut(want, lo, hi, J, m), (name, h, m, lo, J))
          assert not got[4].any()
    if vi == 0:
      run = lambda it: _run_mf(csr, p, v, bias, alpha, use_data, it, m, lo, hi)[:4]
      _same(run(items[lo:hi]), got[:4], "mf, second run")
      _permuted(run, items[lo:hi], got[:4], "mf")
    if not bias_given:                                       # without a bias nothing is left over
      assert not got[2].any()
  print("h = %d: f32 restatement against float64, relative to sum |c_e| + |baseline|: %.3g"
        % (h, max(U.mf_error(h, vi) for vi in range(len(U.VARIANTS)))))


def test_mf_singular_row_has_status_one_and_zero_contributions():
  s = U.singular_case()
  want = U.mf_explain32(s["csr"], s["Y"], s["G"], s["v"], s["bias"], s["alpha"], s["items"], 3)
  got = _run_mf(s["csr"], s, s["v"], s["bias"], s["alpha"], True, s["items"], 3)
  assert got[4].tolist() == want[4].tolist() == [1]
  _same(got[:4], want[:4], "singular")
  assert got[0][0].tolist() == [[0, 2, -1], [-1, -1, -1], [0, 2, -1]] and not got[3].any()
  # a regular row in the same call is not touched by it: reg = 1 on the same Y
  G = s["G"] + np.eye(3, dtype=F32)
  two = sp.csr_matrix(np.array([[0, 0, 0, 0], [2.0, 0, 1.0, 0]], F32))
  items = np.array([[1, 0, 3], [1, -1, 2]], np.int64)
  want = U.mf_explain32(two, s["Y"], G, s["v"], s["bias"], 10.0, items, 3)
  got = _run_mf(two, dict(s, G=G), s["v"], s["bias"], 10.0, True, items, 3)
  assert got[4].tolist() == [0, 0]
  _same(got[:4], want[:4], "regular rows")
  assert (got[0][0] == -1).all() and got[3][0].tobytes() == got[2][0].tobytes()      # empty history: total = baseline


# ------------------------------------------------------------------------------------------------------- end to end
def _slice():
  z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_ml20m_slice.npz"))
  shape = tuple(int(v) for v in z["shape"])
  return sp.csr_matrix((z["x/data"], z["x/indices"], z["x/indptr"]), shape=shape)


def _batch(x, users):
  from recoder_amd.data import UsersInteractions
  return UsersInteractions(users, x[users])


def _check_shapes_and_order(ex, batch_matrix, recs, m):
  B, J = recs.shape
  assert ex.contributors.shape == ex.contributions.shape == (B, J, m) and ex.contributors.dtype == np.int64
  assert ex.baseline.shape == ex.total.shape == (B, J) and ex.total.dtype == ex.contributions.dtype == F32
  for u in range(B):
    hist = batch_matrix[u].indices
    keep = min(m, len(hist))
    for q in range(J):
      ids, c = ex.contributors[u, q], ex.contributions[u, q]
      assert (ids[:keep] >= 0).all() and np.isin(ids[:keep], hist).all() and len(set(ids[:keep])) == keep
      assert (ids[keep:] == -1).all() and not c[keep:].any()
      assert (np.diff(c[:keep]) <= 0).all(), "contributions must not increase along m"


def test_explain_an_ease_fit_on_the_slice():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  x = _slice()
  rec = Recoder(model=ShallowAutoencoder(500.0))
  rec.train_ease(RecommendationDataset(x))
  users = np.arange(64)
  batch = _batch(x, users)
  recs = rec.recommend_array(batch, 5)
  ex = rec.explain(batch, recs)
  _check_shapes_and_order(ex, batch.interactions_matrix, recs, 5)
  assert not ex.baseline.any()
  scores = rec.predict(batch)[0].cpu().numpy()
  W = rec.model.item_weights.data
  worst = 0.0
  for u in range(64):
    row = batch.interactions_matrix[u]
    for q, j in enumerate(recs[u]):
      w = W[torch.as_tensor(row.indices, dtype=torch.int64, device=W.device), int(j)].cpu().numpy().astype(np.float64)
      bound = len(row.indices) * 2.0 ** -23 * np.abs(row.data.astype(np.float64) * w).sum()
      err = abs(float(ex.total[u, q]) - float(scores[u, j]))
      worst = max(worst, err / max(bound, 1e-300))
      assert err <= bound, (u, q, err, bound)
  print("EASE: |total - predict| at most %.3g of r 2^-23 sum |x W|" % worst)


# measured on an MI355X: the restatement's error 2.24e-06 (h = 64); |total - (y_j . fold_in + b_j)| reached 0.39 of it
ALS_FACTOR = 4.0


def test_explain_an_als_fit_on_the_slice():
  """total against y_j . fold_in(batch)[u] + b_j, both f32 in different orders: within ALS_FACTOR times the f32
  restatement's measured error against float64 (``explain_util.mf_error`` at h = 64, relative to the pair's
  sum |c_e| + |baseline|), times that scale.  The measured slack is printed beside the factor."""
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x = _slice()
  rec = Recoder(model=MatrixFactorization(64), loss="mse", loss_params={"confidence": 10.0}, optimizer_type="adam")
  rec.train_als(RecommendationDataset(x), num_iterations=2, reg=100.0, cg_steps=3)
  users = np.arange(64)
  batch = _batch(x, users)
  recs = rec.recommend_array(batch, 5)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    ex = rec.explain(batch, recs)
    X = rec.fold_in(batch.interactions_matrix).cpu().numpy()
  _check_shapes_and_order(ex, batch.interactions_matrix, recs, 5)
  Y = rec.model.item_embedding_layer.weight.data.cpu().numpy()
  b = rec.model.bias.data.cpu().numpy()
  G = Y.astype(np.float64).T @ Y.astype(np.float64) + 100.0 * np.eye(64)
  v = (Y.astype(np.float64).T @ b.astype(np.float64)).astype(F32)
  measured = max(U.mf_error(64, vi) for vi in range(len(U.VARIANTS)))
  worst = 0.0
  for u in range(64):
    row = batch.interactions_matrix[u]
    ref = U.mf_row64(row.indices, row.data, Y, G.astype(F32), v, b, 30.0, recs[u], 5)
    for q, j in enumerate(recs[u]):
      score = float(F32(Y[j].astype(np.float64) @ X[u].astype(np.float64)) + b[j])
      slack = abs(float(ex.total[u, q]) - score) / (measured * ref[5][q])
      worst = max(worst, slack)
  print("ALS: measured error %.3g; |total - (y_j . fold_in + b_j)| is at most %.3g times it (factor %g)"
        % (measured, worst, ALS_FACTOR))
  assert worst <= ALS_FACTOR, (worst, measured)
