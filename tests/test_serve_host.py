"""CPU: the restatements of tests/serve_util.py against each other and against brute force, the argument checks of
recoder_amd.serve (all before any GPU work), metrics.sampled_candidates, and the ALS library's exports."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import recommend_util as RU
from tests import serve_util as S
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_pair_scores", "rk_als_pairs_topk", "rk_als_pairs_topk_max_row", "rk_als_serve_mask"]


def test_the_als_library_exports_exactly_its_header(built):
  from recoder_amd import _als_lib, _lib, serve
  header = declared([os.path.join(INC, "recoder_als.h")])
  assert exports(built.ALS_LIB) == header == sorted(_als_lib.SIGNATURES)
  assert all(name in header for name in NEW)
  lib = _als_lib.load()
  assert lib.rk_als_pairs_topk_max_row() == serve.PAIRS_MAX_ROW == _als_lib.PAIRS_TOPK_MAX_ROW == 8192
  assert _lib.load().rk_topk_max_k() == serve.TOPK_MAX_K
  assert lib.rk_als_ials_max_h() == _als_lib.IALS_MAX_H


# ------------------------------------------------------------------------------------------------ restatements
def test_pair_order_depends_on_h_alone_and_covers_every_dimension_once():
  for h in (4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 520, 1024, 1028, 2048):
    W, Q = S.pair_order(h)
    dims = sorted(4 * (j + W * q) + c for j in range(W) for q in range(Q) for c in range(4))
    assert dims[:h] == list(range(h)) and len(set(dims)) == len(dims), h
  assert S.pair_order(64) == (16, 1) and S.pair_order(68) == (32, 1) and S.pair_order(520) == (64, 4)


@pytest.mark.parametrize("h", [4, 64, 68, 520])
def test_pair_restatement_is_within_the_forward_bound_of_float64(h):
  rng = np.random.RandomState(h)
  z = rng.randn(h).astype(np.float32)
  Y = rng.randn(37, h).astype(np.float32)
  b = rng.randn(37).astype(np.float32)
  for bias in (None, b):
    got = S.pair_scores(z, Y, bias).astype(np.float64)
    want = Y.astype(np.float64) @ z.astype(np.float64) + (0.0 if bias is None else bias.astype(np.float64))
    assert (np.abs(got - want) <= S.forward_bound(z, Y, bias)).all()


def test_pair_restatement_is_exact_on_small_integers():
  rng = np.random.RandomState(1)
  for h in (4, 36, 64, 200):
    z = rng.randint(-8, 9, size=h).astype(np.float32)
    Y = rng.randint(-8, 9, size=(50, h)).astype(np.float32)
    b = rng.randint(-8, 9, size=50).astype(np.float32)
    assert np.array_equal(S.pair_scores(z, Y, b), (Y.astype(np.int64) @ z.astype(np.int64) + b).astype(np.float32))


def test_ragged_topk_restatement_against_brute_force_and_its_edges():
  rng = np.random.RandomState(2)
  n, k = 90, 7
  counts = [0, k - 1, k, k + 1, 60]
  cand = S.csr_lists(len(counts), n, counts, rng)
  scores = (rng.randint(-6, 6, size=cand.nnz) / 4.0).astype(np.float32)       # (quantised: ties under different ids)
  ok = rng.rand(cand.nnz) > 0.2
  ids, val, cnt = S.ragged_topk(cand.indptr, cand.indices, scores, k, ok)
  dense = np.full((len(counts), n), -np.inf)
  okd = np.zeros((len(counts), n), dtype=bool)
  rows = np.repeat(np.arange(len(counts)), counts)
  dense[rows, cand.indices] = scores
  okd[rows, cand.indices] = ok
  want_ids, want_val = S.brute_force(dense, okd, k)
  assert np.array_equal(ids, want_ids) and np.array_equal(val.astype(np.float64), want_val)
  assert np.array_equal(cnt, okd.sum(axis=1))
  # both zeros are one value (the lower id first), the canonical NaN ranks above +inf
  sc = np.array([0.0, -0.0, np.inf, RU.CANON_NAN, -1.0], dtype=np.float32)
  ids, val, _ = S.ragged_topk([0, 5], np.array([9, 3, 5, 7, 1]), sc, 5)
  assert ids.tolist() == [[7, 5, 3, 9, 1]] and np.isnan(val[0, 0]) and not np.signbit(val[0, 2:4]).any()


def test_mask_words_layout():
  ok = np.zeros((2, 33), dtype=bool)
  ok[0, [0, 31, 32]] = True
  bits, elig = S.mask_words(ok, 3)
  assert bits[0].tolist() == [0x7ffffffe, 0xfffffffe, 0xffffffff] and bits[1].tolist() == [0xffffffff] * 3
  assert elig.tolist() == [3, 0]


def test_eligibility_definition_on_its_edges():
  seen = sp.csr_matrix(np.array([[1.0, 0.0, -2.0, 3.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]]))
  ua = sp.csr_matrix((np.array([0.0, 1.0, 1.0]), np.array([1, 2, 3]), np.array([0, 3, 3])), shape=(2, 5))
  ok = S.eligible_dense(2, 5, seen)
  assert ok.tolist() == [[False, True, True, False, True], [True] * 5]          # (a negative value does not mask)
  ok = S.eligible_dense(2, 5, seen, user_allow=ua, deny_items=[2, 2])
  assert ok.tolist() == [[False, True, False, False, False], [False] * 5]       # (the explicit zero at 1 is present)
  assert S.eligible_dense(2, 5, seen, filter_seen=False, allow_items=np.zeros(0, np.int64)).sum() == 0


def test_filters_canonicalise_like_the_definition():
  from recoder_amd import serve
  rng = np.random.RandomState(3)
  n, B = 70, 4
  ua = sp.random(B, n, density=0.3, random_state=rng, format="coo")
  ua = sp.coo_matrix((np.concatenate([ua.data, ua.data]) * 0, (np.concatenate([ua.row, ua.row]),
                                                               np.concatenate([ua.col, ua.col]))), shape=(B, n))
  f = serve.Filters(B, n, True, allow_items=rng.rand(n) > 0.3, deny_items=[5, 5, 69], user_allow=ua)
  indptr, ids = f.user_allow
  for r in range(B):
    row = ids[indptr[r]:indptr[r + 1]]
    assert (np.diff(row) > 0).all() and np.array_equal(np.nonzero(S.pattern(ua, B, n)[r])[0], row)
  assert np.array_equal(f.deny, S.catalogue([5, 69], n)) and f.max_row == int(np.diff(indptr).max())
  words = serve.pack_bits(f.deny)
  assert words.dtype == np.uint32 and len(words) == 3 and words.tolist() == [1 << 5, 0, 1 << 5]


# ------------------------------------------------------------------------------------------------- validation
def _rec(model=None, **kw):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  kw.setdefault("optimizer_type", "adam")
  return Recoder(model=MatrixFactorization(16) if model is None else model, loss="mse",
                 loss_params={"confidence": 10.0}, **kw)


def _batch(B=3, n=40):
  from recoder_amd.data import UsersInteractions
  return UsersInteractions(np.arange(B), sp.csr_matrix(np.eye(B, n, dtype=np.float32)))


@pytest.mark.parametrize("case", [
    "bad_allow_id", "bad_deny_id", "negative_id", "bool_wrong_length", "float_ids", "two_d_ids", "allow_rows",
    "allow_cols", "deny_dense", "pairs_without_candidates", "pairs_on_autoencoder", "pairs_on_activation",
    "pairs_too_long", "route_name", "k_above_cap", "k_zero", "k_above_items", "generic_engine"])
def test_recommend_filtered_refuses_before_gpu_work(case, monkeypatch):
  import recoder_amd.model as model_mod
  from recoder_amd import device, serve
  from recoder_amd.nn import DynamicAutoencoder, MatrixFactorization

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  n = 40
  cand = sp.csr_matrix(np.ones((3, n), dtype=np.float32))
  rec, k, kw, batch = _rec(), 5, {}, _batch()
  if case == "bad_allow_id":
    kw = dict(allow_items=[0, n])
  elif case == "bad_deny_id":
    kw = dict(deny_items=np.array([n + 7]))
  elif case == "negative_id":
    kw = dict(deny_items=[-1])
  elif case == "bool_wrong_length":
    kw = dict(allow_items=np.ones(n - 1, dtype=bool))
  elif case == "float_ids":
    kw = dict(deny_items=np.array([1.0, 2.0]))
  elif case == "two_d_ids":
    kw = dict(deny_items=np.zeros((2, 2), dtype=np.int64))
  elif case == "allow_rows":
    kw = dict(user_allow=sp.csr_matrix((4, n)))
  elif case == "allow_cols":
    kw = dict(user_allow=sp.csr_matrix((3, n + 1)))
  elif case == "deny_dense":
    kw = dict(user_deny=np.zeros((3, n)))
  elif case == "pairs_without_candidates":
    kw = dict(route="pairs")
  elif case == "pairs_on_autoencoder":
    rec, kw = _rec(DynamicAutoencoder(hidden_layers=[16])), dict(route="pairs", user_allow=cand)
  elif case == "pairs_on_activation":
    rec, kw = _rec(MatrixFactorization(16, activation_type="tanh")), dict(route="pairs", user_allow=cand)
  elif case == "pairs_too_long":
    n = serve.PAIRS_MAX_ROW + 1
    batch = _batch(1, n)
    kw = dict(route="pairs", user_allow=sp.csr_matrix(np.ones((1, n), dtype=np.float32)))
  elif case == "route_name":
    kw = dict(route="dense")
  elif case == "k_above_cap":
    k, batch = serve.TOPK_MAX_K + 1, _batch(3, 2000)
  elif case == "k_zero":
    k = 0
  elif case == "k_above_items":
    k = n + 1
  elif case == "generic_engine":
    rec = _rec(optimizer_type="sgd")
  with pytest.raises(ValueError) as e:
    rec.recommend_filtered(batch, k, **kw)
  if case == "generic_engine":
    assert "generic" in str(e.value) and "no dense fallback" in str(e.value)
  if case == "k_above_cap":
    assert str(serve.TOPK_MAX_K) in str(e.value)
  if case.startswith("pairs_"):
    assert "route='pairs'" in str(e.value)
    with pytest.raises(ValueError):
      rec.rerank(batch, kw.get("user_allow"), k, route="pairs")


def test_auto_route_takes_pairs_only_where_it_is_legal():
  from recoder_amd import serve
  from recoder_amd.nn import DynamicAutoencoder
  cand = sp.csr_matrix(np.ones((3, 40), dtype=np.float32))
  pick = lambda rec, route, **kw: serve.pick_route(rec, serve.Filters(3, 40, **kw), route)
  assert pick(_rec(), "auto", user_allow=cand) == "pairs"
  assert pick(_rec(), "mask", user_allow=cand) == "mask"
  assert pick(_rec(), "auto") == "mask"
  assert pick(_rec(DynamicAutoencoder(hidden_layers=[16])), "auto", user_allow=cand) == "mask"
  assert serve.Filters(3, 40, filter_seen=False, user_allow=cand).only_candidates()
  assert not serve.Filters(3, 40, user_allow=cand).only_candidates()


# ----------------------------------------------------------------------------------------- sampled candidates
def _protocol_matrices():
  rng = np.random.RandomState(5)
  n_users, n = 6, 30
  seen = sp.random(n_users, n, density=0.3, random_state=rng, format="lil", dtype=np.float32)
  seen[5, :] = 1.0
  seen[5, [3, 4, 7, 9]] = 0.0                                   # user 5: 4 items that are not seen,
  target = sp.lil_matrix((n_users, n), dtype=np.float32)
  for u in range(n_users):
    free = np.setdiff1d(np.arange(n), seen.rows[u])
    target[u, free[0]] = 1.0                                    # one of them its target: 3 negatives at most
  return sp.csr_matrix(target), sp.csr_matrix(seen)


def test_sampled_candidates():
  from recoder_amd.metrics import sampled_candidates
  target, seen = _protocol_matrices()
  a = sampled_candidates(target, seen, 8, seed=11)
  b = sampled_candidates(target, seen, 8, seed=11)
  c = sampled_candidates(target, seen, 8, seed=12)
  assert a.shape == target.shape and (a != b).nnz == 0 and (a != c).nnz > 0
  pa, pt, ps = (S.pattern(m, *target.shape) for m in (a, target, seen))
  assert not (pa & ps).any()                                    # no seen item
  assert (pa | ~pt).all()                                       # the targets included
  neg = (pa & ~pt).sum(axis=1)
  assert neg[:5].tolist() == [8] * 5 and neg[5] == 3            # a user short of negatives takes all it has
  for u in range(6):
    row = a.indices[a.indptr[u]:a.indptr[u + 1]]
    assert (np.diff(row) > 0).all()
  # a row's draw does not depend on the other rows
  one = sampled_candidates(target[:3], seen[:3], 8, seed=11)
  assert (one != a[:3]).nnz == 0
  with pytest.raises(ValueError):
    sampled_candidates(target, seen[:, :-1], 8, seed=0)
  with pytest.raises(ValueError):
    sampled_candidates(target, seen, -1, seed=0)


def test_host_metrics_count_an_id_outside_the_catalogue_as_a_miss():
  """The padding id -1 must not alias item n - 1 of the row before (the flat key of batch_metrics)."""
  from recoder_amd.metrics import NDCG, AveragePrecision, Recall, batch_metrics
  target = sp.csr_matrix(np.array([[0, 0, 1], [1, 0, 0]], dtype=np.float32))
  recs = np.array([[2, -1], [-1, 3]], dtype=np.int64)
  out = batch_metrics(recs, target, [Recall(2), NDCG(2), AveragePrecision(2)])
  assert [out[m] for m in out] == [[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]]
