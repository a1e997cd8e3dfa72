"""CPU: the built library's rk_als_ugcn_* names and argument checks, the pin of the numpy restatement
(tests/ultragcn_util.py) -- its coefficients, users' rows, item gradient and loss terms against torch autograd in
float64, its item graph against a dense brute force on a fixture with an empty column, an isolated column and a tie,
its draws against the sampler's and the sampled softmax's -- and what train_ultragcn and the wrappers refuse before any
GPU work."""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from tests import bpr_util, ssm_util, ultragcn_util as uu
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_ugcn_grad", "rk_als_ugcn_scatter", "rk_als_ugcn_workspace_bytes"]
W = (0.3, 1.0, 0.2, 0.7)


# ------------------------------------------------------------------ library
def test_the_library_exports_exactly_the_declared_ugcn_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_ugcn_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_ugcn_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib, ultragcn
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()

  def grad(T=8, R=4, K=2, step=0, n_users=5, n_items=5, ldx=8, h=8, users=p, nbr=p, loss=p):
    return lib.rk_als_ugcn_grad(users, p, T, R, K, 0, step, n_users, n_items, p, ldx, p, 8, h, p, p, nbr, p, 1.0, 1.0,
                                1.0, 1.0, 1.0, 1.0, p, p, p, p, loss, None)
  assert grad(ldx=4) == -2 and "ldx, ldy >= h" in err() and err().startswith("rk_als_ugcn_grad: ")
  assert grad(h=513, ldx=513) == -2 and "1 <= h <= 512" in err()
  for kw in (dict(T=0), dict(T=4097), dict(R=0), dict(R=1025), dict(K=-1), dict(K=65), dict(T=4096, R=1024, K=0)):
    assert grad(**kw) == -2 and "T (1 + R + K) <= 2^22" in err(), kw
  assert grad(n_items=0) == -2 and "n_users, n_items >= 1" in err()
  assert grad(step=-1) == -2 and "step >= 0" in err()
  assert grad(users=None) == -2 and "null pointer" in err()
  assert grad(loss=None) == -2 and "null pointer" in err()
  assert grad(nbr=None) == -2 and "neighbour lists" in err()

  def scatter(n=24, E=3, h=8, ldx=8, ldg=8, n_rows=5, keys=p, count=p):
    return lib.rk_als_ugcn_scatter(keys, p, n, E, p, p, p, ldx, 5, h, 1.0, n_rows, p, ldg, count, None)
  assert scatter(ldg=4) == -2 and "ldx, ldg >= h" in err() and err().startswith("rk_als_ugcn_scatter: ")
  for kw in (dict(E=1), dict(n=25), dict(n=0), dict(n=4097 * 3), dict(n=(1 << 22) + 1090, E=1090)):
    assert scatter(**kw) == -2 and "n = T E" in err(), kw
  assert scatter(n_rows=0) == -2 and "n_rows >= 1" in err()
  assert scatter(keys=None) == -2 and "null pointer" in err()
  assert scatter(count=None) == -2 and "null pointer" in err()
  # the workspace formula and its limits
  for T, R, K, h in ((0, 1, 0, 8), (4097, 1, 0, 8), (8, 0, 0, 8), (8, 1025, 0, 8), (8, 1, -1, 8), (8, 1, 65, 8),
                     (8, 1, 0, 0), (8, 1, 0, 513), (4096, 1024, 0, 8), (4096, 1000, 64, 8)):
    assert lib.rk_als_ugcn_workspace_bytes(T, R, K, h) == -2 == ultragcn.workspace_bytes(T, R, K, h), (T, R, K, h)
  for T, R, K, h in ((1, 1, 0, 1), (9, 5, 3, 6), (1024, 512, 10, 64), (4096, 1023 - 64, 64, 512), (4096, 1, 64, 7)):
    got = lib.rk_als_ugcn_workspace_bytes(T, R, K, h)
    assert got == ultragcn.workspace_bytes(T, R, K, h) >= 4 * T * (2 * (1 + R + K) + 3), (T, R, K, h)


# ------------------------------------------------------------------- draws
def test_the_draws_are_in_range_private_to_the_slot_and_apart_from_every_other_domain():
  n = 7915
  d = uu.draws(11, 5, 300, 37, n)
  assert d.shape == (300, 37) and d.dtype == np.int32 and d.min() >= 0 and d.max() < n
  # (uniform over the catalogue: N draws of n values leave n (1 - exp(-N / n)) distinct ones)
  assert abs(len(np.unique(d)) / (n * (1 - np.exp(-d.size / n))) - 1) < 0.03
  assert abs(d.mean() / n - 0.5) < 0.01
  # a function of (seed, step, t R + r) alone: a shorter batch draws a prefix, a slot can be drawn by itself
  assert np.array_equal(uu.draws(11, 5, 120, 37, n), d[:120])
  assert np.array_equal(uu.draws(11, 5, 0, 37, n, slots=[299, 4]), d[[299, 4]])
  assert not np.array_equal(uu.draws(12, 5, 300, 37, n), d) and not np.array_equal(uu.draws(11, 6, 300, 37, n), d)
  # slots do not share their negatives, and the counters 0 .. T R - 1 differ from BPR's draws (slot = the counter,
  # any draw number) and from the sampled softmax's shared draws at the same counters
  assert not np.array_equal(d[0], d[1])
  flat = d.reshape(-1)
  keys = bpr_util.slot_keys(11, 5, flat.size)
  for k in range(0, 3):
    assert (bpr_util.draw(keys, k, n) == flat).mean() < 0.01, k
  assert (ssm_util.shared_draws(11, 5, flat.size, n) == flat).mean() < 0.01
  assert uu.TAG not in (ssm_util.TAG, 0x80000000) and uu.TAG >> 24 != 0 and 300 * 37 < 1 << 24


# ------------------------------------------------------- the model, autograd
def _autograd(X, Y, users, items, negs, bu, bi, nbr_ids, nbr_w, w, nw, iw):
  """(the three terms per slot, d sum L / d s per candidate, d / d X, d / d Y) by torch autograd in float64."""
  N = Y.shape[0]
  Xt, Yt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (X, Y))
  cand, ok = uu.candidates(users, items, negs, nbr_ids, X.shape[0], N)
  T, R = negs.shape
  terms, scores = torch.zeros(T, 3, dtype=torch.float64), {}
  rows = []
  for t in np.nonzero(ok)[0]:
    u, i = int(users[t]), int(items[t])
    s = [(Xt[u] * Yt[int(j)]).sum() if j < N else None for j in cand[t]]
    for e, v in enumerate(s):
      if v is not None:
        v.retain_grad()
        scores[t, e] = v
    beta = lambda j: float(bu[u]) * float(bi[int(j)])
    pos = (w[0] + w[1] * beta(i)) * F.softplus(-s[0])
    neg = sum((nw / R) * (w[2] + w[3] * beta(cand[t, 1 + r])) * F.softplus(s[1 + r]) for r in range(R))
    nbr = sum((iw * float(nbr_w[i, n]) * F.softplus(-s[1 + R + n]) for n in range(cand.shape[1] - 1 - R)
               if s[1 + R + n] is not None), torch.zeros((), dtype=torch.float64))
    rows.append((t, pos, neg, nbr))
  total = sum(p + n + b for _, p, n, b in rows)
  total.backward()
  for t, p, n, b in rows:
    terms[t] = torch.stack([p.detach(), n.detach(), torch.as_tensor(b).detach()])
  coef = np.zeros(cand.shape)
  for (t, e), v in scores.items():
    coef[t, e] = float(v.grad)
  return terms.numpy(), coef, Xt.grad.numpy(), Yt.grad.numpy(), float(total.detach())


def _close(a, b, rel=1e-12):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), np.abs(b).max() * 1e-3 + 1e-300))


@pytest.mark.parametrize("K", [3, 0])
def test_the_restatement_equals_autograd_in_float64(K):
  X, Y, users, items, negs, bu, bi, nbr_ids, nbr_w = uu.small_case(N=40, T=9, R=5, K=K, h=6)
  users[4] = -1                                              # (an invalid slot: nothing anywhere)
  nw, iw = 3.0, 0.4
  cand, coef, DU, valid, loss, DI, count = uu.grad_rows(users, items, negs, X, Y, bu, bi, nbr_ids, nbr_w, W, nw, iw)
  terms, acoef, gX, gY, total = _autograd(X, Y, users, items, negs, bu, bi, nbr_ids, nbr_w, W, nw, iw)
  assert valid.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1] and (cand[4] == 40).all() and (coef[4] == 0).all()
  assert _close(loss, terms) and _close(coef, acoef)
  assert _close(loss.sum(), uu.slot_loss(users, items, negs, X, Y, bu, bi, nbr_ids, nbr_w, W, nw, iw))
  assert _close(DI, gY)                                       # the item gradient: every candidate's weighted user row
  Gu = np.zeros_like(X)
  np.add.at(Gu, users[valid > 0], DU[valid > 0])
  assert _close(Gu, gX)                                       # the users' rows, summed per user
  assert (count == np.bincount(items[valid > 0], minlength=40)).all()
  if K:                                                      # the absent neighbour of slot 0's positive
    assert cand[0, -1] == 40 and coef[0, -1] == 0 and (cand[0, :-1] < 40).all()
  # one step's gradient is that of (1 / T) sum L_t, with the L2 counts of users and positives only
  cons = type("C", (), dict(bu=bu, bi=bi, nbr_ids=nbr_ids, nbr_w=nbr_w))
  Gu1, Gi1, cu, ci, lsum, cnt = uu.gradient(X, Y, users, items, negs, cons, W, nw, iw)
  assert _close(Gu1, gX / 9) and _close(Gi1, gY / 9) and cnt == 8 and _close(lsum, terms.sum(0))
  assert (cu == np.bincount(users[valid > 0], minlength=40)).all() and (ci == count).all() and ci.sum() == 8


# -------------------------------------------------------------- the constraints
def _brute_graph(A, K):
  """omega and the neighbour lists entry by entry from the dense binary matrix."""
  n = A.shape[1]
  G = A.T @ A
  g = G.sum(1)
  ids, wts = np.full((n, K), -1, np.int32), np.zeros((n, K), np.float32)
  om = np.full((n, n), -1.0)
  for i in range(n):
    for j in range(n):
      if i != j and G[i, j] > 0 and g[i] - G[i, i] > 0:
        om[i, j] = G[i, j] / (g[i] - G[i, i]) * np.sqrt(g[i] / g[j])
    order = sorted((j for j in range(n) if om[i, j] > 0), key=lambda j: (-om[i, j], j))[:K]
    ids[i, :len(order)] = order
    wts[i, :len(order)] = om[i, order]
  return ids, wts, om


def test_the_item_graph_against_a_dense_brute_force_with_an_empty_an_isolated_and_two_tied_columns():
  m = uu.graph_fixture()
  A = m.toarray().astype(np.float64)
  assert A.shape == (30, 20) and A[:, 0].sum() == 0 and A[:, 1].sum() == 1 and A[0].sum() == 1
  assert (A[:, 2] == A[:, 3]).all() and A[:, 2].sum() >= 3
  for K in (1, 4, 25):
    ids, wts = uu.item_graph(m, K, block=7)
    bids, bwts, om = _brute_graph(A, K)
    assert (ids == bids).all() and np.array_equal(wts, bwts), K
  ids, wts = uu.item_graph(m, 4, block=7)
  assert (ids[0] == -1).all() and (wts[0] == 0).all()          # nobody holds it
  assert (ids[1] == -1).all() and (wts[1] == 0).all()          # its only user holds nothing else
  assert all(0 not in r and 1 not in r for r in ids.tolist())
  # the fixture does force the tie rule: some row reaches both duplicates with bit-equal omega, inside its top 4,
  # and lists column 2 directly before column 3
  tied = [i for i in range(4, 20) if om[i, 2] > 0 and om[i, 2] == om[i, 3] and 2 in ids[i] and 3 in ids[i]]
  assert tied
  for i in tied:
    r = ids[i].tolist()
    assert r.index(3) == r.index(2) + 1 and wts[i, r.index(2)] == wts[i, r.index(3)]
  # a cut through the tie keeps the lower id
  cut = [i for i in tied if ids[i].tolist().index(2) < 3]
  for i in cut:
    k = ids[i].tolist().index(2) + 1
    assert uu.item_graph(m, k, block=7)[0][i, -1] == 2
  assert cut


def test_the_degree_weights_are_finite_for_empty_rows_and_columns():
  from recoder_amd import ultragcn
  m = uu.graph_fixture()
  m = sp.vstack([m, sp.csr_matrix((2, 20), dtype=np.float32)]).tocsr()      # two users without items
  bu, bi = uu.degree_weights(m)
  r, d = np.diff(m.indptr), np.bincount(m.indices, minlength=20)
  assert np.isfinite(bu).all() and np.isfinite(bi).all() and (bu[r == 0] == 0).all() and (bi[d == 0] == 1).all()
  assert bu[0] == np.float32(np.sqrt(2.0)) and bi[1] == np.float32(1 / np.sqrt(2.0))
  k = int(np.argmax(r))
  assert bu[k] == np.float32(np.sqrt(r[k] + 1.0) / r[k])
  hu, hi = ultragcn.degree_weights(r, d)                      # the module's host computation is the same one
  assert np.array_equal(hu, bu) and np.array_equal(hi, bi) and hu.dtype == hi.dtype == np.float32


# ------------------------------------------------------------- refusals
def _no_gpu(monkeypatch):
  from recoder_amd import _als_lib, device
  import recoder_amd.model as model_mod

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)
  monkeypatch.setattr(_als_lib, "load", no_gpu)              # (the library is never touched either)


def _dataset(n=40):
  from recoder_amd.data import RecommendationDataset
  return RecommendationDataset(sp.csr_matrix(np.eye(n, dtype=np.float32)))


def _mf(h=4, **kw):
  from recoder_amd.nn import MatrixFactorization
  return MatrixFactorization(h, **kw)


def _uninitialised(rec):
  return not rec._Recoder__model_initialized and rec.ultragcn_state is None and rec.ultragcn_history == [] and \
      rec.optimizer is None


def test_train_ultragcn_exists_with_the_signature_of_the_contract():
  from recoder_amd import ultragcn
  from recoder_amd.model import Recoder
  sig = inspect.signature(Recoder.train_ultragcn)
  assert list(sig.parameters) == ["self", "train_dataset", "num_epochs", "batch_size", "lr", "reg", "num_negatives",
                                  "negative_weight", "neighbours", "item_weight", "w", "seed", "resume"]
  d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
  assert d["seed"] == 0 and d["resume"] is False and len(d["w"]) == 4 and "num_layers" not in d
  assert ultragcn.check_config(_mf(64), *(d[k] for k in list(sig.parameters)[2:-1]))[0] == 0
  rec = Recoder(model=_mf(4))
  assert rec.ultragcn_state is None and rec.ultragcn_history == []
  assert (ultragcn.MAX_BATCH, ultragcn.MAX_NEGATIVES, ultragcn.MAX_NEIGHBOURS, ultragcn.MAX_ENTRIES) == \
      (4096, 1024, 64, 1 << 22)
  assert ultragcn.METHOD.name == "UltraGCN" and ultragcn.METHOD.method == "train_ultragcn" and \
      ultragcn.METHOD.max_batch == 4096 and ultragcn.METHOD.min_layers == 0


def test_check_config_accepts_the_contract():
  from recoder_amd import ultragcn
  assert ultragcn.check_config(_mf(4), 3, 256, 0.01, 1e-4, 7, 2, 5, 0.5, [1, 0, 1, 0], -3) == \
      (0, 3, 256, 0.01, 1e-4, 7, 2.0, 5, 0.5, (1.0, 0.0, 1.0, 0.0), -3)
  assert ultragcn.check_config(_mf(512), 0, 4096, np.float32(0.5), 0, 1023, 0, 0, 0, np.zeros(4), 0)[5:10] == \
      (1023, 0.0, 0, 0.0, (0.0, 0.0, 0.0, 0.0))
  assert ultragcn.active_neighbours(10, 0.0) == 0 == ultragcn.active_neighbours(0, 1.0)
  assert ultragcn.active_neighbours(10, 1e-3) == 10


def test_train_ultragcn_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd import ultragcn
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_ultragcn trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_ultragcn trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_ultragcn needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_ultragcn needs dropout_prob == 0"),
    (_mf(0), {}, "train_ultragcn supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_ultragcn supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..4096 \\(got 0\\)"),
    (_mf(4), {"batch_size": 4097}, "batch_size must be an integer in 1..4096 \\(got 4097\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"num_negatives": 0}, "num_negatives must be an integer in 1..1024 \\(got 0\\)"),
    (_mf(4), {"num_negatives": 1025}, "num_negatives must be an integer in 1..1024 \\(got 1025\\)"),
    (_mf(4), {"num_negatives": 8.0}, "num_negatives must be an integer in 1..1024"),
    (_mf(4), {"neighbours": -1}, "neighbours must be an integer in 0..64 \\(got -1\\)"),
    (_mf(4), {"neighbours": 65}, "neighbours must be an integer in 0..64 \\(got 65\\)"),
    (_mf(4), {"batch_size": 4096, "num_negatives": 1024}, "must be at most 4194304 \\(got 4096 \\* 1035\\)"),
    (_mf(4), {"negative_weight": -1}, "negative_weight must be finite and >= 0"),
    (_mf(4), {"negative_weight": float("nan")}, "negative_weight must be finite and >= 0"),
    (_mf(4), {"item_weight": -0.1}, "item_weight must be finite and >= 0"),
    (_mf(4), {"item_weight": float("inf")}, "item_weight must be finite and >= 0"),
    (_mf(4), {"w": (1, 1, 1)}, "w must be four numbers"),
    (_mf(4), {"w": (1, 1, 1, 1, 1)}, "w must be four numbers"),
    (_mf(4), {"w": 1.0}, "w must be four numbers"),
    (_mf(4), {"w": "1111"}, "w must be four numbers"),
    (_mf(4), {"w": (1, -1e-9, 1, 1)}, "w\\[1\\] must be finite and >= 0"),
    (_mf(4), {"w": (1, 1, 1, float("nan"))}, "w\\[3\\] must be finite and >= 0"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"seed": 2 ** 63}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_ultragcn"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.train_ultragcn(_dataset(), **kw)
    assert _uninitialised(rec), message
  with pytest.raises(TypeError):
    Recoder(model=_mf(4)).train_ultragcn(_dataset(), num_layers=2)      # (nothing is propagated: not an argument)
  state = {"num_layers": 0, "E0": (torch.zeros(40, 4), torch.zeros(40, 4))}
  with pytest.raises(ValueError, match="do not match the model's"):
    ultragcn.check_resume(state, 0, ((40, 4), (41, 4)))
  ultragcn.check_resume(state, 0, ((40, 4), (40, 4)))
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 0\\)"):
    ultragcn.check_resume(dict(state, num_layers=2), 0)
  rec = Recoder(model=_mf(4))                                  # (another method's state is not this one's)
  rec.lightgcn_state = rec.ssm_state = state
  with pytest.raises(ValueError, match="resume=True needs the state of an earlier train_ultragcn"):
    rec.train_ultragcn(_dataset(), resume=True)


def test_the_wrappers_refuse_sizes_outside_the_kernels_limits(monkeypatch):
  from recoder_amd import ultragcn
  _no_gpu(monkeypatch)
  i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
  f32 = lambda *s: torch.zeros(s, dtype=torch.float32)
  X, Y = f32(5, 4), f32(6, 4)

  def grad(T, R, K, w=(1, 1, 1, 1)):
    E = 1 + R + K
    ultragcn.grad(i32(T), i32(T), R, K, 0, 0, X, Y, f32(5), f32(6), None, None, w, 1.0, 1.0, i32(1, 1), f32(1, 1),
                  f32(1, 4), f32(1), f32(1, 3))
  for T, R, K in ((4097, 1, 0), (8, 0, 0), (8, 1025, 0), (8, 1, 65), (8, 1, -1)):
    with pytest.raises(ValueError, match="rk_als_ugcn_grad needs 1 <= T <= 4096, 1 <= R <= 1024, 0 <= K <= 64"):
      grad(T, R, K)
  with pytest.raises(ValueError, match="w must be four numbers"):
    grad(8, 1, 0, w=(1, 1))
  with pytest.raises(ValueError, match="w\\[0\\] must be finite and >= 0"):
    grad(8, 1, 0, w=(-1, 1, 1, 1))
  for n, T, E in ((9, 4, 2), (8, 4, 1), (0, 0, 2)):
    with pytest.raises(ValueError, match="rk_als_ugcn_scatter needs n = T E keys"):
      ultragcn.scatter(i32(n), torch.zeros(n, dtype=torch.int64), E, i32(T), f32(n), X, 1.0, f32(6, 4), i32(6))
  # the item graph's n x n Gram against one device's memory, as EASE checks its own
  ucsr = type("C", (), dict(shape=(10, 400000), indptr=None, indices=None))
  with pytest.raises(ValueError, match="item graph over n = 400000 items needs .* more than one device's memory"):
    ultragcn.item_graph(ucsr, 10)
  ucsr.shape = (10, 5000)
  with pytest.raises(ValueError, match="needs [0-9]+ bytes of device memory, 1000 are free"):
    ultragcn.item_graph(ucsr, 10, free_bytes=1000)
  with pytest.raises(ValueError, match="neighbours must be an integer in 1..64"):
    ultragcn.item_graph(ucsr, 0)
  # UltraGCN-base asks for no n x n memory: the fit's bytes at a million items stay far below the Gram's
  base = ultragcn.required_bytes(100000, 1000000, 64, 10 ** 7, 1024, 128, 0)
  assert base < 4 * 10 ** 9 < 4 * 10 ** 12 == 1000000 * 1000000 * 4 < ultragcn.required_bytes(
      100000, 1000000, 64, 10 ** 7, 1024, 128, 10)
  with pytest.raises(ValueError, match="UltraGCN over 100000 users x 1000000 items .* more than one device's memory"):
    ultragcn.check_memory(100000, 1000000, 64, 10 ** 7, 1024, 128, 10, free_bytes=float("inf"))
  assert ultragcn.check_memory(100000, 1000000, 64, 10 ** 7, 1024, 128, 0, free_bytes=float("inf")) == base


def test_train_ultragcn_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="train_ultragcn runs on one GPU"):
    rec.train_ultragcn(_dataset())
  assert _uninitialised(rec)
