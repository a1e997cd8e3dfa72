"""CPU: the identities ``Recoder.explain`` rests on, in the float64 restatement of tests/explain_util.py; the f32
restatement's Cholesky held to tests/foldin_util.py's bit for bit; the order of the candidates; the three entry points
in their libraries, headers and bindings; every refusal of ``explain`` before any GPU work."""
import inspect
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp

from tests import explain_util as U
from tests import foldin_util as FU
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

F32 = np.float32


# ------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("h", U.HS)
def test_mf_contributions_and_baseline_sum_to_the_folded_score(h):
  """sum of ALL contributions + baseline == y_j . x_u + b_j with x_u the float64 fold-in: relative error <= 1e-10."""
  csr, items = U.histories()
  p = U.mf_problem(h)
  worst = 0.0
  for name, alpha, use_data, bias_given in U.VARIANTS:
    v, bias = U.variant_inputs(p, bias_given)
    for u, (cols, vals) in enumerate(U._rows(csr, use_data)):
      ids, c, base, tot, score, scale = U.mf_row64(cols, vals, p["Y"], p["G"], v, bias, alpha, items[u], 5)
      for q, j in enumerate(items[u]):
        if j < 0:
          assert (ids[q] == -1).all() and not c[q].any() and base[q] == 0 and tot[q] == 0
          continue
        err = abs(tot[q] - score[q]) / max(abs(score[q]), scale[q], 1e-300)
        worst = max(worst, err)
        assert err <= 1e-10, (name, u, q, err)
        if not len(cols):
          assert tot[q] == base[q] and (ids[q] == -1).all()
  print("h = %d: identity holds to %.3g" % (h, worst))


def test_item_contributions_sum_to_the_matrix_product():
  csr, items = U.histories()
  W = U.dense_w()
  S = np.asarray(csr.astype(np.float64) @ W.astype(np.float64))
  ids, c, base, tot = U.item_explain(csr, W, items, 5, pair=U.item_pair64)
  for u in range(items.shape[0]):
    for q, j in enumerate(items[u]):
      if j >= 0:
        scale = abs(csr[u].astype(np.float64)) @ np.abs(W[:, j].astype(np.float64))
        assert abs(tot[u, q] - S[u, j]) <= 1e-10 * max(scale[0], 1e-300)
  assert not base.any()


# ----------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("h", [1, 3, 33, 128])
def test_factor_and_solves_are_foldin_utils_bit_for_bit(h):
  """``factor32`` + ``solve32`` on the fold-in's own right-hand side give ``foldin_row32``'s row."""
  p = FU.problem(h)
  csr = p["csr"]
  for u in (0, 1, 2, 3, 9):
    lo, hi = csr.indptr[u], csr.indptr[u + 1]
    cols, vals = csr.indices[lo:hi], csr.data[lo:hi]
    want, st = FU.foldin_row32(cols, vals, p["Y"], p["G"], p["v"], p["bias"], FU.ALPHA)
    L, dg, status = U.factor32(cols, vals, p["Y"], p["G"], FU.ALPHA)
    assert st == status == 0
    coef = U.coef32(cols, vals, p["bias"], FU.ALPHA)
    r = -p["v"].copy()
    for e in range(len(cols)):
      r = U._fma(coef[e], p["Y"][cols[e]], r, F32)
    assert U.solve32(L, dg, r).tobytes() == want.tobytes(), u
  s = FU.singular_problem()
  assert U.factor32([], None, s["Y"], s["G"], 10.0)[2] == 1


def test_order_and_padding():
  f = F32
  c = np.array([1.0, np.nan, 2.0, -0.0, 2.0, 0.0, -3.0, np.nan], f)
  assert U.order(c).tolist() == [2, 4, 0, 3, 5, 6, 1, 7]
  ids, vals = U.select(np.arange(10, 18), c, 3)
  assert ids.tolist() == [12, 14, 10] and vals.tolist() == [2.0, 2.0, 1.0]
  ids, vals = U.select([4, 9], np.array([-1.0, -1.0], f), 5)
  assert ids.tolist() == [4, 9, -1, -1, -1] and vals.tolist() == [-1.0, -1.0, 0, 0, 0]
  # the planted case: W zero but W[3, 7] = 2, W[5, 7] = -1, W[9, 7] = 2; history {3, 5, 9}, target 7, m = 2
  W = np.zeros((12, 12), f)
  W[3, 7], W[5, 7], W[9, 7] = 2, -1, 2
  ids, vals, base, tot = U.item_pair32(np.array([3, 5, 9]), None, W[[3, 5, 9], 7], 2)
  assert ids.tolist() == [3, 9] and vals.tolist() == [2.0, 2.0] and base == 0 and tot == 3.0
  # the singular case: every contribution +0, the first entries kept
  s = U.singular_case()
  out = U.mf_explain32(s["csr"], s["Y"], s["G"], s["v"], s["bias"], s["alpha"], s["items"], 3)
  assert out[4].tolist() == [1] and out[0][0].tolist() == [[0, 2, -1], [-1, -1, -1], [0, 2, -1]]
  assert not out[1].any() and not out[2].any() and not out[3].any()


def test_cases_reach_every_branch():
  csr, items = U.histories()
  lens = np.diff(csr.indptr).tolist()
  for m in U.MS:
    assert {0, 1, m - 1, m, m + 1, 63, 64, 65, 300} <= set(lens)
  assert U.B == 7 and all(hi - lo == 7 for lo, hi in U.BATCHES) and U.N_ITEMS == 300
  in_history = [items[u, q] in csr[u].indices for u in range(10) for q in range(3)]
  assert any(in_history) and (items == -1).any() and any(len(set(r)) < 3 for r in items.tolist())
  assert (csr.data != 1).any() and (csr.data < 0).any()
  W = U.dense_w()
  assert (W < 0).any()
  ids, c, _, _ = U.want_items("dense", 5, False)
  assert any(c[u, q, a] == c[u, q, a + 1] and ids[u, q, a] < ids[u, q, a + 1] and ids[u, q, a + 1] >= 0
             for u in range(10) for q in range(3) for a in range(4)), "no exact tie among the kept contributions"
  for K in U.KS:
    nid, w, count = U.neighbour_lists(K)
    assert (count == 0).any() and (count == K).any() and not (nid == U.ABSENT).any()
  assert (items == U.ABSENT).any()


# ------------------------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound(built):
  from recoder_amd import _als_lib, _ease_lib, _slim_lib, explain
  for lib, header, binding, names in (
      (built.EASE_LIB, "recoder_ease.h", _ease_lib, ("rk_ease_explain", "rk_ease_explain_max_contributors")),
      (built.SLIM_LIB, "recoder_slim.h", _slim_lib, ("rk_slim_explain",)),
      (built.ALS_LIB, "recoder_als.h", _als_lib, ("rk_als_explain", "rk_als_explain_workspace_bytes"))):
    for name in names:
      assert name in exports(lib) and name in declared([os.path.join(INC, header)]) and name in binding.SIGNATURES
  assert _ease_lib.load().rk_ease_explain_max_contributors() == explain.MAX_CONTRIBUTORS == U.MAX_M == 64
  als = _als_lib.load()
  assert als.rk_als_explain_workspace_bytes(0) == 256 and als.rk_als_explain_workspace_bytes(65) == 512
  assert als.rk_als_explain_workspace_bytes(-1) < 0
  assert len(_als_lib.SIGNATURES["rk_als_explain"][1]) == 24
  assert len(_ease_lib.SIGNATURES["rk_ease_explain"][1]) == 15
  assert len(_slim_lib.SIGNATURES["rk_slim_explain"][1]) == 18


def test_entry_points_refuse_bad_arguments(built):
  """Sizes out of range and null pointers return the libraries' error code before any launch; no rows is a success."""
  from recoder_amd import _als_lib, _ease_lib, _slim_lib
  p = 4096                                               # (never dereferenced: every case is refused first)

  def call(fn, good, **change):
    a = list(good)
    for i, v in change.items():
      a[int(i[1:])] = v
    return fn(*a)
  ease = _ease_lib.load().rk_ease_explain
  good = [p, p, None, 2, p, 16, 16, p, 3, 5, p, p, p, p, None]
  assert call(ease, good, _9=0) == -2 and call(ease, good, _9=65) == -2 and call(ease, good, _8=0) == -2
  assert call(ease, good, _5=15) == -2 and call(ease, good, _3=-1) == -2 and call(ease, good, _6=0) == -2
  for i in (0, 1, 4, 7, 10, 11, 12, 13):
    assert call(ease, good, **{"_%d" % i: None}) == -2, i
  assert call(ease, good, _3=0) == 0
  assert b"rk_ease_explain" in _ease_lib.load().rk_ease_last_error()
  slim = _slim_lib.load().rk_slim_explain
  good = [p, p, None, 2, 16, p, p, p, 4, 1, p, 3, 5, p, p, p, p, None]
  assert call(slim, good, _12=0) == -2 and call(slim, good, _12=65) == -2 and call(slim, good, _11=0) == -2
  assert call(slim, good, _8=0) == -2 and call(slim, good, _9=2) == -2 and call(slim, good, _3=-1) == -2
  for i in (0, 1, 5, 6, 7, 10, 13, 14, 15, 16):
    assert call(slim, good, **{"_%d" % i: None}) == -2, i
  assert call(slim, good, _3=0) == 0
  als = _als_lib.load().rk_als_explain
  good = [p, p, None, 2, 10, p, 16, 30, 16, p, p, None, 1.0, p, 3, 5, p, p, p, p, p, p, 256, None]
  assert call(als, good, _8=0) == -2 and call(als, good, _8=129, _6=129) == -2 and call(als, good, _6=15) == -2
  assert call(als, good, _15=0) == -2 and call(als, good, _15=65) == -2 and call(als, good, _14=0) == -2
  assert call(als, good, _3=-1) == -2 and call(als, good, _7=0) == -2 and call(als, good, _22=255) == -2
  assert call(als, good, _4=65) == -2                    # (the workspace holds 64 entries)
  for alpha in (-1.0, float("nan"), float("inf")):
    assert call(als, good, _12=alpha) == -2, alpha
  for i in (0, 1, 5, 9, 10, 13, 16, 17, 18, 19, 20, 21):
    assert call(als, good, **{"_%d" % i: None}) == -2, i
  assert call(als, good, _3=0) == 0


# ------------------------------------------------------------------------------------------------------- refusals
def _no_gpu(monkeypatch):
  from recoder_amd import _als_lib, _ease_lib, _slim_lib, device
  import recoder_amd.model as model_mod

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  for lib in (_als_lib, _ease_lib, _slim_lib):
    monkeypatch.setattr(lib, "load", no_gpu)


def test_signature():
  from recoder_amd import explain, foldin
  from recoder_amd.model import Recoder
  assert list(inspect.signature(Recoder.explain).parameters) == \
      ["self", "users_interactions", "items", "num_contributors", "alpha", "reg"]
  d = inspect.signature(Recoder.explain).parameters
  assert (d["num_contributors"].default, d["alpha"].default, d["reg"].default) == \
      (5, foldin.DEFAULT_ALPHA, foldin.DEFAULT_REG)
  assert explain.Explanation._fields == ("contributors", "contributions", "baseline", "total")
  assert "recommend_folded" in Recoder.explain.__doc__ and "NOT the score of the trained user row" in Recoder.explain.__doc__


def test_explain_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd import foldin
  from recoder_amd.model import Recoder
  from recoder_amd.nn import (DynamicAutoencoder, LowRankShallowAutoencoder, MatrixFactorization,
                              NeuralMatrixFactorization, RandomWalkItemModel, ShallowAutoencoder, SparseLinearModel,
                              UserNeighbourhoodModel, VariationalAutoencoder)
  _no_gpu(monkeypatch)
  batch = types.SimpleNamespace(interactions_matrix=sp.csr_matrix(np.eye(5, 12, dtype=F32)))
  items = np.zeros((5, 2), np.int64)

  def ready(model):
    model.init_model(num_items=12, num_users=7)              # (on the host: nothing here reaches a device)
    return model
  mf = lambda h=4, **kw: MatrixFactorization(h, **kw)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "not DynamicAutoencoder"),
    (VariationalAutoencoder(hidden_layers=[8, 4]), {}, "not VariationalAutoencoder"),
    (NeuralMatrixFactorization(), {}, "not NeuralMatrixFactorization"),
    (UserNeighbourhoodModel(), {}, "not UserNeighbourhoodModel"),
    (LowRankShallowAutoencoder(), {}, "not LowRankShallowAutoencoder"),
    (ready(mf(4, activation_type="tanh")), {}, "MatrixFactorization: .* needs activation_type='none' \\(got 'tanh'\\)"),
    (ready(mf(foldin.MAX_H + 1)), {}, "MatrixFactorization: .* embedding sizes 1..128 \\(got 129\\)"),
    (mf(4), {}, "MatrixFactorization: .* needs an initialised model"),
    (ShallowAutoencoder(), {}, "explain needs a fitted ShallowAutoencoder"),
    (SparseLinearModel(), {}, "explain needs a fitted SparseLinearModel"),
    (RandomWalkItemModel(), {}, "explain needs a fitted RandomWalkItemModel"),
    (ready(mf(4)), {"alpha": -1.0}, "MatrixFactorization: alpha must be a finite number >= 0"),
    (ready(mf(4)), {"reg": float("nan")}, "MatrixFactorization: reg must be a finite number >= 0"),
  ]
  for model_kind in (lambda: ready(mf(4)), lambda: ready(ShallowAutoencoder()), lambda: ready(SparseLinearModel())):
    name = type(model_kind()).__name__
    bad = items.copy()
    bad[2, 1] = 12
    low = items.copy()
    low[0, 0] = -2
    cases += [
      (model_kind(), {"items": bad}, "items holds an id outside \\[-1, 12\\) for %s.explain" % name),
      (model_kind(), {"items": low}, "items holds an id outside \\[-1, 12\\) for %s.explain" % name),
      (model_kind(), {"items": items[:4]}, "items has 4 rows, the batch has 5 users \\(%s" % name),
      (model_kind(), {"items": items[:, :0]}, "at least one target a user for %s" % name),
      (model_kind(), {"items": items[0]}, "items must be an integer array \\[users, targets\\] for %s" % name),
      (model_kind(), {"items": items.astype(np.float32)}, "items must be an integer array"),
      (model_kind(), {"num_contributors": 0}, "num_contributors must be an integer in \\[1, 64\\]"),
      (model_kind(), {"num_contributors": 65}, "num_contributors must be an integer in \\[1, 64\\]"),
      (model_kind(), {"num_contributors": True}, "num_contributors must be an integer in \\[1, 64\\]"),
    ]
  for model, kw, message in cases:
    kw = dict({"items": items}, **kw)
    with pytest.raises(ValueError, match=message):
      Recoder(model=model).explain(batch, **kw)
  wide = types.SimpleNamespace(interactions_matrix=sp.csr_matrix(np.eye(5, 13, dtype=F32)))
  with pytest.raises(ValueError, match="interactions_matrix has 13 columns, the ShallowAutoencoder has 12 items"):
    Recoder(model=ready(ShallowAutoencoder())).explain(wide, items)
  # more than one rank
  import torch.distributed as dist
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  for model in (ready(mf(4)), ready(ShallowAutoencoder())):
    with pytest.raises(ValueError, match="explain runs on one GPU: .* %s" % type(model).__name__):
      Recoder(model=model).explain(batch, items)
