"""CPU: the float64 restatement's own pins (tests/gfcf_util.py), GraphFilterModel's model_params, what
train_gfcf and the memory check refuse before any GPU work (and in which order), and the argument checks of
rk_ease_lowrank_add, which need no device."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import gfcf_util as gu
from tests.abi_util import built  # noqa: F401  (a fixture)


# ------------------------------------------------------- the restatement's own pins
def _tiny():
  """Users {0, 1}, {1}, {} over three items, item 2 held by nobody: r = (2, 1, 0), d = (1, 2, 0)."""
  return sp.csr_matrix(np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]], np.float32))


def test_restatement_on_a_graph_worked_by_hand():
  """Rn = [[1/sqrt2, 1/2, 0], [0, 1/sqrt2, 0], 0]; G = Rn^T Rn = [[1/2, sqrt2/4, 0], [sqrt2/4, 3/4, 0], 0] has
  the eigenvalues 1 and 1/4; the top eigenvector is D_I^1/2 1 normalised, (1, sqrt2, 0) / sqrt3, so
  D_I^-1/2 v v^T D_I^1/2 = [[1, 2, 0], [1, 2, 0], 0] / 3; at rank 2, V V^T is the identity on the held items
  and the filter is diag(1, 1, 0)."""
  X = _tiny()
  s2 = np.sqrt(2.0)
  ri, di, dh = gu.scales_f64(X)
  np.testing.assert_allclose(ri, [1 / s2, 1.0, 0.0], rtol=1e-15)
  np.testing.assert_allclose(di, [1.0, 1 / s2, 0.0], rtol=1e-15)
  np.testing.assert_allclose(dh, [1.0, s2, 0.0], rtol=1e-15)
  G = np.array([[0.5, s2 / 4, 0], [s2 / 4, 0.75, 0], [0, 0, 0]])
  np.testing.assert_allclose(gu.gram_f64(X), G, atol=1e-15)
  sigma, V = gu.top_eigenvectors(G, 2)
  np.testing.assert_allclose(sigma, [1.0, 0.5], atol=1e-14)
  np.testing.assert_allclose(np.abs(V[:, 0]), np.array([1, s2, 0]) / np.sqrt(3.0), atol=1e-14)
  L1 = np.array([[1, 2, 0], [1, 2, 0], [0, 0, 0]]) / 3.0
  np.testing.assert_allclose(gu.weights_f64(X, 1, 0.6), G + 0.6 * L1, atol=1e-14)
  np.testing.assert_allclose(gu.weights_f64(X, 2, 0.5), G + 0.5 * np.diag([1.0, 1.0, 0.0]), atol=1e-14)
  W = gu.weights_f64(X, 1, 0.6)
  assert not W[2].any() and not W[:, 2].any() and W[0, 1] != W[1, 0]          # (not symmetric)
  # a given basis is used as it is
  np.testing.assert_allclose(gu.weights_f64(X, 1, 0.6, V=-V[:, :1]), W, atol=1e-14)
  # scores: the user's stored values times W
  Xv = X.copy()
  Xv.data[:] = [2.0, 3.0, 5.0]
  np.testing.assert_allclose(gu.scores_f64(Xv, W), np.asarray(Xv.todense(), np.float64) @ W, atol=1e-14)


def test_stored_values_play_no_part_in_the_restated_fit():
  X = _tiny()
  Xv = X.copy()
  Xv.data[:] = [2.0, 0.5, 7.0]
  np.testing.assert_array_equal(gu.weights_f64(Xv, 1, 0.3), gu.weights_f64(X, 1, 0.3))


def test_the_bounds_are_the_stated_formulas():
  rng = np.random.RandomState(0)
  A, V, a, b = rng.randn(5, 5), rng.randn(5, 3), rng.randn(5), rng.randn(5)
  got = gu.lowrank_bound(A, V, a, b, -0.5)
  i, j = 1, 4
  want = (3 + 4) * 2.0 ** -23 * (abs(A[i, j]) + abs(0.5 * a[i] * b[j]) * np.sum(np.abs(V[i] * V[j])))
  assert abs(got[i, j] - want) <= 1e-18 and got.shape == (5, 5)
  X = sp.csr_matrix((rng.rand(30, 6) < 0.6).astype(np.float32))
  np.testing.assert_array_equal(gu.gram_bound(X), np.diff(X.tocsc().indptr).max() * 2.0 ** -23 * gu.gram_f64(X))


# ---------------------------------------------------------------- the model class
def test_package_exports_the_model():
  import recoder_amd
  from recoder_amd.nn import FactorizationModel, GraphFilterModel, ItemItemModel
  assert recoder_amd.GraphFilterModel is GraphFilterModel and "GraphFilterModel" in recoder_amd.__all__
  assert issubclass(GraphFilterModel, ItemItemModel) and issubclass(GraphFilterModel, FactorizationModel)
  m = GraphFilterModel()
  # the best Recall@20 of the exact-eigenvector grid in profiles/gfcf_quality.jsonl
  assert (m.rank, m.alpha) == (128, 3.0) and GraphFilterModel.fit_method == "train_gfcf"
  for bad in (dict(rank=0), dict(rank=2.5), dict(alpha=-1.0), dict(alpha=float("nan"))):
    with pytest.raises(ValueError):
      GraphFilterModel(**bad)


def test_the_grid_on_record_puts_the_defaults_first():
  import json
  import os
  from recoder_amd.nn import GraphFilterModel
  path = os.path.join(os.path.dirname(gu.SLICE), "..", "..", "profiles", "gfcf_quality.jsonl")
  rows = [json.loads(l) for l in open(path)]
  exact = [r for r in rows if r["bench"] == "gfcf_quality" and r.get("basis") == "exact"]
  assert len(exact) == 20
  best = max(exact, key=lambda r: r["recall20"])
  m = GraphFilterModel()
  assert (best["rank"], best["alpha"]) == (m.rank, m.alpha)


def test_model_params_round_trip_and_torch_forward():
  from recoder_amd.nn import GraphFilterModel
  m = GraphFilterModel(rank=7, alpha=0.25)
  assert m.model_params() == {"rank": 7, "alpha": 0.25}
  m2 = GraphFilterModel()
  m2.load_model_params(m.model_params())
  assert (m2.rank, m2.alpha) == (7, 0.25) and m2.model_params() == m.model_params()
  with pytest.raises(ValueError):
    m2.load_model_params({"rank": 0, "alpha": 1.0})
  m.init_model(num_items=3)
  assert list(m.state_dict()) == ["item_weights"] and m.item_weights.shape == (3, 3) and not bool(m.item_weights.any())
  W = gu.weights_f64(_tiny(), 1, 0.25)
  m.item_weights.data.copy_(torch.from_numpy(W.astype(np.float32)))
  x = torch.tensor([[1.0, 2.0, 0.0]])
  np.testing.assert_allclose(m(x).numpy(), x.numpy().astype(np.float64) @ W, rtol=1e-6)


# ------------------------------------------------------------ what train_gfcf refuses
def _no_gpu(monkeypatch):
  import recoder_amd.model as model_mod
  from recoder_amd import device

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)


def _dataset(n_users=20, n=15):
  from recoder_amd.data import RecommendationDataset
  X = sp.random(n_users, n, density=0.3, format="csr", dtype=np.float32, random_state=np.random.RandomState(4))
  X.data[:] = 1.0
  return RecommendationDataset(X)


# every ValueError of check_config, in the order it checks: each case is valid in all that comes before it
BAD = [(dict(rank=0), "rank must be an integer >= 1"),
       (dict(rank=2.0), "rank must be an integer >= 1"),
       (dict(rank=True), "rank must be an integer >= 1"),
       (dict(alpha=-0.5), "alpha must be finite and >= 0"),
       (dict(alpha=float("inf")), "alpha must be finite and >= 0"),
       (dict(alpha=float("nan")), "alpha must be finite and >= 0"),
       (dict(alpha="x"), "alpha must be finite and >= 0"),
       (dict(oversample=-1), "oversample must be an integer >= 0"),
       (dict(oversample=1.5), "oversample must be an integer >= 0"),
       (dict(rank=500, oversample=13), r"rank \+ oversample must be at most 512 \(got 500 \+ 13\)"),
       (dict(num_power_iterations=-1), "num_power_iterations must be an integer >= 0"),
       (dict(seed=0.5), "seed must be an integer")]


@pytest.mark.parametrize("kw,text", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_value_error_of_check_config(monkeypatch, kw, text):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  _no_gpu(monkeypatch)
  rec = Recoder(model=GraphFilterModel(rank=5, alpha=0.5))
  with pytest.raises(ValueError, match=text):
    rec.train_gfcf(_dataset(), **kw)
  assert rec.model.model_params() == {"rank": 5, "alpha": 0.5}
  assert rec.optimizer is None and rec.items is None and rec.model.item_weights is None


def test_the_order_of_the_checks(monkeypatch):
  from recoder_amd import gfcf
  from recoder_amd.nn import GraphFilterModel, ShallowAutoencoder
  m = GraphFilterModel()
  all_bad = dict(rank=0, alpha=-1.0, oversample=-1, num_power_iterations=-1, seed=0.5)
  with pytest.raises(ValueError, match="train_gfcf fits a GraphFilterModel, not ShallowAutoencoder"):
    gfcf.check_config(ShallowAutoencoder(), **all_bad)
  # (what the call raises while the argument is still bad, then its repair)
  steps = [("rank must", dict(rank=3)), ("alpha must", dict(alpha=1.0)), ("oversample must", dict(oversample=600)),
           ("at most 512", dict(oversample=16)), ("num_power_iterations must", dict(num_power_iterations=2)),
           ("seed must", dict(seed=7))]
  for text, repair in steps:
    with pytest.raises(ValueError, match=text):
      gfcf.check_config(m, **all_bad)
    all_bad.update(repair)
  assert gfcf.check_config(m, **all_bad) == (3, 1.0, 19)
  assert gfcf.check_config(m, 496, 0, 16, 0, -3) == (496, 0.0, 512)


def test_train_gfcf_is_single_gpu_and_comes_after_the_config(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=GraphFilterModel(rank=4))
  with pytest.raises(ValueError, match="rank"):                    # (A before B)
    rec.train_gfcf(_dataset(), rank=0)
  with pytest.raises(NotImplementedError, match="train_gfcf"):
    rec.train_gfcf(_dataset(), rank=6)
  assert rec.model.rank == 4 and rec.model.item_weights is None


def test_a_refused_size_or_rank_leaves_nothing_behind(monkeypatch):
  from recoder_amd import gfcf
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  _no_gpu(monkeypatch)
  # a 1 M-item catalogue gets the ValueError that names it, not an allocation
  rec = Recoder(model=GraphFilterModel(rank=4), num_items=1000000, num_users=2000000)
  with pytest.raises(ValueError, match="n = 1000000") as e:
    rec.train_gfcf(_dataset(), rank=8, alpha=0.7)
  assert str(gfcf.required_bytes(2000000, 1000000, 24, 0)) in str(e.value)
  assert rec.model.model_params() == {"rank": 4, "alpha": 3.0}
  assert rec.optimizer is None and rec.items is None and rec.model.item_weights is None
  # the sketch cannot be wider than the matrix: svd.check_rank's error, before any GPU work
  rec = Recoder(model=GraphFilterModel(rank=4))
  with pytest.raises(ValueError, match=r"= 24 exceeds min\(users, items\) = 15"):
    rec.train_gfcf(_dataset(), rank=8)
  assert rec.model.model_params() == {"rank": 4, "alpha": 3.0}
  assert rec.optimizer is None and rec.items is None and rec.model.item_weights is None


def test_train_points_at_train_gfcf(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  _no_gpu(monkeypatch)
  rec = Recoder(model=GraphFilterModel())
  with pytest.raises(ValueError) as e:
    rec.train(_dataset())
  assert str(e.value) == ("a GraphFilterModel is fitted in closed form from the normalised interaction graph: call "
                          "train_gfcf(train_dataset)")
  assert rec.optimizer is None and rec.items is None


def test_other_closed_form_methods_refuse_the_model(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel, ShallowAutoencoder
  _no_gpu(monkeypatch)
  with pytest.raises(ValueError, match="train_ease fits a ShallowAutoencoder, not GraphFilterModel"):
    Recoder(model=GraphFilterModel()).train_ease(_dataset())
  with pytest.raises(ValueError, match="train_gfcf fits a GraphFilterModel, not ShallowAutoencoder"):
    Recoder(model=ShallowAutoencoder()).train_gfcf(_dataset())


# ------------------------------------------------------------------- memory
def test_memory_arithmetic_without_touching_a_device(monkeypatch):
  from recoder_amd import gfcf, svd
  _no_gpu(monkeypatch)
  u, n, l, nnz = 10000, 7915, 144, 1100000
  need = gfcf.required_bytes(u, n, l, nnz)
  # the n x n parameter, the SVD's own buffers (both CSRs with a value array each), its two result tables
  # and r^-1/2, d^-1/2, d^1/2
  assert need == n * n * 4 + svd.required_bytes(u, n, l, nnz) + (u + n) * l * 4 + (u + 2 * n) * 4
  assert gfcf.required_bytes(u, n, l, nnz, allocate_matrix=False) == need - n * n * 4
  assert need < 2 * n * n * 4, "no second n x n image"
  assert gfcf.check_memory(u, n, l, nnz, free_bytes=need) == need
  with pytest.raises(ValueError) as e:
    gfcf.check_memory(u, n, l, nnz, free_bytes=need - 1)
  assert "n = 7915" in str(e.value) and str(need) in str(e.value) and str(need - 1) in str(e.value)
  assert gfcf.check_memory(u, n, l, nnz, free_bytes=need - n * n * 4, allocate_matrix=False) == need - n * n * 4
  with pytest.raises(ValueError, match="more than one device's memory"):
    gfcf.check_memory(10, 1000000, 32, 0)
  with pytest.raises(ValueError, match="at least one item"):
    gfcf.check_memory(10, 0, 32, 0)


# ------------------------------------------------- rk_ease_lowrank_add's argument checks
def test_lowrank_add_refuses_bad_arguments_without_a_device(built):
  from recoder_amd import _ease_lib
  lib = _ease_lib.load()
  P = 4096                                  # (any non-null address: a refused call reads nothing)
  good = dict(A=P, n=10, lda=10, V=P, k=4, ldv=4, a=P, b=P, alpha=1.0, lo=0, hi=10)

  def call(**kw):
    g = dict(good, **kw)
    return lib.rk_ease_lowrank_add(g["A"], g["n"], g["lda"], g["V"], g["k"], g["ldv"], g["a"], g["b"], g["alpha"],
                                   g["lo"], g["hi"], None)
  cases = [(dict(A=None), "null pointer"), (dict(V=None), "null pointer"), (dict(a=None), "null pointer"),
           (dict(b=None), "null pointer"), (dict(n=0, hi=0), "bad sizes"), (dict(lda=9), "bad sizes"),
           (dict(k=0), "k must be in"), (dict(k=513, ldv=513), "k must be in"), (dict(ldv=3), "ldv >= k"),
           (dict(lo=-1), "bad row range"), (dict(hi=11), "bad row range"), (dict(lo=6, hi=5), "bad row range")]
  for kw, text in cases:
    assert call(**kw) < 0, kw
    msg = lib.rk_ease_last_error().decode()
    assert msg.startswith("rk_ease_lowrank_add: ") and text in msg, (kw, msg)
  assert call(lo=5, hi=5) == 0              # (an empty range is valid and launches nothing)
