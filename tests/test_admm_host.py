"""CPU: AdmmSlimModel's model_params, what train_admm_slim and the memory check refuse before any GPU work, the
restatements' own pins (tests/admm_util.py: the float64 loop against EASE and against the objective's KKT condition,
the f32 loop's distance from it on the input the GPU test uses), and the argument checks of rk_ease_gemm and
rk_ease_admm_update, which need no device."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import admm_util as au, ease_util
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)


# ---------------------------------------------------------------- the model class
def test_package_exports_the_model():
  import recoder_amd
  from recoder_amd.nn import AdmmSlimModel, FactorizationModel, ItemItemModel
  assert recoder_amd.AdmmSlimModel is AdmmSlimModel and "AdmmSlimModel" in recoder_amd.__all__
  assert issubclass(AdmmSlimModel, ItemItemModel) and issubclass(AdmmSlimModel, FactorizationModel)
  assert AdmmSlimModel.fit_method == "train_admm_slim"
  for bad in (dict(l1_reg=-1.0), dict(l2_reg=float("nan")), dict(rho=0.0), dict(num_iterations=0),
              dict(num_iterations=2.5), dict(nonneg=1)):
    with pytest.raises(ValueError):
      AdmmSlimModel(**bad)


def test_model_params_round_trip_and_torch_forward():
  from recoder_amd.nn import AdmmSlimModel
  m = AdmmSlimModel(l1_reg=0.5, l2_reg=7.0, rho=3.0, num_iterations=9, nonneg=False)
  want = {"l1_reg": 0.5, "l2_reg": 7.0, "rho": 3.0, "num_iterations": 9, "nonneg": False}
  assert m.model_params() == want
  m2 = AdmmSlimModel()
  assert m2.model_params() != want
  m2.load_model_params(m.model_params())
  assert m2.model_params() == want and m2.nonneg is False and isinstance(m2.num_iterations, int)
  with pytest.raises(ValueError):
    m2.load_model_params(dict(want, rho=0.0))
  m.init_model(num_items=3)
  assert list(m.state_dict()) == ["item_weights"] and m.item_weights.shape == (3, 3) and not bool(m.item_weights.any())
  W = np.array([[0, 1, 2], [3, 0, 4], [5, 6, 0]], np.float32)
  m.item_weights.data.copy_(torch.from_numpy(W))
  x = torch.tensor([[1.0, 2.0, 0.0]])
  np.testing.assert_array_equal(m(x).numpy(), x.numpy() @ W)


# ------------------------------------------------------ what train_admm_slim refuses
def _no_gpu(monkeypatch):
  import recoder_amd.model as model_mod
  from recoder_amd import device

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)


def _dataset(n_users=20, n=15, negative=False):
  from recoder_amd.data import RecommendationDataset
  X = sp.random(n_users, n, density=0.3, format="csr", dtype=np.float32, random_state=np.random.RandomState(4))
  X.data[:] = 1.0
  if negative:
    X.data[3] = -1.0
  return RecommendationDataset(X)


PARAMS = {"l1_reg": 0.5, "l2_reg": 7.0, "rho": 3.0, "num_iterations": 9, "nonneg": True}


def _untouched(rec):
  assert rec.model.model_params() == PARAMS
  assert rec.optimizer is None and rec.items is None and rec.model.item_weights is None


def test_other_models_are_refused(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel, ShallowAutoencoder, SparseLinearModel
  _no_gpu(monkeypatch)
  for model in (ShallowAutoencoder(), SparseLinearModel()):
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match="train_admm_slim fits an AdmmSlimModel, not " + type(model).__name__):
      rec.train_admm_slim(_dataset())
    assert rec.optimizer is None and rec.items is None
  with pytest.raises(ValueError, match="train_ease fits a ShallowAutoencoder, not AdmmSlimModel"):
    Recoder(model=AdmmSlimModel()).train_ease(_dataset())
  with pytest.raises(ValueError, match="train_slim fits a SparseLinearModel, not AdmmSlimModel"):
    Recoder(model=AdmmSlimModel()).train_slim(_dataset())


BAD = [(dict(l1_reg=-0.5), "l1_reg must be finite and >= 0"),
       (dict(l1_reg=float("inf")), "l1_reg must be finite and >= 0"),
       (dict(l2_reg=-1.0), "l2_reg must be finite and >= 0"),
       (dict(l2_reg="x"), "l2_reg must be finite and >= 0"),
       (dict(rho=0.0), "rho must be finite and > 0"),
       (dict(rho=float("nan")), "rho must be finite and > 0"),
       (dict(num_iterations=0), "num_iterations must be an integer >= 1"),
       (dict(num_iterations=3.0), "num_iterations must be an integer >= 1"),
       (dict(num_iterations=True), "num_iterations must be an integer >= 1"),
       (dict(nonneg=1), "nonneg must be True or False")]


@pytest.mark.parametrize("kw,text", BAD, ids=[str(i) for i in range(len(BAD))])
def test_a_bad_hyperparameter_leaves_nothing_behind(monkeypatch, kw, text):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  _no_gpu(monkeypatch)
  rec = Recoder(model=AdmmSlimModel(**PARAMS))
  with pytest.raises(ValueError, match=text):
    rec.train_admm_slim(_dataset(), **kw)
  _untouched(rec)


def test_negative_values_are_refused_with_nonneg_only(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  _no_gpu(monkeypatch)
  rec = Recoder(model=AdmmSlimModel(**PARAMS))
  with pytest.raises(ValueError, match="1 of the 90 stored values are negative"):
    rec.train_admm_slim(_dataset(negative=True), rho=5.0)
  _untouched(rec)
  # without the constraint the values are free: the call gets as far as the GPU
  with pytest.raises(AssertionError, match="GPU work started"):
    rec.train_admm_slim(_dataset(negative=True), nonneg=False)


def test_multi_gpu_is_refused_after_the_config(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=AdmmSlimModel(**PARAMS))
  with pytest.raises(ValueError, match="rho must"):                    # (A before B)
    rec.train_admm_slim(_dataset(), rho=-1.0)
  with pytest.raises(NotImplementedError, match="train_admm_slim"):
    rec.train_admm_slim(_dataset(), rho=6.0)
  _untouched(rec)


def test_an_impossible_n_is_a_value_error_before_any_allocation(monkeypatch):
  from recoder_amd import admm
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  _no_gpu(monkeypatch)
  rec = Recoder(model=AdmmSlimModel(**PARAMS), num_items=1000000)
  with pytest.raises(ValueError, match="n = 1000000") as e:
    rec.train_admm_slim(_dataset(), l1_reg=2.0)
  assert str(admm.required_bytes(1000000, 9)) in str(e.value)
  _untouched(rec)


def test_train_points_at_train_admm_slim(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  _no_gpu(monkeypatch)
  rec = Recoder(model=AdmmSlimModel())
  with pytest.raises(ValueError) as e:
    rec.train(_dataset())
  assert str(e.value) == ("an AdmmSlimModel is fitted by ADMM on the Gram matrix: call train_admm_slim(train_dataset) "
                          "(gradient steps would keep neither its zero diagonal nor its zeros)")
  assert rec.optimizer is None and rec.items is None


# ------------------------------------------------------------------- memory
def test_memory_arithmetic_without_touching_a_device(monkeypatch):
  from recoder_amd import admm, ease
  _no_gpu(monkeypatch)
  n, its = 7915, 50
  need = admm.required_bytes(n, its)
  # C, P, U, M and the inverse's workspace, whose n x n image is T: five n x n images in all, not six
  assert need == 4 * n * n * 4 + ease.inverse_workspace_bytes(n) + 4 * n * 4 + 4 + its * 24
  assert 5 * n * n * 4 < need < 5 * n * n * 4 + (1 << 23)
  assert admm.required_bytes(n, its, allocate_matrix=False) == need - n * n * 4
  assert admm.check_memory(n, its, free_bytes=need) == need
  with pytest.raises(ValueError) as e:
    admm.check_memory(n, its, free_bytes=need - 1)
  assert "n = 7915" in str(e.value) and str(need) in str(e.value) and str(need - 1) in str(e.value)
  with pytest.raises(ValueError, match="more than one device's memory"):
    admm.check_memory(1000000)
  with pytest.raises(ValueError, match="at least one item"):
    admm.check_memory(0)
  # T lies inside the workspace, after the panels and the float64 pivot block, 16-byte aligned
  off = admm._image_offset(n)
  assert off % 16 == 0 and off + n * n * 4 == ease.inverse_workspace_bytes(n)


# ------------------------------------------------------- the restatements' own pins
L2, ITERS = 50.0, 30


@pytest.fixture(scope="module")
def X():
  return au.zipf_matrix(600, 257, seed=0)


def test_without_l1_the_float64_loop_meets_ease(X):
  """l1 = 0, no sign constraint, rho = l2 / 5: the fixed point is EASE's B at reg = l2."""
  B64, _ = ease_util.fit(X, L2)
  seen = {}
  C, info = au.fit(X, 0.0, L2, L2 / 5, ITERS, False, trace=lambda it, C: seen.__setitem__(it, np.abs(C - B64).max()))
  rel = np.abs(C - B64).max() / np.abs(B64).max()
  print("l1 = 0: relative distance to EASE after 10 / 20 / 30 iterations: %.3g / %.3g / %.3g"
        % (seen[10] / np.abs(B64).max(), seen[20] / np.abs(B64).max(), rel))
  assert rel <= 1e-9
  assert not np.diag(C).any()
  # (theta = 0: C = V and U stays 0, so B - C is 0 throughout; the run shows in C - C_previous)
  assert not any(info["primal_residual"]) and info["dual_residual"][-1] < 1e-9 * info["dual_residual"][0]


@pytest.mark.parametrize("nonneg", [True, False])
def test_with_l1_the_float64_loop_is_sparse_and_meets_the_kkt_condition(X, nonneg):
  l1, rho = 2.0, 100.0
  C, info = au.fit(X, l1, L2, rho, 50, nonneg)
  d = np.diag(C)
  assert not d.any() and not np.signbit(d).any(), "the diagonal is exactly +0"
  if nonneg:
    assert C.min() == 0.0
  assert 0 < info["density"] < 0.2
  # the identity behind the bound: for C != 0 off the diagonal,
  #   grad + l1 sign(C) = ((G + l2 I)(C - B))_ij - rho (C - C_previous)_ij
  lam = np.linalg.eigvalsh(ease_util.gram(X, 0.0))[-1]
  bound = (lam + L2) * info["primal_residual"][-1] + info["dual_residual"][-1]
  kkt = au.kkt_violation(X, C, l1, L2, nonneg)
  print("nonneg %s: density %.4f, primal %.3g, dual %.3g, KKT violation %.3g (bound %.3g)"
        % (nonneg, info["density"], info["primal_residual"][-1], info["dual_residual"][-1], kkt, bound))
  assert kkt <= bound
  assert kkt <= 1e-2, "and small in absolute terms: the gradient's entries are of the order of l1 = 2"
  assert info["primal_residual"][-1] < info["primal_residual"][9] < info["primal_residual"][0]


@pytest.mark.parametrize("nonneg", [True, False])
def test_the_f32_loop_leaves_under_one_percent_undecided(X, nonneg):
  """What tests/test_admm.py relies on: on this input, the entries whose float64 |V| lies within the f32 loop's own
  error of theta (they may fall either side of the threshold) are under 1 % of the matrix."""
  l1, rho = 2.0, 100.0
  C64, i64 = au.fit(X, l1, L2, rho, ITERS, nonneg)
  C32, _ = au.fit(X, l1, L2, rho, ITERS, nonneg, dtype=np.float32)
  scale = np.abs(C64).max()
  e32 = np.abs(C32 - C64).max()
  V = i64["V"] if nonneg else np.abs(i64["V"])
  undecided = np.abs(V - l1 / rho) <= e32
  print("nonneg %s: f32 loop error %.3g of max|C64| %.3g; undecided %.4f %%"
        % (nonneg, e32, scale, 100 * undecided.mean()))
  assert undecided.mean() <= 0.01
  assert e32 <= 1e-4 * scale


# ---------------------------------------------------------------------- the library
def test_the_library_exports_the_two_new_functions(built):
  import os
  from recoder_amd import _ease_lib
  names = exports(built.EASE_LIB)
  assert names == declared([os.path.join(INC, "recoder_ease.h")]) == sorted(_ease_lib.SIGNATURES)
  assert "rk_ease_gemm" in names and "rk_ease_admm_update" in names
  assert len(_ease_lib.SIGNATURES["rk_ease_gemm"][1]) == 16
  assert len(_ease_lib.SIGNATURES["rk_ease_admm_update"][1]) == 20


def test_gemm_refuses_bad_arguments_without_a_device(built):
  from recoder_amd import _ease_lib
  lib = _ease_lib.load()
  A, B, D = 1 << 20, 2 << 20, 3 << 20       # (non-null, far apart: a refused call reads nothing)
  good = dict(A=A, lda=4, B=B, ldb=10, E=None, lde=0, D=D, ldd=10, m=10, n=10, k=4, lo=0, hi=10)

  def call(**kw):
    g = dict(good, **kw)
    return lib.rk_ease_gemm(g["A"], g["lda"], g["B"], g["ldb"], g["E"], g["lde"], g["D"], g["ldd"], g["m"], g["n"],
                            g["k"], 1.0, 1.0, g["lo"], g["hi"], None)
  cases = [(dict(A=None), "null pointer"), (dict(B=None), "null pointer"), (dict(D=None), "null pointer"),
           (dict(k=0), "bad sizes"), (dict(lda=3), "bad sizes"), (dict(ldb=9), "bad sizes"), (dict(ldd=9), "bad sizes"),
           (dict(E=4 << 20, lde=9), "bad sizes"), (dict(lo=-1), "bad row range"), (dict(hi=11), "bad row range"),
           (dict(lo=6, hi=5), "bad row range"), (dict(D=A), "must not overlap"), (dict(D=B + 8), "must not overlap"),
           (dict(E=D + 4, lde=10), "E must be NULL, D or not overlap D"), (dict(E=D, lde=12), "lde == ldd")]
  for kw, text in cases:
    assert call(**kw) < 0, kw
    msg = lib.rk_ease_last_error().decode()
    assert msg.startswith("rk_ease_gemm: ") and text in msg, (kw, msg)
  assert call(lo=5, hi=5) == 0              # (an empty range is valid and launches nothing)
  assert call(lo=5, hi=5, E=D, lde=10) == 0 and call(lo=5, hi=5, E=A, lde=10) == 0


def test_admm_update_refuses_bad_arguments_without_a_device(built):
  from recoder_amd import _ease_lib
  lib = _ease_lib.load()
  p = 4096
  good = dict(T=p, P=p, C=p, U=p, M=p, ld=10, n=10, theta=0.5, nonneg=1, gamma=p, rp=p, rd=p, rn=p, lo=0, hi=10)

  def call(**kw):
    g = dict(good, **kw)
    return lib.rk_ease_admm_update(g["T"], g["ld"], g["P"], g["ld"], g["C"], g["ld"], g["U"], g["ld"], g["M"], g["ld"],
                                   g["n"], g["theta"], g["nonneg"], g["gamma"], g["rp"], g["rd"], g["rn"], g["lo"],
                                   g["hi"], None)
  cases = [(dict(T=None), "null pointer"), (dict(M=None), "null pointer"), (dict(gamma=None), "null pointer"),
           (dict(rn=None), "null pointer"), (dict(n=0, hi=0), "bad sizes"), (dict(ld=9), "bad sizes"),
           (dict(theta=-1.0), "theta must be"), (dict(theta=float("nan")), "theta must be"),
           (dict(theta=float("inf")), "theta must be"), (dict(nonneg=2), "nonneg must be"),
           (dict(lo=-1), "bad row range"), (dict(hi=11), "bad row range"), (dict(lo=6, hi=5), "bad row range")]
  for kw, text in cases:
    assert call(**kw) < 0, kw
    msg = lib.rk_ease_last_error().decode()
    assert msg.startswith("rk_ease_admm_update: ") and text in msg, (kw, msg)
  assert call(lo=5, hi=5) == 0
