"""rk_als_foldin without a GPU: the export and its binding, the f32 restatement of tests/foldin_util.py against a
float64 solve of the same inputs within Cholesky's counted error bound, and the refusals of recoder_amd.foldin.

Measured on the cases below (relative error / bound of the row that comes closest to its bound, variant "values"):
  h = 1: 3.2e-07 / 2.3e-06    h = 3: 3.2e-07 / 1.2e-05    h = 33: 7.7e-07 / 2.0e-03    h = 64: 8.0e-07 / 1.2e-02
  h = 128: 7.9e-07 / 8.1e-02"""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from . import foldin_util as U
from .abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)


def test_library_exports_and_binds_foldin(built):
  from recoder_amd import _als_lib, foldin
  for name in ("rk_als_foldin", "rk_als_foldin_max_h"):
    assert name in exports(built.ALS_LIB)
    assert name in declared([os.path.join(INC, "recoder_als.h")])
    assert name in _als_lib.SIGNATURES
  lib = _als_lib.load()
  assert lib.rk_als_foldin.restype is _als_lib.SIGNATURES["rk_als_foldin"][0]
  assert len(_als_lib.SIGNATURES["rk_als_foldin"][1]) == 15
  assert lib.rk_als_foldin_max_h() == _als_lib.FOLDIN_MAX_H == foldin.MAX_H == U.MAX_H >= 128


def test_entry_point_refuses_bad_arguments(built):
  """h above the limit (an error, not another path), short leading dimensions, rows < 0, a negative or non-finite
  alpha and null pointers return the library's error code before any launch; rows == 0 is a success."""
  from recoder_amd import _als_lib
  from recoder_amd._lib import RecoderHipError
  lib = _als_lib.load()
  p = 4096                                               # (never dereferenced: every case is refused first)
  good = [p, p, None, 4, p, 16, 16, p, p, None, 1.0, p, 16, p, None]

  def call(**change):
    a = list(good)
    for i, v in change.items():
      a[int(i[1:])] = v
    return lib.rk_als_foldin(*a)
  assert call(_6=0) == -2 and call(_6=129, _5=129, _12=129) == -2      # h
  assert call(_5=15) == -2 and call(_12=15) == -2                      # ldy, ldx < h
  assert call(_3=-1) == -2
  for alpha in (-1.0, float("nan"), float("inf")):
    assert call(_10=alpha) == -2, alpha
  for i in (0, 1, 4, 7, 8, 11, 13):
    assert call(**{"_%d" % i: None}) == -2, i
  assert call(_3=0) == 0                                               # no rows: nothing is launched
  assert call(_3=0, _0=None, _11=None) == 0
  with pytest.raises(RecoderHipError, match="rk_als_foldin"):
    _als_lib.check(call(_6=129, _5=129, _12=129), "rk_als_foldin")


@pytest.mark.parametrize("h", U.HS)
def test_restatement_against_float64(h):
  """Every row of the batch at the first variant and three rows of each other one (empty, 5 entries, the long row):
  |x - x64| / |x64| within the counted bound.  reg = 1e-2 tr(G) / h >= 1e-3 tr(G) / h."""
  p = U.problem(h)
  csr = p["csr"]
  G64 = p["Y"].astype(np.float64).T @ p["Y"].astype(np.float64)
  assert p["reg"] >= 1e-3 * np.trace(G64) / h
  worst = (0.0, 0.0)
  for vi, (name, alpha, use_data, bias_given) in enumerate(U.VARIANTS):
    v, bias = U.variant_inputs(p, bias_given)
    X, st = U.want(h, vi)
    assert not st.any()
    for u in (range(csr.shape[0]) if vi == 0 else (0, 2, 3)):
      lo, hi = csr.indptr[u], csr.indptr[u + 1]
      cols, vals = csr.indices[lo:hi], (csr.data[lo:hi] if use_data else None)
      x64, bound = U.solve64(cols, vals, p["Y"], p["G"], v, bias, alpha)
      nrm = np.linalg.norm(x64)
      if nrm == 0:                                           # (an empty row without a bias: exactly zero)
        assert not X[u].any(), (name, u)
        continue
      err = np.linalg.norm(X[u].astype(np.float64) - x64) / nrm
      if vi == 0 and err / bound >= worst[0] / max(worst[1], 1e-300):
        worst = (err, bound)
      assert err <= bound, (name, u, hi - lo, err, bound)
  print("h = %d: worst relative error %.3g at bound %.3g" % (h, worst[0], worst[1]))


def test_restatement_edges():
  """One entry at h = 1 is a scalar equation; the empty row without a bias is exactly zero; the singular case stops at
  its second pivot with status 1."""
  f = np.float32
  Y = np.array([[0.5], [2.0]], f)
  G = np.array([[4.25 + 1.0]], f)
  x, st = U.foldin_row32([1], [3.0], Y, G, np.array([0.25], f), np.array([0.0, 0.5], f), 2.0)
  # (G + 2 * 2 * 2) x = ((1 + 2) * 3 - 2 * 0.5) * 2 - 0.25
  assert st == 0 and x[0] == f(f(15.75) / f(np.sqrt(f(13.25)))) / f(np.sqrt(f(13.25)))
  p = U.problem(33)
  x, st = U.foldin_row32([], None, p["Y"], p["G"], np.zeros(33, f), None, 10.0)
  assert st == 0 and not x.any()
  s = U.singular_problem()
  X, st = U.foldin32(s["csr"], s["Y"], s["G"], s["v"], s["bias"], 10.0)
  assert st.tolist() == [1] and X.tobytes() == np.zeros((1, 3), f).tobytes()


def test_property_seed_leaves_few_positions_undecided():
  """tests/test_foldin.py compares ``recommend_folded`` with ``recommend`` after PureSVD wherever the exact rows'
  score gaps exceed the bound, and lets at most 2 % of the positions go undecided.  In float64, with the exact
  truncated SVD of the same matrix, the chosen seed leaves 1.2 %."""
  m = U.prop_matrix()
  A = np.asarray(m.todense(), np.float64)
  V = np.linalg.svd(A, full_matrices=False)[2][:8].T
  X = A @ V
  thr = 2 * U.bound(8, np.diff(m.indptr), 1.0) * np.linalg.norm(X, axis=1) * np.linalg.norm(V, axis=1).max()
  _, sure = U.decided(X @ V.T, m, U.PROP_K, thr)
  print("undecided positions: %.2f %%" % (100 * (1 - sure.mean())))
  assert 1 - sure.mean() <= 0.015


# ------------------------------------------------------------------------------------------------------- refusals
def _no_gpu(monkeypatch):
  from recoder_amd import _als_lib, device
  import recoder_amd.model as model_mod

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(_als_lib, "load", no_gpu)


def _mf(h=4, **kw):
  from recoder_amd.nn import MatrixFactorization
  return MatrixFactorization(h, **kw)


def test_signatures():
  from recoder_amd import foldin
  from recoder_amd.model import Recoder
  from recoder_amd.recommender import FoldInRecommender
  assert list(inspect.signature(Recoder.fold_in).parameters) == ["self", "interactions_matrix", "alpha", "reg"]
  assert list(inspect.signature(Recoder.recommend_folded).parameters) == \
      ["self", "users_interactions", "num_recommendations", "alpha", "reg"]
  assert list(inspect.signature(foldin.fold_in).parameters) == ["recoder", "matrix", "alpha", "reg"]
  assert list(inspect.signature(FoldInRecommender.__init__).parameters) == \
      ["self", "model", "num_recommendations", "alpha", "reg"]
  for fn in (Recoder.fold_in, Recoder.recommend_folded, foldin.fold_in, FoldInRecommender.__init__):
    d = inspect.signature(fn).parameters
    assert (d["alpha"].default, d["reg"].default) == (foldin.DEFAULT_ALPHA, foldin.DEFAULT_REG)
  for name in ("recommend", "recommend_array", "recommend_device"):
    assert callable(getattr(FoldInRecommender, name))
  assert "user_rows" in inspect.signature(Recoder._recommend_device).parameters
  assert inspect.signature(Recoder._recommend_device).parameters["user_rows"].default is None


def test_fold_in_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd import foldin
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  m = sp.csr_matrix(np.eye(5, 12, dtype=np.float32))

  def ready(model):
    model.init_model(num_items=12, num_users=7)              # (on the host: nothing here reaches a device)
    return model
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "fold_in serves a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "fold_in serves a MatrixFactorization, not ShallowAutoencoder"),
    (ready(_mf(4, activation_type="tanh")), {}, "fold_in needs activation_type='none' \\(got 'tanh'\\)"),
    (ready(_mf(foldin.MAX_H + 1)), {}, "fold_in supports embedding sizes 1..128 \\(got 129\\)"),
    (ready(_mf(4)), {"alpha": -1.0}, "alpha must be a finite number >= 0 \\(got -1.0\\)"),
    (ready(_mf(4)), {"alpha": float("nan")}, "alpha must be a finite number >= 0"),
    (ready(_mf(4)), {"reg": -0.5}, "reg must be a finite number >= 0 \\(got -0.5\\)"),
    (ready(_mf(4)), {"reg": True}, "reg must be a finite number >= 0"),
    (_mf(4), {}, "fold_in needs an initialised model"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.fold_in(m, **kw)
    with pytest.raises(ValueError, match=message):
      foldin.fold_in(rec, m, **kw)
  rec = Recoder(model=None)
  with pytest.raises(ValueError, match="fold_in serves a MatrixFactorization, not NoneType"):
    rec.fold_in(m)
  # more than one rank
  import torch.distributed as dist
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(ValueError, match="fold_in runs on one GPU"):
    Recoder(model=ready(_mf(4))).fold_in(m)
  monkeypatch.undo()
  # more columns than the model has items (the canonical CSR is host work)
  _no_gpu(monkeypatch)
  with pytest.raises(ValueError, match="interactions_matrix has 13 columns, the model has 12 items"):
    foldin.batch_csr(sp.csr_matrix(np.eye(5, 13, dtype=np.float32)), 12, torch.device("cpu"))
  with pytest.raises(ValueError, match="rk_als_foldin takes h <= 128 \\(got 129\\)"):
    foldin.solve(None, torch.zeros(3, 129), None, None, None, 1.0)
