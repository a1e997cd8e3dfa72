"""CPU: ShallowAutoencoder's torch forward, its model_params, what train_ease and the memory check
refuse before any GPU work, and the float64 restatement's own pins (tests/ease_util.py)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import als_util, ease_util


def _model(B):
  from recoder_amd.nn import ShallowAutoencoder
  m = ShallowAutoencoder(reg=7.0)
  m.init_model(num_items=B.shape[0])
  assert m.item_weights.shape == B.shape and not bool(m.item_weights.any())      # zero until fitted
  m.item_weights.data.copy_(torch.from_numpy(B))
  return m


def test_package_exports_the_model():
  import recoder_amd
  from recoder_amd.nn import FactorizationModel, ShallowAutoencoder
  assert recoder_amd.ShallowAutoencoder is ShallowAutoencoder
  assert issubclass(ShallowAutoencoder, FactorizationModel)
  assert ShallowAutoencoder().reg == 500.0
  with pytest.raises(ValueError):
    ShallowAutoencoder(reg=0.0)


@pytest.mark.parametrize("subset", ["all", "input", "target", "both"])
def test_torch_forward_matches_the_float64_scores(subset):
  X = als_util.random_csr(40, 37, 0.15, seed=3, values="counts", empty_rows=(5,))
  B64, _ = ease_util.fit(X, 7.0)
  m = _model(B64.astype(np.float32))
  rng = np.random.RandomState(1)
  ii = np.sort(rng.choice(37, 20, replace=False)) if subset in ("input", "both") else None
  tt = rng.choice(37, 11, replace=False) if subset in ("target", "both") else None
  dense = np.asarray(X.todense(), np.float32)
  x = dense if ii is None else dense[:, ii]
  got = m.torch_forward(torch.from_numpy(x), input_items=None if ii is None else torch.from_numpy(ii),
                        target_items=None if tt is None else torch.from_numpy(tt)).numpy()
  assert torch.equal(m(torch.from_numpy(x), input_items=None if ii is None else torch.from_numpy(ii),
                       target_items=None if tt is None else torch.from_numpy(tt)), torch.from_numpy(got))
  Xs = X if ii is None else X[:, ii]
  want = ease_util.scores(Xs, B64 if ii is None else B64[ii])
  want = want if tt is None else want[:, tt]
  bound = 40 * 2.0 ** -23 * (np.abs(x).astype(np.float64) @ np.abs(B64 if ii is None else B64[ii])).max()
  assert np.abs(got - want).max() <= bound


def test_model_params_round_trip():
  from recoder_amd.nn import ShallowAutoencoder
  m = ShallowAutoencoder(reg=123.5)
  assert m.model_params() == {"reg": 123.5}
  m2 = ShallowAutoencoder()
  m2.load_model_params(m.model_params())
  assert m2.reg == 123.5 and m2.model_params() == m.model_params()
  with pytest.raises(ValueError):
    m2.load_model_params({"reg": -1.0})


def _no_gpu(monkeypatch):
  import recoder_amd.als  # noqa: F401
  import recoder_amd.ease  # noqa: F401
  import recoder_amd.model as model_mod
  from recoder_amd import device

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)


def _dataset(n=5):
  import scipy.sparse as sp
  from recoder_amd.data import RecommendationDataset
  return RecommendationDataset(sp.csr_matrix(np.eye(n, dtype=np.float32)))


def test_train_ease_rejects_other_models_before_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, MatrixFactorization
  _no_gpu(monkeypatch)
  for model in (MatrixFactorization(16), DynamicAutoencoder(hidden_layers=[16])):
    with pytest.raises(ValueError, match="ShallowAutoencoder"):
      Recoder(model=model).train_ease(_dataset())


def test_train_ease_rejects_a_bad_reg_before_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  _no_gpu(monkeypatch)
  for reg in (0.0, -3.0, float("nan"), float("inf")):
    rec = Recoder(model=ShallowAutoencoder(50.0))
    with pytest.raises(ValueError, match="reg"):
      rec.train_ease(_dataset(), reg=reg)
    assert rec.model.reg == 50.0 and rec.model.item_weights is None


def test_train_points_at_train_ease(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  _no_gpu(monkeypatch)
  with pytest.raises(ValueError, match="train_ease"):
    Recoder(model=ShallowAutoencoder()).train(_dataset())


def test_train_ease_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError, match="train_ease"):
    Recoder(model=ShallowAutoencoder()).train_ease(_dataset())


def test_memory_check_raises_without_touching_a_device(monkeypatch):
  from recoder_amd import ease
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  _no_gpu(monkeypatch)
  with pytest.raises(ValueError) as e:
    ease.check_memory(1000000)
  assert "1000000" in str(e.value) and str(ease.required_bytes(1000000)) in str(e.value)
  assert ease.required_bytes(1000000) > 4 * 10 ** 12
  # against a stated amount of free memory: ML-20M's 1.6 GB matrix and the inverse's carries of the same
  # size do not fit in 2 GB, fit in 4 GB
  need = ease.required_bytes(20108)
  assert 2 * 20108 * 20108 * 4 < need < 2 * 20108 * 20108 * 4 + 2 ** 24
  with pytest.raises(ValueError) as e:
    ease.check_memory(20108, free_bytes=2 ** 31)
  assert "20108" in str(e.value) and str(need) in str(e.value)
  assert ease.check_memory(20108, free_bytes=2 ** 32) == need
  assert ease.check_memory(20108, free_bytes=2 ** 31, allocate_matrix=False) == need - 20108 * 20108 * 4
  # the public entry point: a 1 M-item catalogue gets the ValueError, not an allocation
  rec = Recoder(model=ShallowAutoencoder(), num_items=1000000)
  with pytest.raises(ValueError, match="1000000"):
    rec.train_ease(_dataset())
  assert rec.model.item_weights is None


# ------------------------------------------------------- the restatement's own pins
def test_restatement_solves_the_constrained_least_squares():
  """B minimises |X - X B|^2 + reg |B|^2 subject to diag(B) = 0: zero gradient off the diagonal."""
  X = als_util.random_csr(60, 23, 0.2, seed=7, values="counts")
  B, P = ease_util.fit(X, 3.0)
  assert np.all(np.diag(B) == 0)
  G = ease_util.gram(X, 0.0)
  grad = G @ B - G + 3.0 * B
  off = ~np.eye(23, dtype=bool)
  assert np.abs(grad[off]).max() <= 1e-9 * np.abs(G).max()
  assert ease_util.residual(ease_util.gram(X, 3.0), P) <= 1e-12
  np.testing.assert_array_equal(ease_util.finalize_f32(P.astype(np.float32)).diagonal(), np.zeros(23, np.float32))


def test_host_fmaf_is_an_exact_fma():
  rng = np.random.RandomState(0)
  a, b, c = (rng.randn(3000).astype(np.float32) for _ in range(3))
  # sums that land on an f32 rounding midpoint in float64 while the true sum does not
  a = np.concatenate([a, np.float32([2.0 ** -12, 2.0 ** -12 * (1 + 2.0 ** -20), -(2.0 ** -12)])])
  b = np.concatenate([b, np.float32([2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12, 2.0 ** -12 * (1 + 2.0 ** -23)])])
  c = np.concatenate([c, np.float32([1, 1, 1])])
  got = ease_util.fmaf(a, b, c)
  assert got.dtype == np.float32
  for x, y, z, g in zip(a, b, c, got):
    t = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
    d = abs(t - Fraction(float(g)))
    for nb in (np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))):
      dn = abs(t - Fraction(float(nb)))
      assert d < dn or (d == dn and not (g.view(np.uint32) & 1))
  assert got[-3] == np.float32(1 + 2.0 ** -23) and got[-1] == np.float32(1 - 2.0 ** -24)


def test_host_score_chain_agrees_with_float64():
  X = als_util.random_csr(9, 31, 0.3, seed=2, values="counts", empty_rows=(4,))
  W = np.random.RandomState(3).randn(31, 31).astype(np.float32)
  got = ease_util.scores_chain_f32(X, W)
  want = ease_util.scores(X, W)
  assert np.all(got[4] == 0)
  assert np.abs(got - want).max() <= 31 * 2.0 ** -23 * (np.abs(X).astype(np.float64) @ np.abs(W)).max()
  np.testing.assert_array_equal(ease_util.scores_chain_f32(X, W, 5, 20), got[:, 5:20])
