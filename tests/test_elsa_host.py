"""CPU: ELSA's host side (recoder_amd/elsa.py, nn.LowRankShallowAutoencoder, Recoder.train_elsa), and the Gram form the
module's docstring states against the published dense formulation in float64.  The first two tests pin the comparator
(tests/elsa_util.py) at the module's own start and constants; the kernels meet it in tests/test_elsa.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import elsa_util as eu
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)


# ------------------------------------------------------- the Gram form is exact
@pytest.mark.parametrize("B,n,h", [(1, 33, 1), (37, 33, 20), (1, 129, 20), (37, 129, 1), (37, 129, 20)])
def test_the_gram_form_equals_the_dense_formulation_in_float64(B, n, h):
  X = eu.sparse_matrix(B, n, seed=B + n + h, values=True)
  if B == 1:                                   # (a single user: keep the row, not the empty one)
    X = eu.sparse_matrix(3, n, seed=n + h, values=True)[2:3]
  else:
    assert X[1].nnz == 0 and X[:, n - 1].nnz == 0, "an empty user row and an item nobody holds"
  from recoder_amd import elsa
  W = elsa.initial_factors(n, h, 1).astype(np.float64)          # (the fit's own start)
  W[n // 2] = 0.0                              # (a zero row of W: its A is zero, its gradient is dA / 1e-12)
  loss_d, dW_d = eu.dense(X, W)
  loss_g, dW_g, parts = eu.gram(X, W)
  assert abs(loss_g - loss_d) <= 1e-12 * abs(loss_d)
  live = np.arange(n) != n // 2
  scale = np.abs(dW_d)[live].max()
  if h == 1:
    # one column: A_j = +-1 and the projection removes all of dA_j, the gradient is exactly 0 and both forms leave the
    # rounding of dA_j - <dA_j, A_j> A_j; the scale is that of the two terms of the difference, |dA_j| / |W_j|
    scale = (np.abs(parts["dA"]) / np.abs(np.where(W == 0, 1.0, W)))[live].max()
  assert np.abs(dW_g - dW_d)[live].max() <= 1e-12 * scale
  # the zero row: h = 1 excepted (torch's normalize has no gradient at 0 there either way), both are dA / 1e-12
  assert np.abs(dW_g - dW_d)[~live].max() <= 1e-12 * max(np.abs(dW_d)[~live].max(), 1e-300) + 1e-300


def test_the_header_orders_restate_the_formulas():
  from recoder_amd import elsa
  assert (eu.BETA1, eu.BETA2, eu.EPS) == (elsa.BETA1, elsa.BETA2, elsa.EPS), "the comparator's Adam is the module's"
  rng = np.random.RandomState(0)
  x, y = rng.randn(5, 200).astype(np.float32), rng.randn(5, 200).astype(np.float32)
  want = (x.astype(np.float64) * y.astype(np.float64)).sum(1)
  assert np.abs(eu.row_dot64(x, y) - want).max() <= 1e-13 * np.abs(x * y).sum(1).max()
  r = rng.rand(700)
  assert abs(eu.loss_sum(r, 700.0 * 9) - r.sum() / 6300) <= 1e-15
  A, nrm = eu.normalize_f32(np.vstack([x, np.zeros((1, 200), np.float32)]))
  assert A.dtype == np.float32 and not A[5].any() and nrm[5] == 0
  np.testing.assert_allclose((A[:5].astype(np.float64) ** 2).sum(1), 1.0, rtol=1e-6)


# ---------------------------------------------------------------- the model class
def test_package_exports_the_model():
  import recoder_amd
  from recoder_amd.nn import CsrScoresModel, LowRankShallowAutoencoder
  assert recoder_amd.LowRankShallowAutoencoder is LowRankShallowAutoencoder
  assert "LowRankShallowAutoencoder" in recoder_amd.__all__
  assert issubclass(LowRankShallowAutoencoder, CsrScoresModel)
  assert LowRankShallowAutoencoder.fit_method == "train_elsa"
  assert LowRankShallowAutoencoder().embedding_size == 256
  for bad in (0, 513, 2.0, True, "64", None):
    with pytest.raises(ValueError, match="embedding_size"):
      LowRankShallowAutoencoder(bad)


def test_model_params_round_trip_and_torch_forward():
  from recoder_amd.nn import LowRankShallowAutoencoder
  m = LowRankShallowAutoencoder(embedding_size=7)
  assert m.model_params() == {"embedding_size": 7}
  m2 = LowRankShallowAutoencoder()
  m2.load_model_params(m.model_params())
  assert m2.model_params() == {"embedding_size": 7} and isinstance(m2.embedding_size, int)
  with pytest.raises(ValueError):
    m2.load_model_params({"embedding_size": 0})
  m.init_model(num_items=5)
  assert list(m.state_dict()) == ["item_factors"] and m.item_factors.shape == (5, 7) and not bool(m.item_factors.any())
  W = eu.initial_factors(5, 7, 3)
  W[4] = 0.0
  m.item_factors.data.copy_(torch.from_numpy(W))
  m._weights_written()
  x = np.array([[1.0, 0.0, 2.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
  want = eu.scores(sp.csr_matrix(x), W)
  np.testing.assert_allclose(m(torch.from_numpy(x)).numpy(), want, rtol=0, atol=1e-6)
  got = m.torch_forward(torch.from_numpy(x[:, [0, 2]]), input_items=torch.tensor([0, 2]), target_items=torch.tensor([1, 3]))
  want2 = eu.scores(sp.csr_matrix(x * np.array([1, 0, 1, 0, 0], np.float32)), W)[:, [1, 3]]
  np.testing.assert_allclose(got.numpy(), want2, rtol=0, atol=1e-6)


# ------------------------------------------------------ what train_elsa refuses
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


def _untouched(rec):
  assert rec.model.model_params() == {"embedding_size": 8}
  assert rec.optimizer is None and rec.items is None and rec.model.item_factors is None
  assert not hasattr(rec, "elsa_history")


def test_other_models_are_refused(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=ShallowAutoencoder())
  with pytest.raises(ValueError, match="train_elsa fits a LowRankShallowAutoencoder, not ShallowAutoencoder"):
    rec.train_elsa(_dataset())
  assert rec.optimizer is None and rec.items is None
  with pytest.raises(ValueError, match="train_ease fits a ShallowAutoencoder, not LowRankShallowAutoencoder"):
    Recoder(model=LowRankShallowAutoencoder()).train_ease(_dataset())


BAD = [(dict(num_epochs=0), "num_epochs must be an integer >= 1"),
       (dict(num_epochs=2.0), "num_epochs must be an integer >= 1"),
       (dict(num_epochs=True), "num_epochs must be an integer >= 1"),
       (dict(batch_size=0), "batch_size must be an integer >= 1"),
       (dict(batch_size="x"), "batch_size must be an integer >= 1"),
       (dict(lr=0.0), "lr must be finite and > 0"),
       (dict(lr=float("nan")), "lr must be finite and > 0"),
       (dict(lr=float("inf")), "lr must be finite and > 0"),
       (dict(seed=-1), "seed must be an integer"),
       (dict(seed=1.5), "seed must be an integer"),
       (dict(seed=2 ** 32), "seed must be an integer")]


@pytest.mark.parametrize("kw,text", BAD, ids=[str(i) for i in range(len(BAD))])
def test_a_bad_argument_is_a_value_error_and_leaves_nothing_behind(monkeypatch, kw, text):
  from recoder_amd import elsa
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=LowRankShallowAutoencoder(8))
  with pytest.raises(ValueError, match=text):
    rec.train_elsa(_dataset(), **kw)
  _untouched(rec)
  with pytest.raises(ValueError, match=text):
    elsa.check_params(**dict(dict(embedding_size=8, num_epochs=1, batch_size=4, lr=0.1, seed=0), **kw))


def test_multi_gpu_is_refused_after_the_config(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=LowRankShallowAutoencoder(8))
  with pytest.raises(ValueError, match="lr must"):                     # (A before B)
    rec.train_elsa(_dataset(), lr=-1.0)
  with pytest.raises(NotImplementedError, match="train_elsa"):
    rec.train_elsa(_dataset())
  _untouched(rec)


def test_an_impossible_size_is_a_value_error_before_any_allocation(monkeypatch):
  from recoder_amd import elsa
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=LowRankShallowAutoencoder(8), num_items=2 * 10 ** 9)
  with pytest.raises(ValueError, match="n = 2000000000") as e:
    rec.train_elsa(_dataset())
  assert str(elsa.required_bytes(20, 2 * 10 ** 9, 8, 1024, 0)) in str(e.value)
  _untouched(rec)
  # a call that passes A-D gets as far as the GPU, and not further
  with pytest.raises(AssertionError, match="GPU work started"):
    Recoder(model=LowRankShallowAutoencoder(8)).train_elsa(_dataset())


def test_train_points_at_train_elsa(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=LowRankShallowAutoencoder())
  with pytest.raises(ValueError) as e:
    rec.train(_dataset())
  assert str(e.value) == LowRankShallowAutoencoder.fit_sentence % "train_elsa" and "call train_elsa(" in str(e.value)
  assert rec.optimizer is None and rec.items is None


# ------------------------------------------------------------------- memory
def test_memory_arithmetic_without_touching_a_device(monkeypatch):
  from recoder_amd import elsa
  _no_gpu(monkeypatch)
  U, n, h, B, nnz = 138493, 20108, 256, 1024, 20000263
  need = elsa.required_bytes(U, n, h, B, nnz)
  tables = 5 * n * h * 4 + n * 4                       # W, two moments, A, dA; the norms
  csrs = (U + 1 + n + 1) * 8 + 2 * nnz * 8 + U * 4 + 5 * nnz * 8
  batch = 5 * B * h * 4 + B * 8
  small = 2 * h * h * 4 + 64 * h * (h + 1) * 4
  assert need == tables + csrs + batch + small
  assert elsa.required_bytes(U, n, h, B, nnz, allocate_model=False) == need - n * h * 4
  assert elsa.required_bytes(10, n, h, B, 0) == tables + (10 + 1 + n + 1) * 8 + 40 + 5 * 10 * h * 4 + 80 + small
  assert elsa.check_memory(U, n, h, B, nnz, free_bytes=need) == need
  with pytest.raises(ValueError) as e:
    elsa.check_memory(U, n, h, B, nnz, free_bytes=need - 1)
  assert "n = 20108" in str(e.value) and str(need) in str(e.value) and str(need - 1) in str(e.value)
  # the catalogues the n x n models cannot hold: C5's million items at h = 256 is 5 GB of tables
  assert elsa.check_memory(10 ** 6, 10 ** 6, 256, B, 10 ** 8, free_bytes=float("inf")) < 12 * 2 ** 30
  with pytest.raises(ValueError, match="more than one device's memory"):
    elsa.check_memory(10, 2 * 10 ** 8, 512, B, 0, free_bytes=float("inf"))
  with pytest.raises(ValueError, match="at least one item"):
    elsa.check_memory(10, 0, 8, B, 0)


def test_the_seeded_draws_are_the_restatements():
  from recoder_amd import elsa
  assert np.array_equal(elsa.initial_factors(33, 7, 5), eu.initial_factors(33, 7, 5))
  assert elsa.initial_factors(33, 7, 5).dtype == np.float32
  assert np.array_equal(elsa.epoch_order(50, 5, 2), eu.epoch_order(50, 5, 2))
  assert not np.array_equal(elsa.epoch_order(50, 5, 2), elsa.epoch_order(50, 5, 3))
  step, isb2 = elsa.adam_scalars(0.1, 1)
  assert abs(step - 1.0) < 1e-12 and abs(isb2 - 1.0 / np.sqrt(0.001)) < 1e-9


# ---------------------------------------------------------------------- ABI
NEW = ["rk_ease_csr_sub", "rk_ease_elsa_adam", "rk_ease_elsa_normalize", "rk_ease_elsa_project", "rk_ease_elsa_rows",
       "rk_ease_elsa_scatter"]


def test_the_library_exports_the_new_functions(built):
  import os
  from recoder_amd import _ease_lib
  names = declared([os.path.join(INC, "recoder_ease.h")])
  assert set(NEW) <= set(names)
  assert exports(built.EASE_LIB) == names == sorted(_ease_lib.SIGNATURES)
  assert os.path.join(built.CSRC, "ease", "elsa.h") in built.headers_of("ease")
  for stem in ("als", "slim", "rp3"):
    assert not any("elsa" in h for h in built.headers_of(stem))


def test_the_calls_refuse_bad_arguments_without_a_device(built):
  from recoder_amd import _ease_lib
  lib = _ease_lib.load()
  err = lambda: lib.rk_ease_last_error().decode()
  p = 4096
  assert lib.rk_ease_elsa_normalize(p, 8, 4, 513, p, 8, p, None, 0, None) == -2 and "1 <= h <= 512" in err()
  assert lib.rk_ease_elsa_normalize(p, 7, 4, 8, p, 8, p, None, 0, None) == -2
  assert lib.rk_ease_elsa_normalize(p, 8, 4, 8, p, 8, p, p, 3, None) == -2 and "ldt >= n" in err()
  assert lib.rk_ease_elsa_normalize(None, 8, 4, 8, p, 8, p, None, 0, None) == -2 and "null pointer" in err()
  assert lib.rk_ease_elsa_rows(p, 8, p, 8, p, 4, 8, 0, p, 8, p, 8, p, None, None) == -2
  assert lib.rk_ease_elsa_rows(p, 8, p, 8, p, 4, 8, 9, p, 7, p, 8, p, None, None) == -2 and "lde" in err()
  assert lib.rk_ease_elsa_rows(None, 8, None, 8, None, 0, 8, 9, None, 8, None, 8, None, None, None) == 0    # (no rows)
  assert lib.rk_ease_elsa_scatter(p, p, None, 4, 3, 2, p, 8, 8, p, 8, None) == -2 and "lo <= hi" in err()
  assert lib.rk_ease_elsa_scatter(p, p, None, 4, 0, 2, None, 8, 8, p, 8, None) == -2 and "E must be given" in err()
  assert lib.rk_ease_elsa_scatter(p, p, None, 4, 0, 2, p, 8, 8, p, 7, None) == -2
  assert lib.rk_ease_elsa_project(p, 8, p, 8, p, 4, 8, p, 7, None) == -2
  assert lib.rk_ease_elsa_adam(p, 8, p, 8, p, 8, p, p, p, 4, 8, 0.9, 1.0, 1e-8, 0.1, 1.0, None) == -2 and "beta" in err()
  assert lib.rk_ease_elsa_adam(p, 8, p, 8, p, 8, p, p, None, 4, 8, 0.9, 0.999, 1e-8, 0.1, 1.0, None) == -2
  assert lib.rk_ease_csr_sub(p, p, None, 4, 5, 3, p, 8, None) == -2
  assert lib.rk_ease_csr_sub(p, p, None, 4, 0, 9, p, 8, None) == -2 and "ldo" in err()
  assert lib.rk_ease_csr_sub(None, None, None, 0, 0, 9, None, 9, None) == 0                               # (no rows)
