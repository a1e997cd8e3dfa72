"""CPU: the built library's rk_als_lgcn_* names, the pins of the numpy restatement (tests/lightgcn_util.py) --
its gradient against finite differences, its propagation against the dense normalised adjacency, its Adam
against torch.optim.Adam -- the memory arithmetic, and what train_lightgcn refuses before any GPU work."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util, lightgcn_util as lg
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_lgcn_adam", "rk_als_lgcn_propagate", "rk_als_lgcn_scatter"]


# ------------------------------------------------------------------ library
def test_the_library_exports_and_binds_the_three_kernels(built):
  from recoder_amd import _als_lib, lightgcn
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_lgcn_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert all(name in declared([header]) for name in NEW)
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)
  long_row = re.search(r"^#define RK_ALS_LGCN_LONG_ROW (\d+)$", open(header).read(), flags=re.M)
  assert long_row and int(long_row.group(1)) == _als_lib.LGCN_LONG_ROW == lightgcn.LONG_ROW


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()
  assert lib.rk_als_lgcn_propagate(p, p, p, p, 0, 4, p, 4, 8, p, 8, None, 0, 1.0, None) == -2 and "ldf >= h" in err()
  assert lib.rk_als_lgcn_propagate(p, p, p, p, 3, 2, p, 8, 8, p, 8, None, 0, 1.0, None) == -2 and "row_lo" in err()
  assert lib.rk_als_lgcn_propagate(p, p, p, p, 0, 4, p, 8, 8, None, 0, None, 0, 1.0, None) == -2 and "Out / Acc" in err()
  assert lib.rk_als_lgcn_propagate(p, p, p, p, 0, 4, p, 8, 8, p, 8, p, 4, 1.0, None) == -2 and "lda >= h" in err()
  assert lib.rk_als_lgcn_propagate(p, p, p, p, 0, 4, p, 600, 513, p, 600, None, 0, 1.0, None) == -2
  assert lib.rk_als_lgcn_propagate(p, None, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, None) == -2 and "null pointer" in err()
  assert lib.rk_als_lgcn_propagate(None, None, None, None, 4, 4, None, 8, 8, p, 8, None, 0, 1.0, None) == 0   # (no rows)
  assert lib.rk_als_lgcn_scatter(p, p, 8, 3, p, p, 8, 0.1, 5, p, 8, p, None) == -2 and "roles" in err()
  assert lib.rk_als_lgcn_scatter(p, p, 7, 2, p, p, 8, 0.1, 5, p, 8, p, None) == -2 and "roles * T" in err()
  assert lib.rk_als_lgcn_scatter(p, p, 8, 1, p, p, 8, 0.1, 5, p, 4, p, None) == -2 and "ldg >= h" in err()
  assert lib.rk_als_lgcn_scatter(p, p, 8, 1, p, p, 8, 0.1, 5, p, 8, None, None) == -2 and "null pointer" in err()
  assert lib.rk_als_lgcn_adam(p, 4, p, 8, p, 0.0, p, p, 5, 8, 0.1, 0.9, 0.999, 1e-8, 1, None) == -2 and "lde >= h" in err()
  assert lib.rk_als_lgcn_adam(p, 8, p, 8, p, 0.0, p, p, 5, 8, 0.1, 0.9, 0.999, 1e-8, 0, None) == -2 and "t >= 1" in err()
  assert lib.rk_als_lgcn_adam(p, 8, p, 8, p, 0.0, p, p, 5, 8, 0.1, 1.0, 0.999, 1e-8, 1, None) == -2 and "beta1" in err()
  assert lib.rk_als_lgcn_adam(p, 8, p, 8, None, 0.0, p, p, 5, 8, 0.1, 0.9, 0.999, 1e-8, 1, None) == -2


# -------------------------------------------------------------- restatement
def _small():
  """9 users x 7 items: user 4 holds nothing, item 6 is held by nobody, user 0 holds all the others."""
  rng = np.random.RandomState(3)
  m = (rng.rand(9, 7) < 0.4).astype(np.float32)
  m[4, :] = 0
  m[0, :] = 1
  m[:, 6] = 0
  m[1, 2] = 1
  m = sp.csr_matrix(m)
  m.sort_indices()
  return m


def test_the_restated_gradient_equals_finite_differences_of_its_own_loss():
  m, h, K, reg = _small(), 3, 2, 0.3
  rng = np.random.RandomState(0)
  Eu, Ei = rng.randn(9, h), rng.randn(7, h)
  users, pos, neg = bpr_util.sample(m, 1, 0, 40)
  neg[5] = -1                                                  # (an invalid slot adds nothing, but counts in T)
  assert (neg >= 0).sum() > 20
  gu, gi = lg.gradient(m, Eu, Ei, K, users, pos, neg, reg)[:2]
  eps = 1e-6
  for E, got in ((Eu, gu), (Ei, gi)):
    fd = np.zeros_like(E)
    for idx in np.ndindex(*E.shape):
      old = E[idx]
      E[idx] = old + eps
      up = lg.loss(m, Eu, Ei, K, users, pos, neg, reg)
      E[idx] = old - eps
      down = lg.loss(m, Eu, Ei, K, users, pos, neg, reg)
      E[idx] = old
      fd[idx] = (up - down) / (2 * eps)
    assert np.abs(got).max() > 1e-3
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(fd).max()


def test_the_restated_propagation_is_the_dense_normalised_adjacency():
  m, h, K = _small(), 3, 2
  rng = np.random.RandomState(1)
  Eu, Ei = rng.randn(9, h), rng.randn(7, h)
  A = lg.adjacency(m)
  assert np.array_equal(A, A.T) and not A[4].any() and not A[9 + 6].any()
  E = np.concatenate([Eu, Ei])
  su, si = lg.scales(m)
  one, _ = lg.propagate(m, su, si, Ei)
  np.testing.assert_allclose(one, (A @ E)[:9], rtol=1e-13, atol=1e-15)
  two, _ = lg.propagate(lg.transpose(m), si, su, Eu)
  np.testing.assert_allclose(two, (A @ E)[9:], rtol=1e-13, atol=1e-15)
  want = (E + A @ E + A @ A @ E) / (K + 1)
  P, Q = lg.forward(m, Eu, Ei, K)
  np.testing.assert_allclose(np.concatenate([P, Q]), want, rtol=1e-13, atol=1e-15)
  # the float32 form in the kernels' order stays within f32 rounding of it
  P32, Q32 = lg.forward(m, Eu.astype(np.float32), Ei.astype(np.float32), K, np.float32)
  assert P32.dtype == np.float32 and np.abs(np.concatenate([P32, Q32]) - want).max() < 1e-5
  # degree^-1/2 in float64, rounded once
  assert su[0] == np.float32(6 ** -0.5) and su[4] == 0 and si[6] == 0


def test_the_restated_adam_is_torch_adam_in_float64():
  rng = np.random.RandomState(2)
  e0 = rng.randn(6, 4)
  p = torch.nn.Parameter(torch.tensor(e0))
  opt = torch.optim.Adam([p], lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
  e, m, v = e0.copy(), np.zeros_like(e0), np.zeros_like(e0)
  count = np.array([0, 1, 2, 0, 5, 40])
  for t in (1, 2, 3):
    H = rng.randn(6, 4)
    H[3] = 0                                                  # (a zero gradient still decays the moments)
    p.grad = torch.tensor(H + 0.01 * count[:, None] * p.detach().numpy())
    opt.step()
    e, m, v = lg.adam(e, H, count, 0.01, m, v, 0.05, t)
    np.testing.assert_allclose(e, p.detach().numpy(), rtol=1e-12, atol=1e-14)
  st = opt.state[p]
  np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-16)
  np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-16)
  e32, m32, v32 = lg.adam(e0.astype(np.float32), H.astype(np.float32), count, 0.01, np.zeros((6, 4), np.float32),
                          np.zeros((6, 4), np.float32), 0.05, 1, np.float32)
  e64 = lg.adam(e0.astype(np.float32), H.astype(np.float32), count, 0.01, np.zeros((6, 4)), np.zeros((6, 4)), 0.05, 1)[0]
  assert e32.dtype == np.float32 and np.abs(e32 - e64).max() < 1e-5


# ------------------------------------------------------------------ memory
def test_required_bytes_grows_with_each_argument_and_check_memory_names_the_sizes():
  from recoder_amd import bpr, lightgcn
  from recoder_amd.device import DEVICE_HBM_BYTES
  base = (1000, 500, 64, 20000, 256)
  need = lightgcn.required_bytes(*base)
  rows = 1500
  assert need == rows * 64 * 4 + 500 * 4 + 7 * rows * 64 * 4 + 2 * rows * 4 + bpr.workspace_bytes(256, 64) + \
      6 * 256 * 16 + 1001 * 8 + 501 * 8 + 2 * 20000 * 4
  for k in range(5):
    more = list(base)
    more[k] += 1
    assert lightgcn.required_bytes(*more) > need, k
  assert lightgcn.required_bytes(*base, allocate_model=False) == need - (rows * 64 * 4 + 500 * 4)
  assert lightgcn.required_bytes(*base, allocate_state=False) == need - 3 * rows * 64 * 4
  assert lightgcn.required_bytes(*base, allocate_csrs=False) == need - (1001 * 8 + 501 * 8 + 2 * 20000 * 4)
  # a continued fit holds its state and its CSRs already: the check against what is free leaves them out
  held = lightgcn.required_bytes(*base, allocate_model=False, allocate_state=False, allocate_csrs=False)
  assert lightgcn.check_memory(*base, free_bytes=held, allocate_model=False, allocate_state=False,
                               allocate_csrs=False) == held
  assert lightgcn.check_memory(*base, free_bytes=1 << 30) == need
  with pytest.raises(ValueError, match="LightGCN needs 1 <= batch_size <= 16777216 and 1 <= h <= 512 \\(got 0, 64\\)"):
    lightgcn.check_memory(10, 10, 64, 10, 0, free_bytes=1 << 30)
  users = DEVICE_HBM_BYTES // (512 * 4 * 8)
  with pytest.raises(ValueError, match="LightGCN over %d users x 1000 items at h = 512 with 5 entries and batches "
                                       "of 256 needs \\d+ bytes: more than one device's memory" % users):
    lightgcn.check_memory(users, 1000, 512, 5, 256, free_bytes=float("inf"))
  with pytest.raises(ValueError, match="LightGCN over 1000 users x 500 items at h = 64 with 20000 entries and "
                                       "batches of 256 needs %d bytes of device memory, 1000 are free" % need):
    lightgcn.check_memory(*base, free_bytes=1000)


def test_check_data_speaks_of_train_lightgcn():
  from recoder_amd import lightgcn
  assert lightgcn.check_data(1000, 10, 5, 256) == 4
  with pytest.raises(ValueError, match="train_lightgcn needs at least one stored entry"):
    lightgcn.check_data(0, 10, 1, 256)
  with pytest.raises(ValueError, match="train_lightgcn draws a stored entry with 32-bit arithmetic"):
    lightgcn.check_data(2 ** 31, 10, 1, 256)


# ------------------------------------------------------------------ refusals
def _no_gpu(monkeypatch):
  import recoder_amd.lightgcn  # noqa: F401
  import recoder_amd.model as model_mod
  from recoder_amd import device

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)


def _dataset(n=40):
  from recoder_amd.data import RecommendationDataset
  return RecommendationDataset(sp.csr_matrix(np.eye(n, dtype=np.float32)))


def _mf(h=4, **kw):
  from recoder_amd.nn import MatrixFactorization
  return MatrixFactorization(h, **kw)


def _uninitialised(rec):
  return not rec._Recoder__model_initialized and rec.lightgcn_state is None and rec.lightgcn_history == [] and \
      rec.optimizer is None


def test_check_config_accepts_the_contract():
  from recoder_amd import lightgcn
  assert lightgcn.check_config(_mf(4), 2, 3, 256, 0.01, 1e-4, 0) == (2, 3, 256, 0.01, 1e-4, 0)
  assert lightgcn.check_config(_mf(512), np.int64(8), 0, 1, np.float32(0.5), 0, -7) == (8, 0, 1, 0.5, 0.0, -7)


def test_train_lightgcn_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_lightgcn trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_lightgcn trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_lightgcn needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_lightgcn needs dropout_prob == 0"),
    (_mf(0), {}, "train_lightgcn supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_lightgcn supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"num_layers": 0}, "num_layers must be an integer in 1..8 \\(got 0\\)"),
    (_mf(4), {"num_layers": 9}, "num_layers must be an integer in 1..8 \\(got 9\\)"),
    (_mf(4), {"num_layers": True}, "num_layers must be an integer in 1..8"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"lr": -0.1}, "lr must be finite and > 0"),
    (_mf(4), {"lr": float("nan")}, "lr must be finite and > 0"),
    (_mf(4), {"lr": float("inf")}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..16777216 \\(got 0\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"seed": 2 ** 63}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_lightgcn"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.train_lightgcn(_dataset(), **kw)
    assert _uninitialised(rec), message
  from recoder_amd import lightgcn
  state = {"num_layers": 2, "E0": (torch.zeros(40, 4), torch.zeros(40, 4))}
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 3\\)"):
    lightgcn.check_resume(state, 3)
  with pytest.raises(ValueError, match="do not match the model's"):
    lightgcn.check_resume(state, 2, ((40, 4), (41, 4)))
  lightgcn.check_resume(state, 2, ((40, 4), (40, 4)))


def test_train_lightgcn_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(NotImplementedError, match="train_lightgcn runs on one GPU"):
    rec.train_lightgcn(_dataset())
  assert _uninitialised(rec)
