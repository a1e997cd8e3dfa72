"""CPU: what train_bpr, bpr.check_config, bpr.check_data and bpr.check_memory refuse before any GPU work,
the workspace arithmetic, the built library's new names and argument checks, and the numpy restatement's
own pins (tests/bpr_util.py): the sampler's contract and one step against a literal per-triple sum."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util
from tests.abi_util import built, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_bpr_apply", "rk_als_bpr_grad", "rk_als_bpr_sample", "rk_als_bpr_workspace_bytes"]


def _no_gpu(monkeypatch):
  import recoder_amd.bpr  # noqa: F401
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


# ------------------------------------------------------------------ refusals
def test_check_config_accepts_the_contract():
  from recoder_amd import bpr
  assert bpr.check_config(_mf(4), 3, 256, 0.05, 0.01, 0) == (3, 256, 0.05, 0.01, 0)
  assert bpr.check_config(_mf(512), np.int64(0), np.int64(1), np.float32(0.5), 0, -7) == (0, 1, 0.5, 0.0, -7)
  assert bpr.check_config(_mf(1), 1, bpr.MAX_BATCH, 1, 0.0, 2 ** 63 - 1)[1] == 1 << 24


def test_check_config_rejects_each_bad_argument():
  from recoder_amd import bpr
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  ok = (3, 256, 0.05, 0.01, 0)
  for model in (DynamicAutoencoder(hidden_layers=[8]), ShallowAutoencoder()):
    with pytest.raises(ValueError, match="train_bpr trains a MatrixFactorization, not "):
      bpr.check_config(model, *ok)
  with pytest.raises(ValueError, match="train_bpr needs activation_type='none' \\(got 'tanh'\\)"):
    bpr.check_config(_mf(4, activation_type="tanh"), *ok)
  with pytest.raises(ValueError, match="train_bpr needs dropout_prob == 0"):
    bpr.check_config(_mf(4, dropout_prob=0.5), *ok)
  for h in (0, -1, 2.0, 513):
    with pytest.raises(ValueError, match="train_bpr supports embedding sizes 1..512"):
      bpr.check_config(_mf(h), *ok)
  for v in (-1, 1.5, None, True):
    with pytest.raises(ValueError, match="num_epochs must be an integer >= 0"):
      bpr.check_config(_mf(4), v, 256, 0.05, 0.01, 0)
  for v in (0, -4, 2.0, None, True, (1 << 24) + 1):
    with pytest.raises(ValueError, match="batch_size must be an integer in 1..16777216"):
      bpr.check_config(_mf(4), 3, v, 0.05, 0.01, 0)
  for v in (0, 0.0, -0.1, float("nan"), float("inf"), None, True, "0.1"):
    with pytest.raises(ValueError, match="lr must be finite and > 0"):
      bpr.check_config(_mf(4), 3, 256, v, 0.01, 0)
  for v in (-1e-9, float("nan"), float("inf"), None, False):
    with pytest.raises(ValueError, match="reg must be finite and >= 0"):
      bpr.check_config(_mf(4), 3, 256, 0.05, v, 0)
  for v in (0.5, None, True, 2 ** 63, -2 ** 63 - 1):
    with pytest.raises(ValueError, match="seed must be an integer that fits 64 bits"):
      bpr.check_config(_mf(4), 3, 256, 0.05, 0.01, v)


def test_check_data_rejects_what_the_sampler_cannot_draw():
  from recoder_amd import bpr
  assert bpr.check_data(1000, 10, 5, 256) == 4 and bpr.steps_per_epoch(1024, 256) == 4
  assert bpr.check_data(2 ** 31 - 1, 10, 1, 1 << 24) == 128
  for nnz in (2 ** 31, 2 ** 40):
    with pytest.raises(ValueError, match="nnz must be below 2\\^31 \\(got %d\\)" % nnz):
      bpr.check_data(nnz, 10, 1, 256)
  with pytest.raises(ValueError, match="at least one stored entry"):
    bpr.check_data(0, 10, 1, 256)
  with pytest.raises(ValueError, match="num_epochs \\* ceil\\(nnz / batch_size\\) must be below 2\\^31"):
    bpr.check_data(2 ** 30, 10, 4, 1)


def test_check_memory_names_the_sizes():
  from recoder_amd import bpr
  from recoder_amd.device import DEVICE_HBM_BYTES
  need = bpr.check_memory(1000, 500, 64, 20000, 256, free_bytes=1 << 30)
  assert need == (1000 + 500) * 64 * 4 + 500 * 4 + 1001 * 8 + 20000 * 4 + bpr.workspace_bytes(256, 64) + 6 * 256 * 16
  assert bpr.check_memory(1000, 500, 64, 20000, 256, free_bytes=1 << 30, allocate_model=False) == \
      need - ((1000 + 500) * 64 * 4 + 500 * 4)
  with pytest.raises(ValueError, match="BPR needs 1 <= batch_size <= 16777216 and 1 <= h <= 512 \\(got 0, 64\\)"):
    bpr.check_memory(10, 10, 64, 10, 0, free_bytes=1 << 30)
  with pytest.raises(ValueError, match="got 256, 513"):
    bpr.check_memory(10, 10, 513, 10, 256, free_bytes=1 << 30)
  users = DEVICE_HBM_BYTES // (512 * 4)
  with pytest.raises(ValueError, match="BPR over %d users x 1000 items at h = 512 with 5 entries and batches of 256 "
                                       "needs \\d+ bytes: more than one device's memory" % users):
    bpr.check_memory(users, 1000, 512, 5, 256, free_bytes=float("inf"))
  with pytest.raises(ValueError, match="needs %d bytes of device memory, 1000 are free" % need):
    bpr.check_memory(1000, 500, 64, 20000, 256, free_bytes=1000)


def test_train_bpr_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder
  _no_gpu(monkeypatch)
  with pytest.raises(ValueError, match="MatrixFactorization"):
    Recoder(model=DynamicAutoencoder(hidden_layers=[8])).train_bpr(_dataset())
  with pytest.raises(ValueError, match="activation_type"):
    Recoder(model=_mf(4, activation_type="relu")).train_bpr(_dataset())
  with pytest.raises(ValueError, match="embedding sizes"):
    Recoder(model=_mf(600)).train_bpr(_dataset())
  with pytest.raises(ValueError, match="lr must be"):
    Recoder(model=_mf(4)).train_bpr(_dataset(), lr=0)


def test_train_bpr_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError, match="train_bpr runs on one GPU"):
    Recoder(model=_mf(4)).train_bpr(_dataset())


# ------------------------------------------------------- workspace, library
def _want_workspace(T, h):
  r = lambda x: (x + 255) // 256 * 256
  return 5 * r(4 * T) + 2 * r(4 * T * h)


def test_workspace_bytes_restates_the_library(built):
  from recoder_amd import _als_lib, bpr
  lib = _als_lib.load()
  assert bpr.workspace_bytes(1, 1) == 7 * 256
  assert bpr.workspace_bytes(257, 65) == 5 * 1280 + 2 * 67072      # (4 * 257 * 65 = 66820)
  for T in (1, 63, 64, 257, 4096, 1 << 24):
    for h in (1, 7, 64, 65, 512):
      assert bpr.workspace_bytes(T, h) == lib.rk_als_bpr_workspace_bytes(T, h) == _want_workspace(T, h), (T, h)
  for T, h in ((0, 8), (-1, 8), ((1 << 24) + 1, 8), (8, 0), (8, 513)):
    assert bpr.workspace_bytes(T, h) == lib.rk_als_bpr_workspace_bytes(T, h) == -2


def test_the_library_exports_and_binds_the_new_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_bpr_")] == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  """Every refusal returns -2 with the function's name in the message; none of them reaches a launch."""
  from recoder_amd import _als_lib
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()
  assert lib.rk_als_bpr_sample(p, p, 5, 5, 2 ** 31, 0, 0, 8, p, p, p, None) == -2 and "nnz < 2^31" in err()
  assert lib.rk_als_bpr_sample(p, p, 5, 5, 0, 0, 0, 8, p, p, p, None) == -2 and "rk_als_bpr_sample" in err()
  assert lib.rk_als_bpr_sample(p, p, 5, 5, 9, 0, -1, 8, p, p, p, None) == -2 and "step >= 0" in err()
  assert lib.rk_als_bpr_sample(p, p, 5, 5, 9, 0, 0, 8, p, None, p, None) == -2 and "null pointer" in err()
  assert lib.rk_als_bpr_grad(p, p, p, 8, 5, 5, p, 4, p, 8, p, 8, p, p, None, p, p, None) == -2 and "ldx >= h" in err()
  assert lib.rk_als_bpr_grad(p, p, p, 8, 5, 5, p, 600, p, 600, p, 513, p, p, None, p, p, None) == -2
  assert lib.rk_als_bpr_grad(p, p, p, 8, 5, 5, p, 8, p, 8, None, 8, p, p, None, p, p, None) == -2 and "null pointer" in err()
  assert lib.rk_als_bpr_apply(p, p, 8, 3, p, p, 8, 0.1, 0.0, 5, p, 8, None, None) == -2 and "roles" in err()
  assert lib.rk_als_bpr_apply(p, p, 7, 2, p, p, 8, 0.1, 0.0, 5, p, 8, None, None) == -2 and "roles * T" in err()
  assert lib.rk_als_bpr_apply(p, p, 8, 1, p, p, 8, 0.1, 0.0, 5, p, 4, None, None) == -2 and "ldt >= h" in err()
  assert lib.rk_als_bpr_apply(p, p, 8, 1, p, p, 8, 0.1, 0.0, 0, p, 8, None, None) == -2 and "n_rows" in err()


# ------------------------------------------------------------------ sampler
_matrix = bpr_util.edge_matrix


def test_mix_is_splitmix64():
  """The first outputs of splitmix64 from state 0 (Vigna's reference implementation)."""
  got = bpr_util.mix(np.array([0, 0x9E3779B97F4A7C15], dtype=np.uint64))
  assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


def test_sampler_draws_stored_positives_and_unseen_negatives():
  m = _matrix()
  dense = m.toarray() > 0
  seen_full = seen_nearly = 0
  for step in range(6):
    users, pos, neg = bpr_util.sample(m, 5, step, 257)
    assert users.dtype == pos.dtype == neg.dtype == np.int32
    assert dense[users, pos].all() and not (users == 7).any()
    ok = neg >= 0
    assert not dense[users[ok], neg[ok]].any() and (neg[ok] < 53).all()
    assert (neg[users == 5] == -1).all() and set(users[~ok]) <= {3, 5}       # (3: 32 draws can all miss item 17)
    assert (neg[(users == 3) & ok] == 17).all()
    seen_full += int((users == 5).sum())
    seen_nearly += int(((users == 3) & ok).sum())
  assert seen_full > 50 and seen_nearly > 10
  # about one entry in nnz per slot: every stored entry's share of the draws is near 1 / nnz
  users, pos, _ = bpr_util.sample(m, 1, 0, 200000)
  share = np.bincount(users, minlength=37) / 200000.0
  want = np.diff(m.indptr) / m.nnz
  assert np.abs(share - want).max() < 0.005


def test_sampler_is_a_pure_function_of_seed_step_and_slot():
  m = _matrix()
  a = bpr_util.sample(m, 9, 4, 300)
  b = bpr_util.sample(m, 9, 4, 300)
  short = bpr_util.sample(m, 9, 4, 120)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  assert all(np.array_equal(x[:120], y) for x, y in zip(a, short))          # (a slot does not depend on T)
  assert not np.array_equal(a[0], bpr_util.sample(m, 9, 5, 300)[0])
  assert not np.array_equal(a[0], bpr_util.sample(m, 10, 4, 300)[0])
  assert not np.array_equal(bpr_util.sample(m, -1, 0, 300)[0], bpr_util.sample(m, 2 ** 63 - 1, 0, 300)[0])


def test_sampler_gives_up_on_a_user_who_holds_everything():
  m = sp.csr_matrix(np.ones((4, 9), np.float32))
  users, pos, neg = bpr_util.sample(m, 0, 0, 64)
  assert (neg == -1).all() and (pos >= 0).all() and set(users) <= {0, 1, 2, 3}
  X, Y, b = bpr_util.init_tables(4, 9, 5, 0)
  X1, Y1, b1, loss, count = bpr_util.step(users, pos, neg, X, Y, b, 0.1, 0.1)
  assert count == 0 and loss == 0 and np.array_equal(X1, X) and np.array_equal(Y1, Y) and np.array_equal(b1, b)


# --------------------------------------------------------------------- step
def test_one_step_is_the_literal_sum_of_the_triples_gradients():
  m = _matrix()
  rng = np.random.RandomState(2)
  X, Y = rng.randn(37, 6), rng.randn(53, 6)
  b = rng.randn(53)
  users, pos, neg = bpr_util.sample(m, 3, 1, 257)
  assert (neg < 0).any() and (neg >= 0).sum() > 150
  X1, Y1, b1, loss, count = bpr_util.step(users, pos, neg, X, Y, b, 0.05, 0.02)
  Xl, Yl, bl = bpr_util.step_literal(users, pos, neg, X, Y, b, 0.05, 0.02)
  for got, want in ((X1, Xl), (Y1, Yl), (b1, bl)):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
  assert count == int((neg >= 0).sum())
  ok = neg >= 0
  x = (X[users[ok]] * (Y[pos[ok]] - Y[neg[ok]])).sum(1) + b[pos[ok]] - b[neg[ok]]
  assert abs(loss - np.log1p(np.exp(-x)).sum()) <= 1e-10 * loss
  untouched_u = np.setdiff1d(np.arange(37), users[ok])
  untouched_i = np.setdiff1d(np.arange(53), np.concatenate([pos[ok], neg[ok]]))
  assert len(untouched_u) and np.array_equal(X1[untouched_u], X[untouched_u])
  assert np.array_equal(Y1[untouched_i], Y[untouched_i]) and np.array_equal(b1[untouched_i], b[untouched_i])


def test_the_restated_fit_lowers_its_loss_on_a_planted_matrix():
  tr, ho = bpr_util.planted()
  X, Y, b = bpr_util.init_tables(200, 120, 16, 1)
  before = bpr_util.auc(X, Y, b, tr, ho)
  X, Y, b, hist = bpr_util.fit(tr, X, Y, b, 5, 256, 0.05, 0.01, seed=0)
  assert len(hist) == 5 and all(v < hist[0] for v in hist[1:])
  assert bpr_util.auc(X, Y, b, tr, ho) > max(before, 0.5) + 0.1
