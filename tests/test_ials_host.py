"""iALS++ without a GPU: the float64 restatement of tests/ials_util.py pins itself (L never rises over a block step,
block_size = h is the closed-form ridge solve), the permutation, the regularisers, the refusals of
recoder_amd.ials, the signature and the binding; and the float32 errors that size tests/test_ials.py's bounds."""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

from . import ials_util as U
from .abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NAMES = {"rk_als_ials_max_h": 0, "rk_als_ials_max_block": 0, "rk_als_ials_predict": 11, "rk_als_ials_block": 21,
         "rk_als_ials_panel_workspace_bytes": 3, "rk_als_ials_gram_panel": 11,
         "rk_als_ials_objective_workspace_bytes": 0, "rk_als_ials_objective": 18}


def test_library_exports_and_binds_ials(built):
  from recoder_amd import _als_lib, ials
  for name, argc in NAMES.items():
    assert name in exports(built.ALS_LIB)
    assert name in declared([os.path.join(INC, "recoder_als.h")])
    assert len(_als_lib.SIGNATURES[name][1]) == argc, name
  lib = _als_lib.load()
  assert lib.rk_als_ials_max_h() == _als_lib.IALS_MAX_H == ials.MAX_H == 2048
  assert lib.rk_als_ials_max_block() == _als_lib.IALS_MAX_BLOCK == ials.MAX_BLOCK == 128
  assert lib.rk_als_max_h() == 512                       # (the CG solver's limit stays)
  assert lib.rk_als_ials_panel_workspace_bytes(2000, 200, 64) == 2 * 64 * 200 * 4
  assert lib.rk_als_ials_panel_workspace_bytes(10, 64, 65) < 0 and lib.rk_als_ials_panel_workspace_bytes(10, 2049, 8) < 0
  assert lib.rk_als_ials_objective_workspace_bytes() == 8192


def test_entry_points_refuse_bad_arguments(built):
  from recoder_amd import _als_lib
  lib = _als_lib.load()
  p = 4096                                               # (never dereferenced: every case is refused first)
  good = [p, p, None, 0, 4, None, 0, p, 16, p, 16, 16, p, 16, p, 0.5, 8, 8, p, p, None]

  def call(**change):
    a = list(good)
    for i, v in change.items():
      a[int(i[1:])] = v
    return lib.rk_als_ials_block(*a)
  assert call(_11=2049, _8=2049, _10=2049, _13=2049) == -2        # h
  assert call(_17=129) == -2 and call(_17=0) == -2 and call(_16=9) == -2 and call(_16=-1) == -2
  assert call(_8=15) == -2 and call(_10=15) == -2 and call(_13=15) == -2
  assert call(_3=5, _4=4) == -2 and call(_3=-1) == -2
  assert call(_6=-1) == -2 and call(_6=3) == -2                    # n_long < 0; a count without a list
  for alpha0 in (-1.0, float("nan"), float("inf")):
    assert call(_15=alpha0) == -2
  for i in (0, 1, 7, 9, 12, 14, 18, 19):
    assert call(**{"_%d" % i: None}) == -2, i
  assert call(_4=0) == 0                                           # no rows: nothing is launched
  assert lib.rk_als_ials_predict(p, p, 4, 0, p, 8, p, 8, 8, p, None) == 0
  assert lib.rk_als_ials_predict(p, p, 4, 5, p, 7, p, 8, 8, p, None) == -2


def _problem(seed, n_users=25, n_items=31, h=12):
  m = U.random_csr(n_users, n_items, 0.25, seed, empty_rows=(2,), empty_cols=(4,))
  rng = np.random.RandomState(seed + 1)
  return m, rng.randn(n_users, h), rng.randn(n_items, h)


@pytest.mark.parametrize("nu", [0.0, 0.5, 1.0])
def test_objective_never_rises_over_a_block_step_and_falls_over_sweeps(nu):
  m, X, Y = _problem(3)
  mt, perm = U.transpose_permutation(m)
  lam, mu = U.regularisers(m, 0.3, 0.05, nu)
  last, sweeps = U.objective(m, X, Y, lam, mu, 0.3), []
  for s in range(3):
    cache = U.predict(m, X, Y)
    for p0, k in U.blocks(12, 5):                           # (blocks of 5, 5 and 2)
      for side in (0, 1):
        if side == 0:
          U.block_step(m, None, Y, X, U.gram_panel(Y, p0, k), lam, 0.3, p0, k, cache)
        else:
          U.block_step(mt, perm, X, Y, U.gram_panel(X, p0, k), mu, 0.3, p0, k, cache)
        L = U.objective(m, X, Y, lam, mu, 0.3)
        assert abs(L - U.objective(m, X, Y, lam, mu, 0.3, cache)) <= 1e-10 * L       # the cache follows the tables
        assert L <= last * (1 + 1e-12)
        last = L
    sweeps.append(last)
  assert sweeps[0] > sweeps[1] > sweeps[2]
  Xf, Yf, hist = U.fit(m, *_problem(3)[1:], 0.3, 0.05, nu, 5, 3, lam_dtype=np.float64)
  np.testing.assert_allclose(hist, sweeps, rtol=1e-12)
  Xq, Yq, histq = U.fit(m, *_problem(3)[1:], 0.3, 0.05, nu, 5, 3, lam_dtype=np.float64, fast=True)
  np.testing.assert_allclose(histq, sweeps, rtol=1e-10)


def test_full_block_is_the_closed_form_ridge_solve():
  m, X, Y = _problem(7)
  lam, mu = U.regularisers(m, 0.2, 0.1, 1.0)
  cache = U.predict(m, X, Y)
  U.block_step(m, None, Y, X, U.gram_panel(Y, 0, 12), lam, 0.2, 0, 12, cache)
  # (relative to the table: the row without entries is exactly zero in the closed form)
  want = np.array([U.ridge_row(m.indices[m.indptr[u]:m.indptr[u + 1]], Y, lam[u], 0.2) for u in range(m.shape[0])])
  assert np.abs(X - want).max() <= 1e-10 * np.abs(want).max()
  mt, perm = U.transpose_permutation(m)
  U.block_step(mt, perm, X, Y, U.gram_panel(X, 0, 12), mu, 0.2, 0, 12, cache)
  want = np.array([U.ridge_row(mt.indices[mt.indptr[i]:mt.indptr[i + 1]], X, mu[i], 0.2) for i in range(m.shape[1])])
  assert np.abs(Y - want).max() <= 1e-10 * np.abs(want).max()


def test_permutation_maps_every_item_major_entry_to_its_twin():
  from recoder_amd import ials
  m = U.random_csr(40, 23, 0.3, 5, empty_rows=(0, 9), empty_cols=(3,), full_cols=(7,))
  mt, perm = U.transpose_permutation(m)
  mt2, perm2 = ials.transpose_permutation(m)
  assert np.array_equal(perm, perm2) and np.array_equal(perm, U.transpose_permutation_fast(m))
  assert np.array_equal(mt.indptr, mt2.indptr) and np.array_equal(mt.indices, mt2.indices)
  rows = np.repeat(np.arange(40), np.diff(m.indptr))
  for i in range(23):
    for e in range(mt.indptr[i], mt.indptr[i + 1]):
      assert m.indices[perm[e]] == i and rows[perm[e]] == mt.indices[e]
  assert sorted(perm.tolist()) == list(range(m.nnz))


def test_regularisers():
  from recoder_amd import ials
  m = U.random_csr(9, 6, 0.4, 2, empty_rows=(1,))
  r, d = np.diff(m.indptr), np.bincount(m.indices, minlength=6)
  lam, mu = ials.regularisers(r, d, 0.5, 0.2, 1.0)
  np.testing.assert_allclose(lam, 0.2 * (r + 0.5 * 6), rtol=1e-15)
  np.testing.assert_allclose(mu, 0.2 * (d + 0.5 * 9), rtol=1e-15)
  lam, mu = ials.regularisers(r, d, 0.5, 0.2, 0.5)
  np.testing.assert_allclose(lam, 0.2 * np.sqrt(r + 3.0), rtol=1e-15)
  lam, mu = ials.regularisers(r, d, 0.0, 0.2, 0.0)         # nu = 0: reg, an empty row at alpha0 = 0 included
  assert (lam == 0.2).all() and (mu == 0.2).all() and lam.dtype == np.float64
  for a, b in zip(ials.regularisers(r, d, 0.5, 0.2, 1.0), U.regularisers(m, 0.5, 0.2, 1.0)):
    assert np.array_equal(a, b)
  assert ials.blocks(200, 64) == [(0, 64), (64, 64), (128, 64), (192, 8)] == U.blocks(200, 64)


def test_bounds_of_the_gpu_tests_are_four_times_the_float32_restatement():
  """The constants of tests/test_ials.py against a fresh measurement (another BLAS may sum in another order: a factor
  of 2 either way is let through, the constants themselves stay)."""
  from . import test_ials as T

  def near(constant, measured):
    return constant / 2 <= measured <= 2 * constant
  for h, (cp, cn) in T.KERNEL_F32_ERR.items():
    ep, en = U.kernel_f32_errors(h)
    assert near(cp, ep) and near(cn, en), (h, ep, en)
    assert T.KERNEL_BOUND[h] == (4 * cp, 4 * cn)
  for case, err in T.BLOCK_F32_ERR.items():
    assert near(err, U.block_f32_error(case)), case
  assert sorted(T.BLOCK_F32_ERR) == sorted(U.BLOCK_CASES)
  assert near(T.EMPTY_F32_ERR, U.empty_f32_error())
  m, X0, Y0 = U.big_problem()
  tab, L = U.fit_f32_errors(m, X0, Y0, 0.1, 0.01, U.BIG_BLOCK, U.BIG_SWEEPS, fast64=False)
  assert near(T.BIG_F32_ERR[0], tab) and near(T.BIG_F32_ERR[1], L), (tab, L)


def test_bounds_of_the_slice_subset_fit():
  """TABLE_BOUND and L_BOUND of tests/test_ials.py from the float32 fit on the subset, and the Recall@20 cap they give,
  from the restatement alone: below 0.01 (it is 0 of 1326 users)."""
  from recoder_amd import ials
  from . import test_ials as T
  assert (ials.DEFAULT_ALPHA0, ials.DEFAULT_REG) == (U.SUB_ALPHA0, U.SUB_REG)
  x, y, X0, Y0 = U.subset_problem()
  tab, L = U.fit_f32_errors(x, X0, Y0, U.SUB_ALPHA0, U.SUB_REG, U.SUB_BLOCK, U.SUB_SWEEPS)
  print("subset fit: tables %.4g, L %.4g" % (tab, L))
  assert T.SUB_F32_ERR[0] / 2 <= tab <= 2 * T.SUB_F32_ERR[0] and T.SUB_F32_ERR[1] / 2 <= L <= 2 * T.SUB_F32_ERR[1]
  assert (T.TABLE_BOUND, T.L_BOUND) == (4 * T.SUB_F32_ERR[0], 4 * T.SUB_F32_ERR[1])
  X, Y, _ = U.fit(x, X0, Y0, U.SUB_ALPHA0, U.SUB_REG, 1.0, U.SUB_BLOCK, U.SUB_SWEEPS, fast=True)
  S = X @ Y.T
  for u in range(S.shape[0]):
    S[u, x.indices[x.indptr[u]:x.indptr[u + 1]]] = -np.inf
  top = -np.sort(-S, axis=1)[:, :21]
  has = np.diff(y.indptr) > 0
  close = (top[:, 19] - top[:, 20] < T.TABLE_BOUND * np.abs(top[np.isfinite(top)]).max()) & has
  assert close.sum() / has.sum() < 0.01


# ------------------------------------------------------------------------------------------------------- refusals
def _no_gpu(monkeypatch):
  from recoder_amd import _als_lib, device
  import recoder_amd.model as model_mod

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(_als_lib, "load", no_gpu)


def test_signature_and_defaults():
  from recoder_amd import ials
  from recoder_amd.model import Recoder
  sig = inspect.signature(Recoder.train_ials).parameters
  assert list(sig) == ["self", "train_dataset", "num_sweeps", "block_size", "alpha0", "reg", "nu", "init_std", "seed",
                       "val_dataset", "eval_metric", "eval_freq", "eval_batch_size", "eval_num_users", "patience",
                       "restore_best"]
  assert (sig["num_sweeps"].default, sig["block_size"].default, sig["nu"].default, sig["init_std"].default,
          sig["seed"].default, sig["eval_freq"].default, sig["eval_batch_size"].default,
          sig["restore_best"].default) == (16, 64, 1.0, None, 0, 1, 500, False)
  assert (sig["alpha0"].default, sig["reg"].default) == (ials.DEFAULT_ALPHA0, ials.DEFAULT_REG)
  for name in ("check_config", "csr_pair", "fit", "required_bytes", "check_memory"):
    assert callable(getattr(ials, name))


def test_train_ials_refuses_before_any_gpu_work(monkeypatch):
  import recoder_amd.ials  # noqa: F401
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, MatrixFactorization
  _no_gpu(monkeypatch)
  ds = RecommendationDataset(sp.csr_matrix(np.eye(5, dtype=np.float32)))
  nan, inf = float("nan"), float("inf")
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_ials trains a MatrixFactorization, not DynamicAutoencoder"),
    (MatrixFactorization(8, activation_type="tanh"), {}, "train_ials needs activation_type='none'"),
    (MatrixFactorization(8, dropout_prob=0.1), {}, "train_ials needs dropout_prob == 0"),
    (MatrixFactorization(0), {}, "train_ials supports embedding sizes 1..2048 \\(got 0\\)"),
    (MatrixFactorization(2049), {}, "train_ials supports embedding sizes 1..2048 \\(got 2049\\)"),
    (MatrixFactorization(8), {"block_size": 0}, "block_size must be an integer in 1..128"),
    (MatrixFactorization(8), {"block_size": 129}, "block_size must be an integer in 1..128"),
    (MatrixFactorization(8), {"num_sweeps": -1}, "num_sweeps must be an integer"),
    (MatrixFactorization(8), {"init_std": -1.0}, "init_std must be a finite number >= 0"),
    (MatrixFactorization(8), {"seed": 1.5}, "seed must be an integer"),
    (MatrixFactorization(8), {"patience": 2}, "train_ials: patience needs a val_dataset"),
  ]
  for name in ("alpha0", "reg", "nu"):
    for bad in (-1.0, nan, inf, True):
      cases.append((MatrixFactorization(8), {name: bad}, "%s must be a finite number >= 0" % name))
  for model, kw, message in cases:
    rec = Recoder(model=model, loss="mse", optimizer_type="adam")
    with pytest.raises(ValueError, match=message):
      rec.train_ials(ds, **kw)
    assert getattr(rec.model, "user_embedding_layer", None) is None
  import torch.distributed as dist
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError):
    Recoder(model=MatrixFactorization(8), loss="mse", optimizer_type="adam").train_ials(ds)


def test_memory_check_names_the_sizes():
  from recoder_amd import ials
  assert ials.check_config(__import__("recoder_amd.nn", fromlist=["x"]).MatrixFactorization(20), 3, 64, 0.1, 0.01, 1.0) == \
      (3, 20, 0.1, 0.01, 1.0, None, 0)
  need = ials.required_bytes(1000, 500, 64, 10000, 64)
  assert need > (1000 + 500) * 64 * 4 + 10000 * (4 + 4 + 8 + 4)
  assert ials.required_bytes(1000, 500, 64, 10000, 64, allocate_model=False) < need
  assert ials.check_memory(1000, 500, 64, 10000, 64, free_bytes=need) == need
  with pytest.raises(ValueError, match="iALS\\+\\+ over 1000 users x 500 items at h = 64 .* are free"):
    ials.check_memory(1000, 500, 64, 10000, 64, free_bytes=need - 1)
  with pytest.raises(ValueError, match="more than one device's memory"):
    ials.check_memory(10 ** 8, 10 ** 7, 2048, 10 ** 9, 64, free_bytes=float("inf"))
