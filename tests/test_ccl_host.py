"""CPU: the built library's rk_als_ccl_* names and argument checks, the pin of the numpy restatement
(tests/ccl_util.py) -- its coefficients, users' rows, item gradient and loss terms against torch autograd of the
dense formulation in float64, the share of the GPU cases' entries that lie too close to the margin to compare
liveness -- and what train_ccl and the wrappers refuse before any GPU work."""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import ccl_util as cu
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_ccl_grad", "rk_als_ccl_scatter", "rk_als_ccl_workspace_bytes"]


# ------------------------------------------------------------------ library
def test_the_library_exports_exactly_the_declared_ccl_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_ccl_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_ccl_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib, ccl
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()

  def grad(T=8, R=4, step=0, n_users=5, n_items=5, ldx=8, h=8, users=p, live=p):
    return lib.rk_als_ccl_grad(users, p, T, R, 0, step, n_users, n_items, p, ldx, p, 8, h, 0.4, 1.0, p, p, p, p, p, p,
                               p, live, None)
  assert grad(ldx=4) == -2 and "ldx, ldy >= h" in err() and err().startswith("rk_als_ccl_grad: ")
  assert grad(h=513, ldx=513) == -2 and "1 <= h <= 512" in err()
  for kw in (dict(T=0), dict(T=4097), dict(R=0), dict(R=1025), dict(T=4096, R=1024)):       # (both sides: below)
    assert grad(**kw) == -2 and "T (1 + R) <= 2^22" in err(), kw
  assert grad(n_items=0) == -2 and "n_users, n_items >= 1" in err()
  assert grad(step=-1) == -2 and "step >= 0" in err()
  assert grad(users=None) == -2 and "null pointer" in err()
  assert grad(live=None) == -2 and "null pointer" in err()

  def scatter(n=24, E=3, h=8, ldx=8, ldy=8, ldg=8, n_rows=5, keys=p, self_=p, count=p):
    return lib.rk_als_ccl_scatter(keys, p, n, E, p, p, self_, p, ldx, 5, p, ldy, h, 1.0, n_rows, p, ldg, count, None)
  assert scatter(ldg=4) == -2 and "ldx, ldy, ldg >= h" in err() and err().startswith("rk_als_ccl_scatter: ")
  assert scatter(ldy=4) == -2 and "ldx, ldy, ldg >= h" in err()
  for kw in (dict(E=1), dict(n=25), dict(n=0), dict(n=4097 * 3), dict(n=1026 * 2, E=1026),
             dict(n=(1 << 22) + 1025, E=1025)):
    assert scatter(**kw) == -2 and "n = T E" in err(), kw
  assert scatter(n_rows=0) == -2 and "n_rows >= 1" in err()
  for kw in (dict(keys=None), dict(self_=None), dict(count=None)):
    assert scatter(**kw) == -2 and "null pointer" in err(), kw
  # the workspace formula and both sides of its limits
  for T, R, h in ((0, 1, 8), (4097, 1, 8), (8, 0, 8), (8, 1025, 8), (8, 1, 0), (8, 1, 513), (4096, 1024, 8),
                  (4093, 1024, 8)):
    assert lib.rk_als_ccl_workspace_bytes(T, R, h) == -2 == ccl.workspace_bytes(T, R, h), (T, R, h)
  for T, R, h in ((1, 1, 1), (5, 4, 3), (1024, 512, 64), (4096, 1023, 512), (4092, 1024, 512), (4096, 1, 7)):
    got = lib.rk_als_ccl_workspace_bytes(T, R, h)
    assert got == ccl.workspace_bytes(T, R, h) >= 4 * T * (4 * (1 + R) + 3), (T, R, h)
  assert 4092 * 1025 <= 1 << 22 < 4093 * 1025


# -------------------------------------------------------------- restatement
def _small(zero_rows=True):
  """7 users x 11 items, T = 5, R = 4, h = 3; user 2 and item 6 have norm 0 and are in use."""
  rng = np.random.RandomState(4)
  X, Y = rng.randn(7, 3), rng.randn(11, 3)
  users, items = np.array([0, 2, 5, 5, 3], np.int32), np.array([1, 4, 6, 9, 6], np.int32)
  negs = cu.draws(3, 0, 5, 4, 11)
  negs[0, 1], negs[3, 2] = 6, 1                                # (the zero item as a negative; a repeated item)
  if zero_rows:
    X[2], Y[6] = 0, 0
  return X, Y, users, items, negs


@pytest.mark.parametrize("margin,nw", [(0.4, 3.0), (-0.5, 1.5), (0.0, 0.0)])
def test_the_restatement_equals_autograd_in_float64(margin, nw):
  X, Y, users, items, negs = _small()
  r = cu.grad_rows(users, items, negs, X, Y, margin, nw)
  assert r["live"].sum() > 0 and (r["key"] == 11).any() and (r["key"] < 11).any()
  Xt, Yt = torch.tensor(X, requires_grad=True), torch.tensor(Y, requires_grad=True)

  def unit(V):                                                 # (a row of norm 0 gives the zero vector, gradient 0)
    n = V.norm(dim=1, keepdim=True)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    return torch.where(n > 0, V / safe, torch.zeros_like(V))
  C = unit(Xt) @ unit(Yt).T                                    # the dense formulation: every cosine
  u = torch.tensor(users.astype(np.int64))
  pos = 1.0 - C[u, torch.tensor(items.astype(np.int64))]
  neg = (nw / 4) * torch.clamp(C[u[:, None], torch.tensor(negs.astype(np.int64))] - float(np.float32(margin)),
                               min=0).sum(1)
  (pos.sum() + neg.sum()).backward()
  rel = lambda got, want: np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
  Gu = np.zeros_like(X)
  np.add.at(Gu, users.astype(np.int64), r["DU"])
  assert rel(Gu, Xt.grad.numpy()) <= 1e-10 and rel(r["DI"], Yt.grad.numpy()) <= 1e-10
  assert not Gu[2].any() and not r["DI"][6].any()              # the zero-norm rows get gradient 0
  assert rel(r["loss"][:, 0], pos.detach().numpy()) <= 1e-10
  assert np.abs(r["loss"][:, 1] - neg.detach().numpy()).max() <= 1e-10 * max(nw, 1)
  assert abs(r["loss"].sum() - cu.slot_loss(users, items, negs, X, Y, margin, nw)) <= 1e-10
  # the scatter's restatement gives DI from the entries; the sentinels carry nothing
  G, count = cu.scatter_rows(r["key"], r["coef"], r["self"], users, X, Y, 11)
  assert rel(G, r["DI"]) <= 1e-12 and np.array_equal(count, r["count"])
  dead = r["key"] == 11
  assert not r["coef"][dead].any() and not r["self"][dead].any()
  assert np.array_equal(r["cand"][:, 0], items) and np.array_equal(r["cand"][:, 1:], negs)
  assert (r["key"][1] == 11).all() and r["key"][2, 0] == 11 and r["key"][0, 0] == 1   # zero user; zero positive


def test_the_f32_restatement_stays_beside_float64_and_shares_its_liveness():
  for h in (1, 3, 20, 64, 65, 200):
    rng = np.random.RandomState(h)
    X, Y = rng.randn(40, h).astype(np.float32), rng.randn(40, h).astype(np.float32)
    users, items = rng.randint(0, 40, 65).astype(np.int32), rng.randint(0, 40, 65).astype(np.int32)
    negs = cu.draws(5, 9, 65, 5, 40)
    r64 = cu.grad_rows(users, items, negs, X, Y, 0.4, 3.0)
    r32 = cu.grad_rows_f32(users, items, negs, X, Y, 0.4, 3.0)
    far = ~cu.near_margin(r64, 0.4)
    assert np.array_equal(r32["key"][far], r64["key"][far]) and np.array_equal(r32["cand"], r64["cand"])
    for name in ("coef", "self", "DU", "loss"):
      if far.all():
        assert np.abs(r32[name] - r64[name]).max() <= 1e-5 * max(1.0, np.abs(r64[name]).max()), (h, name)
    G32, c32 = cu.scatter_rows(r32["key"], r32["coef"], r32["self"], users, X, Y, 40, np.float32)
    if far.all():
      assert np.abs(G32 - r64["DI"]).max() <= 1e-4 * max(1.0, np.abs(r64["DI"]).max()) and \
          np.array_equal(c32, r64["count"])


def test_the_gpu_cases_leave_at_most_one_percent_of_their_entries_out_of_the_liveness_comparison():
  """The cases of tests/test_ccl.py's comparison against float64: the entries within 1e-5 of the margin."""
  near = total = 0
  for T, R, h in cu.CASES:
    X, Y, users, items = cu.case(T, R, h)
    r = cu.grad_rows(users, items, cu.draws(cu.SEED, cu.STEP, T, R, cu.N), X, Y, cu.MARGIN, cu.NW)
    n = cu.near_margin(r, cu.MARGIN)
    assert n.sum() <= 0.01 * n.size, (T, R, h)
    if h == 1:                                                 # every cosine is +-1 (or 0 for a zero row)
      assert not n.any() and np.isin(np.round(r["cos"], 12), (-1.0, 0.0, 1.0)).all()
    near, total = near + int(n.sum()), total + n.size
  print("entries within 1e-5 of the margin: %d of %d" % (near, total))
  assert near <= 0.01 * total


# ------------------------------------------------------------- the contract
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
  return not rec._Recoder__model_initialized and rec.ccl_state is None and rec.ccl_history == [] and \
      rec.ccl_stats == [] and rec.optimizer is None


def test_train_ccl_exists_with_the_signature_of_the_contract():
  from recoder_amd import ccl
  from recoder_amd.model import Recoder
  sig = inspect.signature(Recoder.train_ccl)
  assert list(sig.parameters) == ["self", "train_dataset", "num_layers", "num_epochs", "batch_size", "lr", "reg",
                                  "num_negatives", "negative_weight", "margin", "normalize", "seed", "resume"]
  d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
  assert d["num_layers"] == 0 and d["batch_size"] == 1024 and d["normalize"] is False and d["seed"] == 0 and \
      d["resume"] is False
  assert ccl.check_config(_mf(64), *(d[k] for k in list(sig.parameters)[2:-1]))[0] == 0
  rec = Recoder(model=_mf(4))
  assert rec.ccl_state is None and rec.ccl_history == [] and rec.ccl_stats == [] and rec.ccl_validation is None
  assert (ccl.MAX_BATCH, ccl.MAX_NEGATIVES, ccl.MAX_ENTRIES, ccl.MAX_H) == (4096, 1024, 1 << 22, 512)
  assert ccl.METHOD.name == "CCL" and ccl.METHOD.method == "train_ccl" and ccl.METHOD.max_batch == 4096 and \
      ccl.METHOD.min_layers == 0


def test_check_config_accepts_the_contract():
  from recoder_amd import ccl
  assert ccl.check_config(_mf(4), 2, 3, 256, 0.01, 1e-4, 7, 2, -1, 1, -3) == \
      (2, 3, 256, 0.01, 1e-4, 7, 2.0, -1.0, True, -3)
  assert ccl.check_config(_mf(512), 0, 0, 4092, np.float32(0.5), 0, 1024, 0, np.float64(0.999), False, 0)[5:9] == \
      (1024, 0.0, 0.999, False)


def test_train_ccl_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd import ccl
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_ccl trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_ccl trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_ccl needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_ccl needs dropout_prob == 0"),
    (_mf(0), {}, "train_ccl supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_ccl supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"num_layers": -1}, "num_layers must be an integer in 0..8 \\(got -1\\)"),
    (_mf(4), {"num_layers": 9}, "num_layers must be an integer in 0..8 \\(got 9\\)"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..4096 \\(got 0\\)"),
    (_mf(4), {"batch_size": 4097}, "batch_size must be an integer in 1..4096 \\(got 4097\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"num_negatives": 0}, "num_negatives must be an integer in 1..1024 \\(got 0\\)"),
    (_mf(4), {"num_negatives": 1025}, "num_negatives must be an integer in 1..1024 \\(got 1025\\)"),
    (_mf(4), {"num_negatives": 8.0}, "num_negatives must be an integer in 1..1024"),
    (_mf(4), {"batch_size": 4093, "num_negatives": 1024}, "must be at most 4194304 \\(got 4093 \\* 1025\\)"),
    (_mf(4), {"negative_weight": -1}, "negative_weight must be finite and >= 0"),
    (_mf(4), {"negative_weight": float("nan")}, "negative_weight must be finite and >= 0"),
    (_mf(4), {"margin": 1.0}, "margin must be a number in \\[-1, 1\\) \\(got 1.0\\)"),
    (_mf(4), {"margin": -1.0001}, "margin must be a number in \\[-1, 1\\)"),
    (_mf(4), {"margin": float("nan")}, "margin must be a number in \\[-1, 1\\)"),
    (_mf(4), {"margin": "0.4"}, "margin must be a number in \\[-1, 1\\)"),
    (_mf(4), {"margin": True}, "margin must be a number in \\[-1, 1\\)"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"seed": 2 ** 63}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_ccl"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.train_ccl(_dataset(), **kw)
    assert _uninitialised(rec), message
  with pytest.raises(TypeError):
    Recoder(model=_mf(4)).train_ccl(_dataset(), val_dataset=_dataset())     # (validation: fit_validation)
  state = {"num_layers": 2, "E0": (torch.zeros(40, 4), torch.zeros(40, 4))}
  with pytest.raises(ValueError, match="do not match the model's"):
    ccl.check_resume(state, 2, ((40, 4), (41, 4)))
  ccl.check_resume(state, 2, ((40, 4), (40, 4)))
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 0\\)"):
    ccl.check_resume(state, 0)
  rec = Recoder(model=_mf(4))                                  # (another method's state is not this one's)
  rec.ultragcn_state = rec.ssm_state = state
  with pytest.raises(ValueError, match="resume=True needs the state of an earlier train_ccl"):
    rec.train_ccl(_dataset(), resume=True)


@pytest.mark.parametrize("settings", [{"val_dataset": None}, {"patience": 2}, {"val_dataset": 1, "epochs": 3}, [1]])
def test_a_bad_fit_validation_is_refused_before_any_gpu_work(settings, monkeypatch):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_mf(4))
  rec.fit_validation = settings
  with pytest.raises(ValueError, match="fit_validation"):
    rec.train_ccl(_dataset(), num_epochs=1)
  assert _uninitialised(rec) and rec.ccl_validation is None


def test_bad_validation_settings_are_refused_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  for settings in ({"val_dataset": _dataset(), "eval_freq": 0}, {"val_dataset": _dataset(), "patience": 0},
                   {"val_dataset": _dataset(41)}):
    rec = Recoder(model=_mf(4))
    rec.fit_validation = settings
    with pytest.raises(ValueError):
      rec.train_ccl(_dataset(), num_epochs=1)
    assert _uninitialised(rec)


def test_the_wrappers_refuse_sizes_outside_the_kernels_limits(monkeypatch):
  from recoder_amd import ccl
  _no_gpu(monkeypatch)
  i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
  f32 = lambda *s: torch.zeros(s, dtype=torch.float32)
  X, Y = f32(5, 4), f32(6, 4)
  for T, R in ((4097, 1), (8, 0), (8, 1025), (4093, 1024)):
    with pytest.raises(ValueError, match="rk_als_ccl_grad needs 1 <= T <= 4096, 1 <= R <= 1024"):
      ccl.grad(i32(T), i32(T), R, 0, 0, X, Y, 0.4, 1.0, i32(1, 1), i32(1, 1), f32(1, 1), f32(1, 1), f32(1, 4), f32(1),
               f32(1, 2), i32(1))
  for n, T, E in ((9, 4, 2), (8, 4, 1), (0, 0, 2), (1026 * 2, 2, 1026)):
    with pytest.raises(ValueError, match="rk_als_ccl_scatter needs n = T E keys"):
      ccl.scatter(i32(n), torch.zeros(n, dtype=torch.int64), E, i32(T), f32(n), f32(n), X, Y, 1.0, f32(6, 4), i32(6))
  base = ccl.required_bytes(100000, 1000000, 64, 10 ** 7, 1024, 512)
  assert ccl.check_memory(100000, 1000000, 64, 10 ** 7, 1024, 512, free_bytes=float("inf")) == base
  assert base - ccl.required_bytes(100000, 1000000, 64, 10 ** 7, 1024, 1) >= 511 * 1024 * 16
  with pytest.raises(ValueError, match="CCL over 100000 users x 1000000 items .* 1000 are free"):
    ccl.check_memory(100000, 1000000, 64, 10 ** 7, 1024, 512, free_bytes=1000)


def test_train_ccl_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="train_ccl runs on one GPU"):
    rec.train_ccl(_dataset())
  assert _uninitialised(rec)
