"""CPU: the built library's rk_als_sx_* names and argument checks, ``history_positions``, the pin of the numpy
restatement (tests/simplex_util.py) against torch autograd of the dense formulation in float64, the driver's hooks
left at their defaults, and what train_simplex refuses before any GPU work."""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import ccl_util as cu, lightgcn_util as lg, simplex_util as su
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_sx_backward", "rk_als_sx_forward", "rk_als_sx_workspace_bytes"]


# ------------------------------------------------------------------ library
def test_the_library_exports_exactly_the_declared_sx_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_sx_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_sx_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib, simplex
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()

  def fwd(T=8, h=8, ldq=8, ldw=8, ldx=8, ldp=8, gamma=0.5, L=4, E=4, n_items=5, users=p, P=p, hkey=p, hcoef=p, X=p):
    return lib.rk_als_sx_forward(users, T, p, p, 5, n_items, p, ldq, P, ldp, p, ldw, h, gamma, L, E, p, X, ldx, 0,
                                 hkey, hcoef, None)
  for kw in (dict(ldq=4), dict(ldw=4), dict(ldx=4), dict(ldp=4), dict(h=0), dict(h=513, ldq=513, ldw=513, ldx=513, ldp=513)):
    assert fwd(**kw) == -2 and "1 <= h <= 512" in err() and err().startswith("rk_als_sx_forward: "), kw
  for kw in (dict(T=0), dict(T=4097), dict(L=0), dict(L=1025), dict(E=0), dict(E=1025), dict(T=4097, E=1024)):
    assert fwd(**kw) == -2 and "T E <= 2^22" in err(), kw
  assert fwd(n_items=0) == -2 and "n_users, n_items >= 1" in err()
  for g in (-0.01, 1.01, float("nan")):
    assert fwd(gamma=g) == -2 and "0 <= gamma <= 1" in err(), g
  assert fwd(users=None) == -2 and "null pointer" in err()
  assert fwd(X=None) == -2 and "null pointer" in err()
  assert fwd(hkey=None) == -2 and "go together" in err()
  assert fwd(hcoef=None) == -2 and "go together" in err()

  def bwd(T=8, h=8, ldw=8, DU=p, dW=p):
    return lib.rk_als_sx_backward(DU, p, p, T, p, ldw, h, 1.0, p, p, dW, None)
  assert bwd(ldw=4) == -2 and "ldw >= h" in err() and err().startswith("rk_als_sx_backward: ")
  assert bwd(T=0) == -2 and bwd(T=4097) == -2 and "1 <= T <= 4096" in err()
  assert bwd(DU=None) == -2 and "null pointer" in err()
  assert bwd(dW=None) == -2 and "null pointer" in err()
  for T, E, h in ((0, 1, 8), (4097, 1, 8), (8, 0, 8), (8, 1025, 8), (8, 1, 0), (8, 1, 513), (4097, 1024, 8)):
    assert lib.rk_als_sx_workspace_bytes(T, E, h) == -2 == simplex.workspace_bytes(T, E, h), (T, E, h)
  for T, E, h in ((1, 1, 1), (5, 4, 3), (1024, 256, 64), (4096, 1024, 512), (257, 12, 33), (256, 2, 7)):
    got = lib.rk_als_sx_workspace_bytes(T, E, h)
    assert got == simplex.workspace_bytes(T, E, h) >= 4 * (2 * T * h + 2 * T * E + -(-T // 256) * h * h + h * h)
  assert 4096 * 1024 == simplex.MAX_ENTRIES == 1 << 22 and simplex.MAX_HISTORY == 1024 and simplex.CHUNK == su.CHUNK


# ------------------------------------------------------------------ history
def test_history_positions_are_the_rows_own_for_short_rows_and_floor_j_r_over_l_beyond():
  from recoder_amd import simplex
  for L in (1, 4, 64, 1024):
    for r in (0, 1, L - 1, L):
      assert np.array_equal(simplex.history_positions(r, L), np.arange(r)), (r, L)
    for r in (L + 1, 3 * L + 1) + ((2 ** 31 - 1,) if L == 1024 else ()):
      pos = simplex.history_positions(r, L)
      assert pos.dtype == np.int64 and len(pos) == L and pos[0] == 0 and pos[-1] < r
      assert (np.diff(pos) > 0).all() if L > 1 else True
      assert pos.tolist() == [j * r // L for j in range(L)] == su.history_positions(r, L).tolist(), (r, L)
  assert simplex.entry_width([3, 300, 7], 256) == 256 and simplex.entry_width([3, 30, 7], 256) == 30
  assert simplex.entry_width([1, 0], 1) == 2 and simplex.entry_width([], 5) == 2      # (the entry scatter's E >= 2)


# -------------------------------------------------------------- restatement
def _small():
  """7 users x 9 items, h = 5, T = 6, R = 3; user 4 holds nothing, user 2 holds more than L = 3 items."""
  rng = np.random.RandomState(4)
  dense = (rng.rand(7, 9) < 0.4).astype(np.float32)
  dense[4], dense[2] = 0, 1
  dense[2, 5] = 0
  m = sp.csr_matrix(dense)
  P, Q, W = rng.randn(7, 5), rng.randn(9, 5), np.eye(5) + 0.3 * rng.randn(5, 5)
  users, items = np.array([0, 2, 5, 5, 4, 2], np.int32), np.array([1, 4, 6, 8, 6, 0], np.int32)
  negs = su.draws(3, 0, 6, 3, 9)
  return m, P, Q, W, users, items, negs


@pytest.mark.parametrize("gamma,margin,nw", [(0.5, 0.4, 3.0), (0.0, -0.5, 1.5), (0.25, 0.0, 2.0), (1.0, 0.2, 3.0)])
def test_the_float64_gradient_equals_autograd_of_the_dense_formulation(gamma, margin, nw):
  m, P, Q, W, users, items, negs = _small()
  L, T = 3, len(users)
  (dP, dQ, dW), (cu_, ci), loss, cnt, live = su.gradient(m, P, Q, W, gamma, L, users, items, negs, margin, nw)
  assert cnt == T and live > 0 and np.array_equal(cu_, np.bincount(users, minlength=7))
  Pt, Qt, Wt = (torch.tensor(a, requires_grad=True) for a in (P, Q, W))
  A = np.zeros((7, 9))                                          # the dense pooling matrix, written out by hand
  for u in range(7):
    row = np.nonzero(m[u].toarray()[0])[0]
    hist = row if len(row) <= L else row[[j * len(row) // L for j in range(L)]]
    for k in hist:
      A[u, k] += 1.0 / len(hist)
  assert len(np.nonzero(m[2].toarray()[0])[0]) > L and not A[4].any()
  X = gamma * Pt + (1 - gamma) * (torch.tensor(A) @ Qt) @ Wt.T

  def unit(V):
    n = V.norm(dim=1, keepdim=True)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    return torch.where(n > 0, V / safe, torch.zeros_like(V))
  C = unit(X) @ unit(Qt).T
  u = torch.tensor(users.astype(np.int64))
  pos = 1.0 - C[u, torch.tensor(items.astype(np.int64))]
  neg = (nw / 3) * torch.clamp(C[u[:, None], torch.tensor(negs.astype(np.int64))] - float(np.float32(margin)),
                               min=0).sum(1)
  ((pos.sum() + neg.sum()) / T).backward()
  rel = lambda got, want: np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
  # (the relative bound of tests/test_ccl_host.py and tests/test_elsa_host.py for the same kind of check)
  assert rel(dP, Pt.grad.numpy()) <= 1e-10 and rel(dQ, Qt.grad.numpy()) <= 1e-10
  if gamma < 1:
    assert rel(dW, Wt.grad.numpy()) <= 1e-10
  else:
    assert not dW.any() and not Wt.grad.numpy().any()
  assert abs(loss[0] - float(pos.detach().sum())) <= 1e-10 and abs(loss[1] - float(neg.detach().sum())) <= 1e-10 * max(nw, 1)


def test_the_f32_restatement_of_the_chains_stays_beside_float64():
  m, P, Q, W, users, items, negs = _small()
  B, X, hkey, hcoef = su.forward_f32(m, users, Q, P, W, 0.5, 3, 3)
  B64, X64 = su.rows64(m, users, P, Q, W, 0.5, 3)
  assert B.dtype == X.dtype == hcoef.dtype == np.float32 and np.abs(B - B64).max() < 1e-5 and np.abs(X - X64).max() < 1e-5
  assert (hkey[4] == 9).all() and not hcoef[4].any() and not B[4].any() and (hkey[1] < 9).all()
  assert np.allclose(hcoef[1], 1 / 3) and np.array_equal(hkey[1], hkey[5])
  DU = np.random.RandomState(1).randn(6, 5).astype(np.float32)
  valid = np.array([1, 1, 0, 1, 1, 1], np.float32)
  dB, dW = su.backward_f32(DU, valid, B, W, 0.25)
  D = DU * valid[:, None]
  assert np.abs(dB - 0.25 * D @ W).max() < 1e-5 and np.abs(dW - 0.25 * D.T @ B64).max() < 1e-5 and not dB[2].any()


def test_gamma_one_in_the_restatement_is_ccl_and_leaves_w_alone():
  m, P, Q, W, users, items, negs = _small()
  s, c = su.new_state(P, Q), lg.new_state(P, Q)
  a = su.step(m, s, 1.0, 3, users, items, negs, 0.01, 1e-3, 0.2, 3.0)
  b = cu.step(m, c, 0, users, items, negs, 0.01, 1e-3, 0.2, 3.0)
  assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
  assert all(np.array_equal(s[k][i], c[k][i]) for k in ("E0", "M", "V") for i in (0, 1))
  assert np.array_equal(s["E0"][2], np.eye(5)) and not s["M"][2].any() and s["step"] == 1


# ------------------------------------------------------------- the driver
def test_the_drivers_new_hooks_default_to_none_and_the_other_methods_leave_them_there():
  from recoder_amd import ccl, directau, lightgcn, simgcl, simplex, ssm, ultragcn
  hooks = ("step_forward", "full_forward", "backward", "new_state", "check_resume")
  assert lightgcn.Method._fields[-5:] == hooks
  for mod in (lightgcn, simgcl, directau, ssm, ultragcn, ccl):
    assert all(getattr(mod.METHOD, k) is None for k in hooks), mod.__name__
  assert all(getattr(simplex.METHOD, k) is not None for k in hooks)
  assert simplex.METHOD.name == "SimpleX" and simplex.METHOD.method == "train_simplex" and \
      simplex.METHOD.max_batch == 4096 and simplex.METHOD.min_layers == 0


def test_the_extended_driver_still_takes_lightgcns_step_unchanged(monkeypatch):
  """``method_step`` of a method without hooks, its kernels replaced by the float64 restatement: forward, draw,
  gradient, backward propagation and Adam on both sides, in that order, give tests/lightgcn_util.py's step."""
  from recoder_amd import bpr, lightgcn
  from tests import bpr_util
  tr, _ = bpr_util.planted()
  n_users, n_items = tr.shape
  h, T, K, lr, reg = 6, 64, 2, 0.05, 1e-3
  rng = np.random.RandomState(2)
  Eu, Ei = 0.3 * rng.randn(n_users, h), 0.3 * rng.randn(n_items, h)
  want = lg.new_state(Eu, Ei)
  users, pos, neg = bpr_util.sample(tr, 7, 5, T)
  lg.step(tr, want, K, users, pos, neg, lr, reg)
  calls = []
  t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
  state = {"E0": (t64(Eu), t64(Ei)), "M": (t64(0 * Eu), t64(0 * Ei)), "V": (t64(0 * Eu), t64(0 * Ei)), "step": 0,
           "num_layers": K}

  class B:
    pass
  ws = B()
  ws.bpr, ws.layers = B(), None
  ws.bpr.T, ws.bpr.users, ws.bpr.pos, ws.bpr.neg = T, None, None, None
  ws.G, ws.H = (t64(0 * Eu), t64(0 * Ei)), (t64(0 * Eu), t64(0 * Ei))
  ws.count = (torch.zeros(n_users, dtype=torch.int32), torch.zeros(n_items, dtype=torch.int32))

  def forward(graph, base, num_layers, layers, out, skip_layer0=False, noise=None):
    calls.append("forward")
    for o, v in zip(out, lg.forward(tr, base[0].numpy(), base[1].numpy(), num_layers)):
      o.copy_(t64(v))

  def sample(csr, seed, step, u, p, n):
    calls.append("sample")
    ws.bpr.drawn = bpr_util.sample(tr, seed, step, T)

  def gradient(X, Y, graph, state, ws, seed, step_index, hyper):
    calls.append("gradient")
    u, p, n = ws.bpr.drawn
    _, g, ls, D, Pt = bpr_util.grad(u, p, n, X.numpy(), Y.numpy(), np.zeros(n_items), np.float64)
    Gu, Gi, cu_, ci = lg.scatter(u, p, n, g, D, Pt, n_users, n_items)
    for o, v in zip(ws.G + ws.count, (Gu, Gi, cu_, ci)):
      o.copy_(torch.tensor(v))

  def adam(E0, H, count, reg_scale, M, V, lr_, t):
    calls.append("adam")
    for o, v in zip((E0, M, V), lg.adam(E0.numpy(), H.numpy(), count.numpy(), reg_scale, M.numpy(), V.numpy(), lr_, t)):
      o.copy_(t64(v))
  monkeypatch.setattr(lightgcn, "forward", forward)
  monkeypatch.setattr(bpr, "sample", sample)
  monkeypatch.setattr(lightgcn, "adam", adam)
  method = lightgcn.METHOD._replace(gradient=gradient)
  graph = B()
  graph.ucsr = None
  X, Y = t64(0 * Eu), t64(0 * Ei)
  lightgcn.method_step(method, X, Y, graph, state, ws, 7, 5, lr, reg)
  assert calls == ["forward", "sample", "gradient", "forward", "adam", "adam"] and state["step"] == 1
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      assert np.array_equal(state[key][side].numpy(), want[key][side]), (key, side)


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


def _dataset(n=40, m=None):
  from recoder_amd.data import RecommendationDataset
  return RecommendationDataset(sp.csr_matrix(np.eye(n, dtype=np.float32)) if m is None else m)


def _mf(h=4, **kw):
  from recoder_amd.nn import MatrixFactorization
  return MatrixFactorization(h, **kw)


def _uninitialised(rec):
  return not rec._Recoder__model_initialized and rec.simplex_state is None and rec.simplex_history == [] and \
      rec.simplex_stats == [] and rec.optimizer is None


def test_train_simplex_exists_with_the_signature_of_the_contract():
  from recoder_amd import simplex
  from recoder_amd.model import Recoder
  sig = inspect.signature(Recoder.train_simplex)
  assert list(sig.parameters) == ["self", "train_dataset", "gamma", "max_history", "num_epochs", "batch_size", "lr",
                                  "reg", "num_negatives", "negative_weight", "margin", "normalize", "seed", "resume",
                                  "val_dataset", "eval_metric", "eval_freq", "eval_batch_size", "eval_num_users",
                                  "patience", "restore_best"]
  d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
  assert (d["max_history"], d["batch_size"], d["lr"], d["reg"], d["num_negatives"], d["negative_weight"], d["margin"],
          d["normalize"], d["seed"], d["resume"]) == (256, 1024, 0.01, 1e-3, 64, 16.0, 0.0, False, 0, False)
  assert (d["val_dataset"], d["eval_metric"], d["eval_freq"], d["eval_batch_size"], d["eval_num_users"], d["patience"],
          d["restore_best"]) == (None, None, 1, 500, None, None, True)
  assert 0.0 <= d["gamma"] <= 1.0 and d["num_epochs"] >= 1
  c = simplex.check_config(_mf(64), *(d[k] for k in list(sig.parameters)[2:13]))
  assert c[0] == (d["gamma"], 256) and c[1:] == (d["num_epochs"], 1024, 0.01, 1e-3, 64, 16.0, 0.0, False, 0)
  rec = Recoder(model=_mf(4))
  assert rec.simplex_state is None and rec.simplex_history == [] and rec.simplex_stats == [] and \
      rec.simplex_validation is None
  assert list(inspect.signature(Recoder.simplex_encode).parameters) == ["self", "interactions_matrix"]
  for name in ("check_config", "check_resume", "check_data", "required_bytes", "check_memory", "history_positions",
               "forward", "backward", "encode", "Workspace", "step", "fit", "METHOD", "workspace_bytes"):
    assert hasattr(simplex, name), name


def test_train_simplex_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd import simplex
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  long_rows = sp.csr_matrix(np.ones((40, 1100), np.float32))
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_simplex trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_simplex trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_simplex needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_simplex needs dropout_prob == 0"),
    (_mf(0), {}, "train_simplex supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_simplex supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"gamma": -0.01}, "gamma must be a number in \\[0, 1\\] \\(got -0.01\\)"),
    (_mf(4), {"gamma": 1.01}, "gamma must be a number in \\[0, 1\\] \\(got 1.01\\)"),
    (_mf(4), {"gamma": float("nan")}, "gamma must be a number in \\[0, 1\\]"),
    (_mf(4), {"gamma": True}, "gamma must be a number in \\[0, 1\\]"),
    (_mf(4), {"gamma": "0.5"}, "gamma must be a number in \\[0, 1\\]"),
    (_mf(4), {"max_history": 0}, "max_history must be an integer in 1..1024 \\(got 0\\)"),
    (_mf(4), {"max_history": 1025}, "max_history must be an integer in 1..1024 \\(got 1025\\)"),
    (_mf(4), {"max_history": 8.0}, "max_history must be an integer in 1..1024"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..4096 \\(got 0\\)"),
    (_mf(4), {"batch_size": 4097}, "batch_size must be an integer in 1..4096 \\(got 4097\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"num_negatives": 0}, "num_negatives must be an integer in 1..1024 \\(got 0\\)"),
    (_mf(4), {"num_negatives": 1025}, "num_negatives must be an integer in 1..1024 \\(got 1025\\)"),
    (_mf(4), {"batch_size": 4093, "num_negatives": 1024}, "must be at most 4194304 \\(got 4093 \\* 1025\\)"),
    (_mf(4), {"negative_weight": -1}, "negative_weight must be finite and >= 0"),
    (_mf(4), {"margin": 1.0}, "margin must be a number in \\[-1, 1\\) \\(got 1.0\\)"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_simplex"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    kw = dict(kw)
    ds = _dataset(m=kw.pop("train", None))
    with pytest.raises(ValueError, match=message):
      rec.train_simplex(ds, **kw)
    assert _uninitialised(rec), message
  # batch_size * E over the entry scatter's cap (E = min(max_history, the longest stored row), from the host matrix):
  # 4096 * 1024 is the cap itself, so the limits on T and max_history keep every fit under it; one entry less shows it
  monkeypatch.setattr(simplex, "MAX_ENTRIES", 4096 * 1024 - 1)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="must be at most 4194303 \\(got 4096 \\* 1024\\): lower max_history or batch_size"):
    rec.train_simplex(_dataset(m=long_rows), batch_size=4096, max_history=1024, num_negatives=8)
  assert _uninitialised(rec)
  monkeypatch.undo()
  with pytest.raises(ValueError, match="lower max_history or batch_size"):
    simplex.check_entries(4096, 1025)
  simplex.check_entries(4096, 1024)
  state = {"gamma": 0.5, "max_history": 8, "E0": (torch.zeros(40, 4), torch.zeros(40, 4), torch.zeros(4, 4))}
  with pytest.raises(ValueError, match="continues a fit with gamma = 0.5 and max_history = 8 \\(got 0.25 and 8\\)"):
    simplex.check_resume(state, (0.25, 8))
  with pytest.raises(ValueError, match="continues a fit with gamma = 0.5 and max_history = 8 \\(got 0.5 and 9\\)"):
    simplex.check_resume(state, (0.5, 9))
  with pytest.raises(ValueError, match="do not match the model's"):
    simplex.check_resume(state, (0.5, 8), ((40, 4), (41, 4)))
  simplex.check_resume(state, (0.5, 8), ((40, 4), (40, 4)))


def test_resume_with_another_gamma_or_history_is_refused_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  state = {"gamma": 0.5, "max_history": 8, "E0": (torch.zeros(40, 4), torch.zeros(40, 4), torch.zeros(4, 4))}
  for kw in ({"gamma": 0.25, "max_history": 8}, {"gamma": 0.5, "max_history": 9}):
    rec = Recoder(model=_mf(4))
    rec.simplex_state = state
    with pytest.raises(ValueError, match="resume=True continues a fit with gamma = 0.5 and max_history = 8"):
      rec.train_simplex(_dataset(), resume=True, **kw)
    assert rec.simplex_state is state and rec.simplex_history == []
  rec = Recoder(model=_mf(4))                                  # (another method's state is not this one's)
  rec.ccl_state = state
  with pytest.raises(ValueError, match="resume=True needs the state of an earlier train_simplex"):
    rec.train_simplex(_dataset(), resume=True)


def test_the_wrappers_refuse_sizes_outside_the_kernels_limits(monkeypatch):
  from recoder_amd import simplex
  _no_gpu(monkeypatch)
  i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
  f32 = lambda *s: torch.zeros(s, dtype=torch.float32)

  class Csr:
    shape, indptr, indices = (5, 6), torch.zeros(6, dtype=torch.int64), i32(1)
  Q, W, X = f32(6, 4), f32(4, 4), f32(5, 4)
  for T, L, gamma in ((4097, 4, 0.5), (8, 0, 0.5), (8, 1025, 0.5), (8, 4, 1.5), (8, 4, -0.1)):
    with pytest.raises(ValueError, match="rk_als_sx_forward needs 1 <= T <= 4096"):
      simplex.forward(i32(T), Csr, Q, None, W, gamma, L, X)
  with pytest.raises(ValueError, match="rk_als_sx_forward needs 1 <= T <= 4096"):
    simplex.forward(i32(8), Csr, Q, None, W, 0.5, 4, X, hkey=i32(8, 1025), hcoef=f32(8, 1025))
  with pytest.raises(ValueError, match="rk_als_sx_backward needs 1 <= T <= 4096"):
    simplex.backward(f32(4097, 4), f32(4097), f32(4097, 4), W, 1.0, f32(4097, 4), f32(17, 4, 4), f32(4, 4))
  base = simplex.required_bytes(100000, 1000000, 64, 10 ** 7, 1024, 64, 256)
  assert simplex.check_memory(100000, 1000000, 64, 10 ** 7, 1024, 64, 256, free_bytes=float("inf")) == base
  assert base - simplex.required_bytes(100000, 1000000, 64, 10 ** 7, 1024, 64, 2) >= 254 * 1024 * (8 + 32)
  assert base > simplex.required_bytes(100000, 1000000, 64, 10 ** 7, 1024, 64, 256, pooled=False)
  with pytest.raises(ValueError, match="SimpleX over 100000 users x 1000000 items .* 1000 are free"):
    simplex.check_memory(100000, 1000000, 64, 10 ** 7, 1024, 64, 256, free_bytes=1000)


def test_train_simplex_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="train_simplex runs on one GPU"):
    rec.train_simplex(_dataset())
  assert _uninitialised(rec)
