"""CPU: the built library's rk_als_dau_* names and argument checks, the pin of the numpy restatement
(tests/directau_util.py) -- its gradient against torch autograd of the loss written out densely as the paper's
code writes it -- the memory arithmetic, and what train_directau refuses before any GPU work."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from tests import directau_util as du, lightgcn_util as lg
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_dau_grad", "rk_als_dau_workspace_bytes"]


# ------------------------------------------------------------------ library
def test_the_library_exports_exactly_the_declared_dau_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_dau_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_dau_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib, directau
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()
  big = 1 << 30
  dau = lambda *a: lib.rk_als_dau_grad(*a, None)
  assert dau(p, p, 8, 5, 5, p, 4, p, 8, 8, 1.0, p, big, p, p, p, p, p) == -2 and "ldx, ldy >= h" in err()
  assert err().startswith("rk_als_dau_grad: ")
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 513, 1.0, p, big, p, p, p, p, p) == -2 and "1 <= h <= 512" in err()
  assert dau(p, p, 0, 5, 5, p, 8, p, 8, 8, 1.0, p, big, p, p, p, p, p) == -2 and "1 <= T <= 4096" in err()
  assert dau(p, p, 4097, 5, 5, p, 8, p, 8, 8, 1.0, p, big, p, p, p, p, p) == -2 and "1 <= T <= 4096" in err()
  assert dau(p, p, 8, 0, 5, p, 8, p, 8, 8, 1.0, p, big, p, p, p, p, p) == -2 and "n_users, n_items >= 1" in err()
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 8, -1.0, p, big, p, p, p, p, p) == -2 and "gamma" in err()
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 8, float("nan"), p, big, p, p, p, p, p) == -2 and "gamma" in err()
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 8, 1.0, p, 100, p, p, p, p, p) == -2 and "workspace too small" in err()
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 8, 1.0, None, big, p, p, p, p, p) == -2 and "workspace too small" in err()
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 8, 1.0, ctypes.c_void_p(20), big, p, p, p, p, p) == -2 and "16-byte" in err()
  assert dau(p, p, 8, 5, 5, p, 8, p, 8, 8, 1.0, p, big, p, p, None, p, p) == -2 and "null pointer" in err()
  assert dau(None, p, 8, 5, 5, p, 8, p, 8, 8, 1.0, p, big, p, p, p, p, p) == -2 and "null pointer" in err()
  # the workspace formula
  assert lib.rk_als_dau_workspace_bytes(0, 8) == -2 == directau.grad_workspace_bytes(0, 8)
  assert lib.rk_als_dau_workspace_bytes(directau.MAX_BATCH + 1, 8) == -2 == directau.grad_workspace_bytes(4097, 8)
  assert lib.rk_als_dau_workspace_bytes(8, 513) == -2 == directau.grad_workspace_bytes(8, 513)
  r256 = lambda x: -(-x // 256) * 256
  for T, h in ((1, 1), (300, 65), (directau.MAX_BATCH, 512)):
    want = 4 * r256(4 * T * h) + r256(4 * T * T) + 5 * r256(4 * T) + 256
    assert lib.rk_als_dau_workspace_bytes(T, h) == directau.grad_workspace_bytes(T, h) == want
    assert want == lib.rk_als_gcl_contrast_workspace_bytes(T, h) + 256              # (one T x T tile for both sides)


# ----------------------------------------------------------------- gradient
def _matrix():
  """30 x 40 at density 0.2: row 4 empty, column 6 empty."""
  rng = np.random.RandomState(3)
  m = (rng.rand(30, 40) < 0.2).astype(np.float32)
  m[4, :] = 0
  m[:, 6] = 0
  m = sp.csr_matrix(m)
  m.sort_indices()
  return m


def _batch(m, T=24):
  """Stored entries: the same pair three times, the same user with another item, slot 5 and slot 6 invalid."""
  rng = np.random.RandomState(1)
  coo = m.tocoo()
  e = rng.randint(0, m.nnz, T)
  e[1], e[2] = e[0], e[0]
  users, items = coo.row[e].astype(np.int32), coo.col[e].astype(np.int32)
  e3 = np.nonzero((coo.row == users[0]) & (coo.col != items[0]))[0][0]
  users[3], items[3] = coo.row[e3], coo.col[e3]
  users[5], items[6] = -1, m.shape[1]
  return users, items


def _torch_loss(m, E, K, users, items, reg, gamma):
  """The paper's code: alignment = mean |normalize(x) - normalize(y)|^2, uniformity =
  log mean exp(-2 pdist(normalize(x))^2), loss = align + gamma (unif_users + unif_items) / 2; LightGCN's encoder
  as the dense adjacency; the L2 term of the rows a slot touches."""
  U, n = m.shape
  A = torch.tensor(lg.adjacency(m))
  L, tot = E, E
  for _ in range(K):
    L = A @ L
    tot = tot + L
  W = tot / (K + 1)
  ok = du.valid_slots(users, items, U, n)
  u, i = torch.tensor(users[ok].astype(np.int64)), torch.tensor(items[ok].astype(np.int64))
  x, y = F.normalize(W[u], dim=-1), F.normalize(W[U + i], dim=-1)
  align = (x - y).norm(p=2, dim=1).pow(2).mean()
  unif = lambda z: torch.pdist(z, p=2).pow(2).mul(-2).exp().mean().log()
  loss = align + gamma * (unif(x) + unif(y)) / 2
  return loss + 0.5 * reg * ((E[u] ** 2).sum() + (E[U + i] ** 2).sum()) / len(users)


@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("gamma", [1.0, 0.0, 5.0])
def test_the_restated_gradient_equals_autograd_of_the_loss_written_out(K, gamma):
  """Measured here: the largest difference over the six cases is 1.3e-15 of the largest gradient entry (float64
  on both sides, sums of a few dozen terms); the assertion allows 1e-12."""
  m, h, reg = _matrix(), 8, 0.3
  rng = np.random.RandomState(K)
  Eu, Ei = rng.randn(30, h), rng.randn(40, h)
  users, items = _batch(m)
  ok = du.valid_slots(users, items, 30, 40)
  assert ok.sum() == 22 and len(set(zip(users[ok], items[ok]))) < ok.sum()     # (a duplicated pair)
  E = torch.tensor(np.concatenate([Eu, Ei]), requires_grad=True)
  loss = _torch_loss(m, E, K, users, items, reg, gamma)
  want = torch.autograd.grad(loss, E)[0].numpy()
  gu, gi, _, _, cu, ci, losses, cnt = du.gradient(m, Eu, Ei, K, users, items, reg, gamma)
  got = np.concatenate([gu, gi])
  scale = np.abs(want).max()
  print("K %d, gamma %g: max |gradient| %.3g, largest difference / it %.3g"
        % (K, gamma, scale, np.abs(got - want).max() / scale))
  assert scale > 1e-3 and np.abs(got - want).max() <= 1e-12 * scale
  assert cnt == 22 and cu.sum() == ci.sum() == 22 and cu[4] == 0 and ci[6] == 0
  # the restated loss is the dense one, and the one written from the rows' differences
  P, Q = lg.forward(m, Eu, Ei, K)
  total = losses[0] + 0.5 * gamma * (losses[1] + losses[2])
  l2 = 0.5 * reg * ((Eu[users[ok]] ** 2).sum() + (Ei[items[ok]] ** 2).sum()) / len(users)
  assert abs(total + l2 - loss.item()) <= 1e-12 * abs(loss.item())
  assert abs(total - du.dense_loss(users, items, P, Q, gamma)) <= 1e-12 * abs(total)


def test_the_restated_loss_on_its_edge_cases():
  rng = np.random.RandomState(2)
  X, Y = rng.randn(10, 5), rng.randn(12, 5)
  (al, uu, ui), m, valid, DU, DI = du.grad_rows([3], [4], X, Y, 1.0)
  assert m == 1 and uu == 0 and ui == 0 and al > 0 and DU.any() and DI.any()    # (one slot: alignment alone)
  (al, uu, ui), m, valid, DU, DI = du.grad_rows([10, -1, 3], [0, 0, 12], X, Y, 1.0)
  assert m == 0 and (al, uu, ui) == (0.0, 0.0, 0.0) and not valid.any() and not DU.any() and not DI.any()
  # every slot the same pair: the uniformity is log(1) and its gradient vanishes
  (al, uu, ui), m, _, DU, DI = du.grad_rows([3] * 6, [4] * 6, X, Y, 5.0)
  one = du.grad_rows([3], [4], X, Y, 5.0)
  assert m == 6 and abs(uu) < 1e-15 and abs(ui) < 1e-15 and abs(al - one[0][0]) < 1e-15
  assert np.abs(DU.sum(0) - one[3][0]).max() < 1e-15 and np.abs(DI.sum(0) - one[4][0]).max() < 1e-15
  # a zero row: z = 0, at distance 1 from every unit row, and no gradient on its own side
  X[2] = 0
  users, items = [7, 2, 2, 5, 7, 10], [1, 3, 3, 0, 1, 2]
  (al, uu, ui), m, valid, DU, DI = du.grad_rows(users, items, X, Y, 2.0)
  assert m == 5 and valid.tolist() == [1, 1, 1, 1, 1, 0] and not DU[1].any() and not DU[2].any() and DI[1].any()
  assert not DU[5].any() and not DI[5].any()
  z = du.normalise(X[[7, 2]])[0]
  assert abs(du.weights(z)[0, 1] - np.exp(-2.0)) < 1e-15
  eps = 1e-6                                                   # (finite differences on one row of either table)
  for V, D, row, slots in ((X, DU, 7, [0, 4]), (Y, DI, 3, [1, 2])):
    for c in range(5):
      old = V[row, c]
      V[row, c] = old + eps
      up = du.dense_loss(users, items, X, Y, 2.0)
      V[row, c] = old - eps
      down = du.dense_loss(users, items, X, Y, 2.0)
      V[row, c] = old
      assert abs((up - down) / (2 * eps) - D[slots, c].sum()) <= 1e-6 * np.abs(D).max()


def test_the_float32_restatement_stays_beside_float64():
  m = _matrix()
  rng = np.random.RandomState(4)
  Eu, Ei = rng.randn(30, 8).astype(np.float32), rng.randn(40, 8).astype(np.float32)
  users, items = _batch(m)
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  l64, c64 = du.step(m, s64, 2, users, items, 0.05, 1e-3, 1.0)
  l32, c32 = du.step(m, s32, 2, users, items, 0.05, 1e-3, 1.0, np.float32)
  assert c64 == c32 == 22 and np.allclose(l64, l32, rtol=0, atol=1e-5)
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      assert s32[key][side].dtype == np.float32 and np.abs(s32[key][side] - s64[key][side]).max() < 1e-4


# ------------------------------------------------------------------ memory
def test_required_bytes_adds_the_workspace_and_two_sorts_to_lightgcn():
  from recoder_amd import directau, lightgcn
  base = (1000, 500, 64, 20000, 256)
  need = directau.required_bytes(*base)
  assert need == lightgcn.required_bytes(*base) + directau.grad_workspace_bytes(256, 64) + 16 + 2 * 2 * 256 * 16
  for k in range(5):
    more = list(base)
    more[k] += 1
    assert directau.required_bytes(*more) > need, k
  assert directau.required_bytes(*base, allocate_state=False) == need - 3 * 1500 * 64 * 4
  assert directau.check_memory(*base, free_bytes=1 << 30) == need
  with pytest.raises(ValueError, match="DirectAU needs 1 <= batch_size <= 4096 and 1 <= h <= 512 \\(got 4097, 64\\)"):
    directau.check_memory(10, 10, 64, 10, 4097, free_bytes=1 << 30)
  with pytest.raises(ValueError, match="DirectAU needs 1 <= batch_size <= 4096 and 1 <= h <= 512 \\(got 256, 513\\)"):
    directau.check_memory(10, 10, 513, 10, 256, free_bytes=1 << 30)
  with pytest.raises(ValueError, match="DirectAU over 1000 users x 500 items at h = 64 with 20000 entries and batches "
                                       "of 256 needs %d bytes of device memory, 1000 are free" % need):
    directau.check_memory(*base, free_bytes=1000)
  from recoder_amd.device import DEVICE_HBM_BYTES
  users = DEVICE_HBM_BYTES // (512 * 4 * 8)
  with pytest.raises(ValueError, match="DirectAU over %d users x 1000 items .* more than one device's memory" % users):
    directau.check_memory(users, 1000, 512, 5, 256, free_bytes=float("inf"))
  assert directau.check_data(1000, 10, 5, 256) == 4
  with pytest.raises(ValueError, match="train_directau needs at least one stored entry"):
    directau.check_data(0, 10, 1, 256)
  with pytest.raises(ValueError, match="train_directau draws a stored entry with 32-bit arithmetic"):
    directau.check_data(2 ** 31, 10, 1, 256)
  with pytest.raises(ValueError, match="num_epochs \\* ceil\\(nnz / batch_size\\) must be below 2\\^31"):
    directau.check_data(2 ** 30, 10, 2 ** 20, 1)


# ------------------------------------------------------------------ refusals
def _no_gpu(monkeypatch):
  import recoder_amd.directau  # noqa: F401
  import recoder_amd.model as model_mod
  from recoder_amd import _als_lib, device

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
  return not rec._Recoder__model_initialized and rec.directau_state is None and rec.directau_history == [] and \
      rec.lightgcn_state is None and rec.simgcl_state is None and rec.optimizer is None


def test_check_config_accepts_the_contract_and_no_layer():
  from recoder_amd import directau, lightgcn
  assert directau.check_config(_mf(4), 2, 3, 256, 0.01, 1e-4, 0.5, 0) == (2, 3, 256, 0.01, 1e-4, 0.5, 0)
  assert directau.check_config(_mf(512), np.int64(0), 0, directau.MAX_BATCH, np.float32(0.5), 0, 0, -7) == \
      (0, 0, directau.MAX_BATCH, 0.5, 0.0, 0.0, -7)
  with pytest.raises(ValueError, match="num_layers must be an integer in 1..8 \\(got 0\\)"):
    lightgcn.check_config(_mf(4), 0, 1, 256, 0.01, 1e-3, 0)


def test_train_directau_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_directau trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_directau trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_directau needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_directau needs dropout_prob == 0"),
    (_mf(0), {}, "train_directau supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_directau supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"num_layers": -1}, "num_layers must be an integer in 0..8 \\(got -1\\)"),
    (_mf(4), {"num_layers": 9}, "num_layers must be an integer in 0..8 \\(got 9\\)"),
    (_mf(4), {"num_layers": 1.0}, "num_layers must be an integer in 0..8"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"lr": float("nan")}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..4096 \\(got 0\\)"),
    (_mf(4), {"batch_size": 4097}, "batch_size must be an integer in 1..4096 \\(got 4097\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"gamma": -0.5}, "gamma must be finite and >= 0"),
    (_mf(4), {"gamma": float("inf")}, "gamma must be finite and >= 0"),
    (_mf(4), {"gamma": True}, "gamma must be finite and >= 0"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"seed": 2 ** 63}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_directau"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.train_directau(_dataset(), **kw)
    assert _uninitialised(rec), message
  from recoder_amd import directau
  state = {"num_layers": 2, "E0": (torch.zeros(40, 4), torch.zeros(40, 4))}
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 0\\)"):
    directau.check_resume(state, 0)
  with pytest.raises(ValueError, match="do not match the model's"):
    directau.check_resume(state, 2, ((40, 4), (41, 4)))
  directau.check_resume(state, 2, ((40, 4), (40, 4)))
  # a LightGCN or SimGCL state on the same Recoder is not DirectAU's, and no layer is still no LightGCN
  rec = Recoder(model=_mf(4))
  rec.lightgcn_state = rec.simgcl_state = state
  with pytest.raises(ValueError, match="resume=True needs the state of an earlier train_directau"):
    rec.train_directau(_dataset(), resume=True)
  with pytest.raises(ValueError, match="num_layers must be an integer in 1..8 \\(got 0\\)"):
    rec.train_lightgcn(_dataset(), num_layers=0)
  with pytest.raises(ValueError, match="num_layers must be an integer in 1..8 \\(got 0\\)"):
    rec.train_simgcl(_dataset(), num_layers=0)


def test_train_directau_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="train_directau runs on one GPU"):
    rec.train_directau(_dataset())
  assert _uninitialised(rec)
