"""CPU: the built library's rk_als_gcl_* names and argument checks, the pins of the numpy restatement
(tests/simgcl_util.py) -- its gradient against torch autograd of the loss written out densely, its noise against
hand-computed integers -- the memory arithmetic, and what train_simgcl refuses before any GPU work."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from tests import lightgcn_util as lg, simgcl_util as sg
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_gcl_contrast", "rk_als_gcl_contrast_workspace_bytes", "rk_als_gcl_propagate"]


# ------------------------------------------------------------------ library
def test_the_library_exports_exactly_the_declared_gcl_names(built):
  from recoder_amd import _als_lib, simgcl
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_gcl_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_gcl_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)
  cap = re.search(r"^#define RK_ALS_GCL_MAX_BATCH (\d+)$", open(header).read(), flags=re.M)
  assert cap and int(cap.group(1)) == _als_lib.GCL_MAX_BATCH == simgcl.MAX_BATCH >= 2048


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib, simgcl
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()
  prop = lambda *a: lib.rk_als_gcl_propagate(*a, None)
  key = (0.1, 0, 0, 1, 1, 0)                                 # eps, seed, step, view, layer, side
  assert prop(p, p, p, p, 0, 4, p, 4, 8, p, 8, None, 0, 1.0, *key) == -2 and "ldf >= h" in err()
  assert err().startswith("rk_als_gcl_propagate: ")
  assert prop(p, p, p, p, 3, 2, p, 8, 8, p, 8, None, 0, 1.0, *key) == -2 and "row_lo" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, None, 0, None, 0, 1.0, *key) == -2 and "Out / Acc" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, p, 4, 1.0, *key) == -2 and "lda >= h" in err()
  assert prop(p, p, p, p, 0, 4, p, 600, 513, p, 600, None, 0, 1.0, *key) == -2
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, -0.1, 0, 0, 1, 1, 0) == -2 and "eps" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, float("nan"), 0, 0, 1, 1, 0) == -2 and "eps" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, 0.1, 0, -1, 1, 1, 0) == -2 and "step >= 0" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, 0.1, 0, 0, 256, 1, 0) == -2 and "view" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, 0.1, 0, 0, 1, 256, 0) == -2 and "layer" in err()
  assert prop(p, p, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, 0.1, 0, 0, 1, 1, 2) == -2 and "side" in err()
  assert prop(p, None, p, p, 0, 4, p, 8, 8, p, 8, None, 0, 1.0, *key) == -2 and "null pointer" in err()
  assert prop(None, None, None, None, 4, 4, None, 8, 8, p, 8, None, 0, 1.0, *key) == 0          # (no rows)
  assert lib.rk_als_gcl_contrast_workspace_bytes(0, 8) == -2 == simgcl.contrast_workspace_bytes(0, 8)
  assert lib.rk_als_gcl_contrast_workspace_bytes(simgcl.MAX_BATCH + 1, 8) == -2
  assert lib.rk_als_gcl_contrast_workspace_bytes(8, 513) == -2 == simgcl.contrast_workspace_bytes(8, 513)
  for T, h in ((1, 1), (300, 65), (simgcl.MAX_BATCH, 512)):
    assert lib.rk_als_gcl_contrast_workspace_bytes(T, h) == simgcl.contrast_workspace_bytes(T, h) > 4 * T * T
  big = 1 << 30
  con = lambda *a: lib.rk_als_gcl_contrast(*a, None)
  assert con(p, 8, 5, p, 4, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, big, p, p) == -2 and "ld1, ld2, ldg1, ldg2 >= h" in err()
  assert err().startswith("rk_als_gcl_contrast: ")
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 4, p, big, p, p) == -2 and "ldg2 >= h" in err()
  assert con(p, 0, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, big, p, p) == -2 and "1 <= T <= 4096" in err()
  assert con(p, 4097, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, big, p, p) == -2 and "1 <= T <= 4096" in err()
  assert con(p, 8, 0, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, big, p, p) == -2 and "n_rows >= 1" in err()
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.0, 0.5, p, 8, p, 8, p, big, p, p) == -2 and "tau" in err()
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.2, -1.0, p, 8, p, 8, p, big, p, p) == -2 and "weight" in err()
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, 100, p, p) == -2 and "workspace too small" in err()
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, None, big, p, p) == -2 and "workspace too small" in err()
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, ctypes.c_void_p(20), big, p, p) == -2 and "16-byte" in err()
  assert con(p, 8, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, big, None, p) == -2 and "null pointer" in err()
  assert con(None, 8, 5, p, 8, p, 8, 8, 0.2, 0.5, p, 8, p, 8, p, big, p, p) == -2 and "null pointer" in err()


# -------------------------------------------------------------------- noise
_M64 = (1 << 64) - 1


def _mix_int(z):
  """splitmix64's output function with Python integers."""
  z = (z + 0x9E3779B97F4A7C15) & _M64
  z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
  z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
  return z ^ (z >> 31)


def _m_int(seed, step, view, layer, side, row, col):
  key = _mix_int(_mix_int(seed & _M64) ^ ((step << 32) | 0x80000000 | (view << 16) | (layer << 8) | side))
  return ((_mix_int((_mix_int((key + row) & _M64) + col) & _M64) >> 41) << 1) | 1


def test_the_noise_is_the_integer_function_it_is_said_to_be():
  for seed, step, view, layer, side in ((0, 0, 1, 1, 0), (-7, 3, 2, 8, 1), (2 ** 63 - 1, 2 ** 31 - 1, 255, 255, 1)):
    key = sg.noise_key(seed, step, view, layer, side)
    m = sg.noise_m(key, [0, 5, 2 ** 31 - 1], 9)
    assert m.dtype == np.uint64
    for a, row in enumerate((0, 5, 2 ** 31 - 1)):
      assert [int(v) for v in m[a]] == [_m_int(seed, step, view, layer, side, row, c) for c in range(9)]
  # three values worked out by hand from the definition above
  assert _m_int(0, 0, 1, 1, 0, 0, 0) == PINS[0] and _m_int(0, 0, 1, 1, 0, 5, 3) == PINS[1]
  assert _m_int(-7, 3, 2, 8, 1, 2 ** 31 - 1, 8) == PINS[2]
  # the sampler's slot keys never carry the tag: a slot is below 2^24
  from recoder_amd import bpr
  assert bpr.MAX_BATCH <= 1 << 24 < sg.TAG


PINS = (13726657, 7653897, 8742003)


def test_the_noise_has_length_eps_in_the_orthant_of_the_row():
  rng = np.random.RandomState(0)
  for h in (1, 4, 65, 512):
    key = sg.noise_key(3, 2, 1, 2, 0)
    m = sg.noise_m(key, np.arange(40), h)
    assert np.all(m % 2 == 1) and m.min() >= 1 and m.max() < 2 ** 24          # u = m 2^-24 in (0, 1), never 0
    u = m.astype(np.float64) * 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # (exact in f32)
    x = rng.randn(40, h)
    x[3] = 0
    x[7, ::2] = 0
    # y - x carries the rounding of y: at most 2^-53 (2^-24) |y| <= 4 units an element, sqrt(h) of them in the norm
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-4)):
      y = sg.perturb(x.astype(dtype), 0.1, key, dtype)
      d = y.astype(np.float64) - x.astype(dtype)
      assert y.dtype == dtype
      np.testing.assert_allclose(np.sqrt((d[[0, 1, 2, 4]] ** 2).sum(1)), 0.1, rtol=tol)
      assert np.all(np.sign(d) == np.sign(x.astype(dtype)))
      assert not y[3].any() and not np.signbit(y[3]).any() and not d[7, ::2].any()
      np.testing.assert_allclose(np.abs(d[0]) / 0.1, u[0] / np.sqrt((u[0] ** 2).sum()), rtol=0, atol=40 * tol)
      assert np.array_equal(sg.perturb(x.astype(dtype), 0.0, key, dtype), x.astype(dtype))
      # the rows' own indices decide, not their position
      assert np.array_equal(sg.perturb(x[5:9].astype(dtype), 0.1, key, dtype, rows=np.arange(5, 9)), y[5:9])
  base = dict(seed=1, step=4, view=1, layer=2, side=0)
  rows = [sg.noise_m(sg.noise_key(**base), [6], 16)]
  for name, other in (("seed", 2), ("step", 5), ("view", 2), ("layer", 1), ("side", 1)):
    rows.append(sg.noise_m(sg.noise_key(**dict(base, **{name: other})), [6], 16))
  rows.append(sg.noise_m(sg.noise_key(**base), [7], 16))
  assert len({r.tobytes() for r in rows}) == len(rows)


# -------------------------------------------------------------- restatement
def _matrix():
  """30 x 40 at density 0.2: row 4 empty, column 6 empty."""
  rng = np.random.RandomState(3)
  m = (rng.rand(30, 40) < 0.2).astype(np.float32)
  m[4, :] = 0
  m[:, 6] = 0
  m = sp.csr_matrix(m)
  m.sort_indices()
  assert (np.diff(m.indptr) == 0).sum() == 1 and (np.bincount(m.indices, minlength=40) == 0).sum() == 1
  return m


def _batch(m, T=24):
  """Stored entries with duplicate users and duplicate positives, negatives the user does not hold, slot 5 invalid."""
  rng = np.random.RandomState(1)
  coo = m.tocoo()
  e = rng.randint(0, m.nnz, T)
  e[1], e[2] = e[0], e[0]                                      # (the same user and positive three times)
  users, pos = coo.row[e].astype(np.int32), coo.col[e].astype(np.int32)
  e[3] = np.nonzero((coo.row == users[0]) & (coo.col != pos[0]))[0][0]
  users[3], pos[3] = coo.row[e[3]], coo.col[e[3]]              # (the same user, another positive)
  dense = m.toarray() > 0
  neg = np.array([rng.choice(np.nonzero(~dense[u])[0]) for u in users], np.int32)
  neg[5] = -1
  ok = neg >= 0
  assert len(set(users[ok])) < ok.sum() and len(set(pos[ok])) < ok.sum()
  return users, pos, neg


def _torch_loss(m, E, K, users, pos, neg, reg, w, eps, tau, seed, step):
  """SELFRec's SimGCL loss written out: dense adjacency, sign, normalize, logsumexp; the noise's u / |u| is data."""
  U, n = m.shape
  A = torch.tensor(lg.adjacency(m))
  T = len(users)
  ok = neg >= 0
  u, i, j = (torch.tensor(a[ok].astype(np.int64)) for a in (users, pos, neg))

  def tables(view):
    L, tot = E, 0
    for k in range(1, K + 1):
      L = A @ L
      if view:
        unit = np.concatenate([sg.perturb(np.ones((rows, E.shape[1])), 1.0, sg.noise_key(seed, step, view, k, side)) - 1
                               for side, rows in ((0, U), (1, n))])
        L = L + eps * torch.sign(L) * torch.tensor(unit)
      tot = tot + L
    return tot / K
  W = tables(0)
  x = (W[u] * (W[U + i] - W[U + j])).sum(1)
  loss = F.softplus(-x).sum() / T
  loss = loss + 0.5 * reg * ((E[u] ** 2).sum() + (E[U + i] ** 2).sum() + (E[U + j] ** 2).sum()) / T
  if w > 0:
    W1, W2 = tables(1), tables(2)
    for idx in (torch.unique(u), U + torch.unique(i)):
      z1, z2 = F.normalize(W1[idx], dim=1), F.normalize(W2[idx], dim=1)
      S = z1 @ z2.T / tau
      loss = loss + w * (torch.logsumexp(S, 1) - torch.diagonal(S)).mean()
  return loss


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("w", [0.5, 0.0])
def test_the_restated_gradient_equals_autograd_of_the_loss_written_out(K, w):
  m, h, reg, eps, tau, seed, step = _matrix(), 8, 0.3, 0.1, 0.2, 5, 7
  rng = np.random.RandomState(K)
  Eu, Ei = rng.randn(30, h), rng.randn(40, h)
  users, pos, neg = _batch(m)
  E = torch.tensor(np.concatenate([Eu, Ei]), requires_grad=True)
  loss = _torch_loss(m, E, K, users, pos, neg, reg, w, eps, tau, seed, step)
  want = torch.autograd.grad(loss, E)[0].numpy()
  gu, gi, _, _, cu, ci, ls, cl = sg.gradient(m, Eu, Ei, K, users, pos, neg, reg, w, eps, tau, seed, step)
  got = np.concatenate([gu, gi])
  scale = np.abs(want).max()
  print("K %d, cl_weight %g: max |gradient| %.3g, largest difference / it %.3g" % (K, w, scale, np.abs(got - want).max() / scale))
  assert scale > 1e-3 and np.abs(got - want).max() <= 1e-9 * scale
  assert cu[4] == 0 and not got[4].any() and (cl > 0) == (w > 0)
  if w == 0:                                                   # plain BPR at the layer-0-free mean
    W = torch.tensor(np.concatenate(sg.forward(m, Eu, Ei, K)))
    assert np.abs(W.numpy() - np.concatenate(sg.forward(m, Eu, Ei, K, eps=0.0, view=1))).max() == 0
    A = lg.adjacency(m)
    mean = sum(np.linalg.matrix_power(A, k) for k in range(1, K + 1)) / K
    np.testing.assert_allclose(W.numpy(), mean @ np.concatenate([Eu, Ei]), rtol=1e-12, atol=1e-14)


def test_the_restated_contrast_on_its_edge_cases():
  rng = np.random.RandomState(2)
  V1, V2 = rng.randn(10, 5), rng.randn(10, 5)
  loss, m, G1, G2 = sg.contrast([3], V1, V2, 0.2)
  assert loss == 0 and m == 1 and not G1.any() and not G2.any()               # (one row: log of one term)
  loss, m, G1, G2 = sg.contrast([10, -1, 12], V1, V2, 0.2)
  assert loss == 0 and m == 0 and not G1.any()
  V1[2] = 0
  loss, m, G1, G2 = sg.contrast([7, 2, 2, 5, 7, 10], V1, V2, 0.2)
  assert m == 3 and loss > 0 and not G1[2].any() and G2[2].any() and G1[5].any()
  assert not G1[[0, 1, 3, 4, 6, 8, 9]].any() and not G2[[0, 1, 3, 4, 6, 8, 9]].any()
  eps = 1e-6                                                   # (finite differences on one row of either view)
  for V, G in ((V1, G1), (V2, G2)):
    for c in range(5):
      old = V[7, c]
      V[7, c] = old + eps
      up = sg.contrast([7, 2, 2, 5, 7, 10], V1, V2, 0.2)[0]
      V[7, c] = old - eps
      down = sg.contrast([7, 2, 2, 5, 7, 10], V1, V2, 0.2)[0]
      V[7, c] = old
      assert abs((up - down) / (2 * eps) - G[7, c]) <= 1e-6 * np.abs(G).max()


def test_the_restated_noisy_propagation_stays_inside_its_own_bound():
  """What tests/test_simgcl.py asks of the kernel, asked of the float32 restatement on the CPU."""
  rng = np.random.RandomState(4)
  m = _matrix()
  su, si = lg.scales(m)
  for h in (1, 4, 65):
    Fm = rng.randn(40, h).astype(np.float32)
    key = sg.noise_key(0, 1, 2, 3, 0)
    got, _ = sg.propagate(m, su, si, Fm, np.float32(0.1), key, np.float32)
    ratio, amb = sg.noisy_errors(got, m, su, si, Fm, float(np.float32(0.1)), key)
    print("h %d: largest err / (2 x bound) %.3f, ambiguous signs %d of %d" % (h, ratio.max(), amb.sum(), amb.size))
    assert got.dtype == np.float32 and ratio.max() <= 1 and amb.mean() <= 0.01
    assert not got[4].any() and not np.signbit(got[4]).any()
    same, _ = sg.propagate(m, su, si, Fm, np.float32(0.0), key, np.float32)
    assert np.array_equal(same, lg.propagate(m, su, si, Fm, np.float32)[0])


# ------------------------------------------------------------------ memory
def test_required_bytes_adds_the_views_and_the_contrast_to_lightgcn():
  from recoder_amd import lightgcn, simgcl
  base = (1000, 500, 64, 20000, 256)
  need = simgcl.required_bytes(*base)
  r256 = lambda x: -(-x // 256) * 256
  ws = 4 * r256(4 * 256 * 64) + r256(4 * 256 * 256) + 5 * r256(4 * 256)
  assert simgcl.contrast_workspace_bytes(256, 64) == ws
  assert need == lightgcn.required_bytes(*base) + 2 * 1500 * 64 * 4 + ws + 2 * 256 * 16
  assert simgcl.required_bytes(*base, contrast=False) == lightgcn.required_bytes(*base)
  for k in range(5):
    more = list(base)
    more[k] += 1
    assert simgcl.required_bytes(*more) > need, k
  assert simgcl.required_bytes(*base, allocate_state=False) == need - 3 * 1500 * 64 * 4
  assert simgcl.check_memory(*base, free_bytes=1 << 30) == need
  with pytest.raises(ValueError, match="SimGCL needs 1 <= batch_size <= 4096 and 1 <= h <= 512 \\(got 4097, 64\\)"):
    simgcl.check_memory(10, 10, 64, 10, 4097, free_bytes=1 << 30)
  with pytest.raises(ValueError, match="SimGCL over 1000 users x 500 items at h = 64 with 20000 entries and batches "
                                       "of 256 needs %d bytes of device memory, 1000 are free" % need):
    simgcl.check_memory(*base, free_bytes=1000)
  from recoder_amd.device import DEVICE_HBM_BYTES
  users = DEVICE_HBM_BYTES // (512 * 4 * 10)
  with pytest.raises(ValueError, match="SimGCL over %d users x 1000 items .* more than one device's memory" % users):
    simgcl.check_memory(users, 1000, 512, 5, 256, free_bytes=float("inf"))
  assert simgcl.check_data(1000, 10, 5, 256) == 4
  with pytest.raises(ValueError, match="train_simgcl needs at least one stored entry"):
    simgcl.check_data(0, 10, 1, 256)


# ------------------------------------------------------------------ refusals
def _no_gpu(monkeypatch):
  import recoder_amd.simgcl  # noqa: F401
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
  return not rec._Recoder__model_initialized and rec.simgcl_state is None and rec.simgcl_history == [] and \
      rec.lightgcn_state is None and rec.optimizer is None


def test_check_config_accepts_the_contract():
  from recoder_amd import simgcl
  assert simgcl.check_config(_mf(4), 2, 3, 256, 0.01, 1e-4, 0.5, 0.1, 0.2, 0) == (2, 3, 256, 0.01, 1e-4, 0.5, 0.1, 0.2, 0)
  assert simgcl.check_config(_mf(512), np.int64(8), 0, simgcl.MAX_BATCH, np.float32(0.5), 0, 0, 0, 1, -7) == \
      (8, 0, simgcl.MAX_BATCH, 0.5, 0.0, 0.0, 0.0, 1.0, -7)


def test_train_simgcl_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_simgcl trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_simgcl trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_simgcl needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_simgcl needs dropout_prob == 0"),
    (_mf(0), {}, "train_simgcl supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_simgcl supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"num_layers": 0}, "num_layers must be an integer in 1..8 \\(got 0\\)"),
    (_mf(4), {"num_layers": 9}, "num_layers must be an integer in 1..8 \\(got 9\\)"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"lr": float("nan")}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..4096 \\(got 0\\)"),
    (_mf(4), {"batch_size": 4097}, "batch_size must be an integer in 1..4096 \\(got 4097\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"cl_eps": -0.1}, "cl_eps must be finite and >= 0"),
    (_mf(4), {"cl_eps": float("inf")}, "cl_eps must be finite and >= 0"),
    (_mf(4), {"cl_temperature": 0}, "cl_temperature must be finite and > 0"),
    (_mf(4), {"cl_temperature": -0.2}, "cl_temperature must be finite and > 0"),
    (_mf(4), {"cl_weight": -0.5}, "cl_weight must be finite and >= 0"),
    (_mf(4), {"cl_weight": True}, "cl_weight must be finite and >= 0"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"seed": 2 ** 63}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_simgcl"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.train_simgcl(_dataset(), **kw)
    assert _uninitialised(rec), message
  from recoder_amd import simgcl
  state = {"num_layers": 2, "E0": (torch.zeros(40, 4), torch.zeros(40, 4))}
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 3\\)"):
    simgcl.check_resume(state, 3)
  with pytest.raises(ValueError, match="do not match the model's"):
    simgcl.check_resume(state, 2, ((40, 4), (41, 4)))
  simgcl.check_resume(state, 2, ((40, 4), (40, 4)))
  # a LightGCN state on the same Recoder is not SimGCL's
  rec = Recoder(model=_mf(4))
  rec.lightgcn_state = state
  with pytest.raises(ValueError, match="resume=True needs the state of an earlier train_simgcl"):
    rec.train_simgcl(_dataset(), resume=True)


def test_train_simgcl_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(NotImplementedError, match="train_simgcl runs on one GPU"):
    rec.train_simgcl(_dataset())
  assert _uninitialised(rec)
