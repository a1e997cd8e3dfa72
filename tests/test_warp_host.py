"""CPU: the restatement of the WARP / DNS sampler (tests/warp_util.py) pinned against bpr_util's sampler and
against its own literal per-slot walk, the rank-weight table, what warp.check_config and train_warp refuse
before any GPU work, the workspace arithmetic, and the built library's two new names."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util, warp_util
from tests.abi_util import built, exports  # noqa: F401  (built: a fixture)


def _mf(h=4, **kw):
  from recoder_amd.nn import MatrixFactorization
  return MatrixFactorization(h, **kw)


# --------------------------------------------------------------- restatement
@pytest.mark.parametrize("seed, step", [(0, 0), (-(2 ** 40) - 3, 7)])
def test_dns_with_one_candidate_and_32_draws_is_the_bpr_sampler(seed, step):
  m = bpr_util.edge_matrix()
  X, Y, b = bpr_util.init_tables(37, 53, 5, 1)
  got = warp_util.Sampler(m).sample(seed, step, 257, X, Y, b, warp_util.DNS, 32, 1)
  want = bpr_util.sample(m, seed, step, 257)
  assert (want[2] < 0).any() and (want[2] >= 0).any()
  for a, w in zip(got[:3], want):
    assert a.dtype == w.dtype and np.array_equal(a, w)
  assert np.array_equal(got[3], (want[2] >= 0).astype(np.int32))


@pytest.mark.parametrize("mode, max_draws, num_candidates, margin", [
    (warp_util.WARP, 32, 1, 1.0), (warp_util.WARP, 65, 1, 0.0), (warp_util.WARP, 1, 1, 0.25),
    (warp_util.DNS, 32, 4, 0.0), (warp_util.DNS, 65, 65, 0.0), (warp_util.DNS, 7, 2, 0.0)])
def test_the_literal_sampler_equals_the_vectorised_one(mode, max_draws, num_candidates, margin):
  """Exact tables (h = 3: ties and near-margin scores are common), so float64 sums agree in any order."""
  m = bpr_util.edge_matrix()
  X, Y, b = warp_util.exact_tables(37, 53, 3, 2, high_bias_users=(3, 11), csr=m)
  sm = warp_util.Sampler(m)
  got = sm.sample(5, 3, 150, X, Y, b, mode, max_draws, num_candidates, margin)
  want = sm.sample_literal(5, 3, 150, X, Y, b, mode, max_draws, num_candidates, margin)
  for name, a, w in zip(("users", "pos", "neg", "trials", "s_pos", "s_neg", "scores"), got, want):
    assert np.array_equal(a, w), name
  users, _, neg, trials = got[:4]
  assert (neg[users == 5] == -1).all() and (users == 5).any()          # (the user who holds everything)
  assert ((neg >= 0) == (trials > 0)).all() and trials.max() <= (max_draws if mode == warp_util.WARP else num_candidates)
  if mode == warp_util.WARP and max_draws > 1:
    assert (trials > 1).any() and ((neg < 0) & (users != 5)).any()     # (a later violator; no violator at all)


def test_weight_table_values():
  from recoder_amd import warp
  for kind in ("log", "harmonic"):
    w = warp.weight_table(13, kind)
    assert w.dtype == np.float32 and w.shape == (257,) and w[0] == 0
    assert np.array_equal(w, warp_util.weight_table(13, kind))
  # (n_items - 1) // N = 12, 6, 4, 3, 2, 2, 1, ... 1 (N = 12), 0 from N = 13
  log, har = warp.weight_table(13, "log"), warp.weight_table(13, "harmonic")
  assert np.array_equal(log[1:8], np.float32([math.log(v) for v in (12, 6, 4, 3, 2, 2, 1)])) and not log[7:].any()
  H = lambda r: sum(1.0 / k for k in range(1, r + 1))
  np.testing.assert_allclose(har[1:8], [H(12), H(6), H(4), H(3), H(2), H(2), 1.0], rtol=2.0 ** -23)
  assert (har[7:13] == 1).all() and not har[13:].any()
  big = warp.weight_table(20108, "harmonic")
  assert abs(big[1] - (math.log(20107) + 0.5772156649 + 0.5 / 20107)) < 1e-5
  with pytest.raises(ValueError, match="rank_weight must be 'log' or 'harmonic'"):
    warp.weight_table(13, "linear")


# ------------------------------------------------------------------ refusals
def test_check_config_accepts_and_refuses():
  from recoder_amd import warp
  from recoder_amd.nn import DynamicAutoencoder
  ok = (3, 256, 0.05, 0.01, 1.0, 32, "log", 0)
  assert warp.check_config(_mf(4), *ok) == ok
  assert warp.check_config(_mf(512), 0, 1, np.float32(0.5), 0, 0, 256, "harmonic", -7) == \
      (0, 1, 0.5, 0.0, 0.0, 256, "harmonic", -7)

  def bad(at, value, match, model=None):
    args = list(ok)
    if at is not None:
      args[at] = value
    with pytest.raises(ValueError, match=match):
      warp.check_config(model or _mf(4), *args)
  bad(None, None, "train_warp trains a MatrixFactorization, not DynamicAutoencoder", DynamicAutoencoder(hidden_layers=[8]))
  bad(None, None, "train_warp needs activation_type='none' \\(got 'tanh'\\)", _mf(4, activation_type="tanh"))
  bad(None, None, "train_warp needs dropout_prob == 0", _mf(4, dropout_prob=0.5))
  bad(None, None, "train_warp supports embedding sizes 1..512 \\(got 513\\)", _mf(513))
  for v in (-0.5, float("inf"), float("nan"), "1", True):
    bad(4, v, "margin must be finite and >= 0")
  for v in (0, 257, 32.0, True):
    bad(5, v, "max_draws must be an integer in 1..256")
  for v in ("linear", None, 1):
    bad(6, v, "rank_weight must be 'log' or 'harmonic'")
  bad(2, 0, "lr must be finite and > 0")
  bad(1, 0, "batch_size must be an integer in 1..16777216")


def test_train_warp_and_num_candidates_refuse_before_gpu_work(monkeypatch):
  import recoder_amd.warp  # noqa: F401
  import recoder_amd.model as model_mod
  import torch.distributed as dist
  from recoder_amd import device
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)
  ds = RecommendationDataset(sp.csr_matrix(np.eye(40, dtype=np.float32)))
  with pytest.raises(ValueError, match="max_draws must be an integer in 1..256"):
    Recoder(model=_mf(8)).train_warp(ds, max_draws=300)
  with pytest.raises(ValueError, match="margin must be finite and >= 0"):
    Recoder(model=_mf(8)).train_warp(ds, margin=-1)
  with pytest.raises(ValueError, match="rank_weight"):
    Recoder(model=_mf(8)).train_warp(ds, rank_weight="wsabie")
  for v in (0, 33, 2.0):
    with pytest.raises(ValueError, match="num_candidates must be an integer in 1..32"):
      Recoder(model=_mf(8)).train_bpr(ds, num_candidates=v)
  rec = Recoder(model=_mf(8))
  assert rec.warp_history == [] and rec.warp_stats == []
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError, match="train_warp runs on one GPU"):
    rec.train_warp(ds)


# ----------------------------------------------------------------- workspace
def test_workspace_and_memory_arithmetic():
  from recoder_amd import bpr, warp
  r = lambda x: -(-x // 256) * 256
  for T, h in ((1, 1), (257, 65), (1024, 64), (1 << 24, 512)):
    assert warp.workspace_bytes(T, h) == 8 * r(4 * T) + 2 * r(4 * T * h) == bpr.workspace_bytes(T, h) + 3 * r(4 * T)
  assert warp.workspace_bytes(0, 4) < 0 and warp.workspace_bytes(4, 513) < 0 and warp.workspace_bytes((1 << 24) + 1, 4) < 0
  args = (1000, 500, 64, 20000, 1024)
  assert warp.required_bytes(*args) == bpr.required_bytes(*args) + 3 * r(4 * 1024) + 4 * 257 + 24
  assert warp.check_memory(*args, free_bytes=float("inf")) == warp.required_bytes(*args)
  with pytest.raises(ValueError, match="WARP over 1000 users x 500 items .* needs %d bytes of device memory, 10 are free"
                     % warp.required_bytes(*args, allocate_model=False)):
    warp.check_memory(*args, free_bytes=10, allocate_model=False)
  with pytest.raises(ValueError, match="more than one device's memory"):
    warp.check_memory(10 ** 9, 10 ** 9, 512, 1, 1, free_bytes=float("inf"))
  with pytest.raises(ValueError, match="WARP needs 1 <= batch_size"):
    warp.check_memory(10, 10, 513, 1, 1, free_bytes=float("inf"))


# ------------------------------------------------------------------- library
def test_the_library_exports_and_binds_the_two_entry_points(built):
  from recoder_amd import _als_lib
  names = exports(built.ALS_LIB)
  assert "rk_als_rank_sample" in names and "rk_als_warp_grad" in names
  assert len(_als_lib.SIGNATURES["rk_als_rank_sample"][1]) == 26 and len(_als_lib.SIGNATURES["rk_als_warp_grad"][1]) == 20
  lib = _als_lib.load()
  # argument checks come before any launch: no device needed
  P = lambda: 256                                              # (a non-null stand-in; never dereferenced)
  base = [P(), P(), 3, 5, 7, 0, 0, 4, P(), 8, P(), 8, P(), 8, 0, 32, 1, 1.0, P(), P(), P(), P(), None, None, None, None]

  def refused(at, value, message):
    a = list(base)
    a[at] = value
    assert lib.rk_als_rank_sample(*a) == -2
    assert lib.rk_als_last_error().decode() == "rk_als_rank_sample: " + message
  refused(15, 257, "1 <= max_draws <= 256")
  refused(15, 0, "1 <= max_draws <= 256")
  refused(14, 2, "mode is RK_ALS_RANK_WARP or RK_ALS_RANK_DNS")
  refused(17, -1.0, "margin must be finite and >= 0")
  refused(17, float("inf"), "margin must be finite and >= 0")
  refused(13, 513, "1 <= h <= 512, ldx >= h, ldy >= h")
  refused(9, 4, "1 <= h <= 512, ldx >= h, ldy >= h")
  refused(7, (1 << 24) + 1, "step >= 0, 1 <= T <= 2^24")
  refused(21, None, "null pointer")
  a = list(base)
  a[14], a[16] = 1, 33
  assert lib.rk_als_rank_sample(*a) == -2 and b"1 <= num_candidates <= max_draws" in lib.rk_als_last_error()
  g = [P(), P(), P(), P(), 4, 3, 5, P(), 8, P(), 8, P(), 8, float("nan"), P(), P(), P(), P(), P(), None]
  assert lib.rk_als_warp_grad(*g) == -2
  assert lib.rk_als_last_error().decode() == "rk_als_warp_grad: margin must be finite and >= 0"
  g[13], g[14] = 1.0, None
  assert lib.rk_als_warp_grad(*g) == -2 and lib.rk_als_last_error().decode() == "rk_als_warp_grad: null pointer"
