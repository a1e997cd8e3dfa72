"""CPU: the built library's rk_als_ssm_* names and argument checks, the pin of the numpy restatement
(tests/ssm_util.py) -- its gradient rows against torch autograd of the loss written with F.normalize, mm and
cross_entropy, its shared draws against a known-answer vector -- the memory arithmetic, what train_ssm refuses before
any GPU work, and the restatement's Recall@20 on the planted matrix beside popularity's."""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from tests import bpr_util, lightgcn_util as lg, ssm_util as su
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_ssm_grad", "rk_als_ssm_workspace_bytes"]
DEFAULTS = dict(num_layers=2, num_epochs=10, batch_size=1024, lr=0.01, reg=1e-3, temperature=0.2, num_negatives=1024)


# ------------------------------------------------------------------ library
def test_the_library_exports_exactly_the_declared_ssm_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_ssm_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_ssm_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  import ctypes
  from recoder_amd import _als_lib, ssm
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()
  big = 1 << 40

  def call(T=8, S=4, step=0, n_users=5, n_items=5, ldx=8, h=8, inv_tau=5.0, cosine=1, ws=p, ws_bytes=big, users=p,
           valid=p):
    return lib.rk_als_ssm_grad(users, p, T, S, 0, step, n_users, n_items, p, ldx, p, 8, h, inv_tau, cosine, None, ws,
                               ws_bytes, p, p, p, valid, p, p, p, None)
  assert call(ldx=4) == -2 and "ldx, ldy >= h" in err() and err().startswith("rk_als_ssm_grad: ")
  assert call(h=513, ldx=513) == -2 and "1 <= h <= 512" in err()
  for kw in (dict(T=0), dict(T=4097), dict(S=-1), dict(S=4097)):
    assert call(**kw) == -2 and "1 <= T <= 4096, 0 <= S <= 4096" in err(), kw
  assert call(n_items=0) == -2 and "n_users, n_items >= 1" in err()
  assert call(step=-1) == -2 and "step >= 0" in err()
  for bad in (0.0, -1.0, float("inf"), float("nan")):
    assert call(inv_tau=bad) == -2 and "inv_tau" in err(), bad
  assert call(cosine=2) == -2 and "cosine 0 or 1" in err()
  assert call(ws_bytes=100) == -2 and "workspace too small" in err()
  assert call(ws=None) == -2 and "workspace too small" in err()
  assert call(ws=ctypes.c_void_p(20)) == -2 and "16-byte" in err()
  assert call(valid=None) == -2 and "null pointer" in err()
  assert call(users=None) == -2 and "null pointer" in err()
  # the workspace formula
  for T, S, h in ((0, 0, 8), (ssm.MAX_BATCH + 1, 0, 8), (8, -1, 8), (8, ssm.MAX_NEGATIVES + 1, 8), (8, 0, 0), (8, 0, 513)):
    assert lib.rk_als_ssm_workspace_bytes(T, S, h) == -2 == ssm.grad_workspace_bytes(T, S, h), (T, S, h)
  r256 = lambda x: -(-x // 256) * 256
  for T, S, h in ((1, 0, 1), (300, 70, 65), (ssm.MAX_BATCH, ssm.MAX_NEGATIVES, 512)):
    C = T + S
    want = 2 * r256(4 * T * h) + 2 * r256(4 * C * h) + r256(4 * T * C) + 4 * r256(4 * T) + 3 * r256(4 * C)
    assert lib.rk_als_ssm_workspace_bytes(T, S, h) == ssm.grad_workspace_bytes(T, S, h) == want


# -------------------------------------------------------------------- draws
def test_the_shared_draws_are_a_known_answer_vector_uniform_and_apart_from_the_sampler():
  got = su.shared_draws(11, 3, 12, 7915)
  assert got.dtype == np.int32 and got.tolist() == KNOWN_DRAWS, got.tolist()
  assert su.shared_draws(11, 3, 5, 7915).tolist() == KNOWN_DRAWS[:5]          # (a function of the index, not of S)
  assert su.shared_draws(11, 4, 12, 7915).tolist() != KNOWN_DRAWS and su.shared_draws(12, 3, 12, 7915).tolist() != KNOWN_DRAWS
  assert su.candidates([5, -1, 9], 11, 3, 12, 7915).tolist() == [5, -1, 9] + KNOWN_DRAWS
  # not the sampler's draws of the same (seed, step): another domain of the key
  keys = bpr_util.slot_keys(11, 3, 12)
  assert not np.array_equal(bpr_util.draw(keys, 0, 7915), got) and not np.array_equal(bpr_util.draw(keys, 1, 7915), got)
  n, N = 120, 100000
  d = np.concatenate([su.shared_draws(0, s, 4000, n) for s in range(25)])
  assert len(d) == N and d.min() == 0 and d.max() == n - 1
  counts = np.bincount(d, minlength=n)
  chi2 = float(((counts - N / n) ** 2 / (N / n)).sum())
  print("chi^2 of 1e5 draws over %d items: %.1f (119 degrees of freedom)" % (n, chi2))
  assert chi2 < 119 + 5 * np.sqrt(2 * 119)                    # (mean + 5 standard deviations of chi^2_119)


KNOWN_DRAWS = [2707, 6461, 6992, 2759, 5622, 3925, 1591, 1983, 7512, 6496, 4457, 1006]   # (seed 11, step 3, 7 915 items)


# ----------------------------------------------------------------- gradient
def _case(seed=0, T=12, S=5, h=6, n_users=9, n_items=10):
  """T slots over small tables: slot 1 repeats slot 0's pair (an excluded duplicate column for either), slot 2 holds
  slot 0's user with another item, slot 4 has an invalid user and slot 5 an invalid item; a shared column is made to
  hold slot 3's positive."""
  rng = np.random.RandomState(seed)
  X, Y = rng.randn(n_users, h), rng.randn(n_items, h)
  users, items = rng.randint(0, n_users, T).astype(np.int32), rng.randint(0, n_items, T).astype(np.int32)
  users[1], items[1] = users[0], items[0]
  users[2], items[2] = users[0], (items[0] + 1) % n_items
  users[4], items[5] = -1, n_items
  cand = su.candidates(items, 3, 7, S, n_items)
  cand[T + 1] = items[3]
  corr = (0.7 * rng.randn(n_items)).astype(np.float32)
  return users, items, cand, X, Y, corr


def _torch_rows(users, items, cand, X, Y, temperature, cosine, corr):
  """(loss, dA, dB): the loss over the valid slots by cross_entropy over masked logits, and autograd's gradient
  with respect to the gathered rows A = X[users] and B = Y[cand] (one leaf row per slot and per column)."""
  ok, cvalid, live = su.live_mask(users, items, cand, X.shape[0], Y.shape[0])
  A, B = np.zeros((len(users), X.shape[1])), np.zeros((len(cand), X.shape[1]))
  A[ok], B[cvalid] = X[users[ok]], Y[cand[cvalid]]
  A, B = torch.tensor(A, requires_grad=True), torch.tensor(B, requires_grad=True)
  a, b = (F.normalize(A, dim=-1), F.normalize(B, dim=-1)) if cosine else (A, B)
  logits = a @ b.T * su.inverse_temperature(temperature)
  if corr is not None:
    cc = np.zeros(len(cand))
    cc[cvalid] = np.asarray(corr, np.float64)[cand[cvalid]]
    logits = logits - torch.tensor(cc)[None, :]
  logits = logits.masked_fill(torch.tensor(~live), float("-inf"))
  rows = torch.tensor(np.nonzero(ok)[0])
  loss = F.cross_entropy(logits[rows], rows, reduction="mean")
  dA, dB = torch.autograd.grad(loss, (A, B))
  return loss.item(), dA.numpy(), dB.numpy()


@pytest.mark.parametrize("with_corr", [False, True])
@pytest.mark.parametrize("cosine", [True, False])
def test_the_restated_gradient_rows_equal_autograd_of_cross_entropy(cosine, with_corr):
  users, items, cand, X, Y, corr = _case()
  corr = corr if with_corr else None
  ok, cvalid, live = su.live_mask(users, items, cand, 9, 10)
  assert ok.sum() == 10 and not ok[4] and not ok[5] and not cvalid[4] and cvalid[12:].all()
  assert not live[0, 1] and not live[1, 0] and live[0, 0] and not live[3, 13] and live[2, 0] and not live[:, 4].any()
  want_loss, dA, dB = _torch_rows(users, items, cand, X, Y, 0.3, cosine, corr)
  (loss, prob), m, valid, cv, DU, DC = su.grad_rows(users, items, cand, X, Y, 0.3, cosine, corr)
  scale = max(np.abs(dA).max(), np.abs(dB).max())
  err = max(np.abs(DU - dA).max(), np.abs(DC - dB).max())
  print("cosine %s corr %s: loss %.6f, max |row| %.3g, largest difference / it %.3g" % (cosine, with_corr, loss, scale, err / scale))
  assert m == 10 and scale > 1e-3 and err <= 1e-10 * scale and abs(loss - want_loss) <= 1e-10 * abs(want_loss)
  assert np.array_equal(valid, ok) and np.array_equal(cv, cvalid) and 0 < prob < 1
  assert not DU[4].any() and not DU[5].any() and not DC[4].any() and not DC[5].any()
  assert abs(loss - su.dense_loss(users, items, cand, X, Y, 0.3, cosine, corr)) <= 1e-12 * abs(loss)


def test_the_restated_loss_on_its_edge_cases():
  rng = np.random.RandomState(2)
  X, Y = rng.randn(10, 5), rng.randn(12, 5)
  (l, p), m, valid, cvalid, DU, DC = su.grad_rows([3], [4], [4], X, Y, 0.1)       # one slot, no negative: nothing to learn
  assert m == 1 and l == 0 and p == 1 and not DU.any() and not DC.any()
  (l, p), m, valid, cvalid, DU, DC = su.grad_rows([10, -1, 3], [0, 0, 12], [0, 0, 12, 5], X, Y, 0.1)
  assert m == 0 and (l, p) == (0.0, 0.0) and not valid.any() and cvalid.tolist() == [0, 0, 0, 1] and not DU.any()
  # every slot the same pair: each row's only live column is its own
  (l, p), m, _, _, DU, DC = su.grad_rows([3] * 6, [4] * 6, [4] * 6, X, Y, 0.1)
  assert m == 6 and l == 0 and p == 1 and not DU.any() and not DC.any()
  # a zero row under the cosine: z = 0, its logits are 0 and its own row has no gradient; under the dot product it has
  X[2] = 0
  users, items = np.array([7, 2, 2, 5]), np.array([1, 3, 6, 0])
  cand = np.array([1, 3, 6, 0, 8, 8])
  _, _, _, _, DU, DC = su.grad_rows(users, items, cand, X, Y, 0.5)
  assert not DU[1].any() and not DU[2].any() and DU[0].any() and DC[1].any()
  assert np.array_equal(DC[4], DC[5])                         # (a repeated shared item is a column of its own)
  _, _, _, _, DUd, _ = su.grad_rows(users, items, cand, X, Y, 0.5, cosine=False)
  assert DUd[1].any()
  eps = 1e-6                                                   # (finite differences on one row of either table)
  for cosine in (True, False):
    _, _, _, _, DU, DC = su.grad_rows(users, items, cand, X, Y, 0.5, cosine)
    for V, D, row, slots in ((X, DU, 7, [0]), (Y, DC, 8, [4, 5])):
      for c in range(5):
        old = V[row, c]
        V[row, c] = old + eps
        up = su.dense_loss(users, items, cand, X, Y, 0.5, cosine)
        V[row, c] = old - eps
        down = su.dense_loss(users, items, cand, X, Y, 0.5, cosine)
        V[row, c] = old
        assert abs((up - down) / (2 * eps) - D[slots, c].sum()) <= 1e-6 * max(np.abs(DU).max(), np.abs(DC).max())


def test_the_correction_is_the_log_share_of_the_columns():
  tr, _ = bpr_util.planted()
  from recoder_amd import ssm
  d = np.bincount(tr.indices, minlength=120)
  for T, S, w in ((256, 64, 1.0), (256, 0, 0.5), (1, 4096, 2.0)):
    corr = su.correction(tr, T, S, w)
    assert corr.dtype == np.float32 and np.array_equal(corr, ssm.correction(d, T, S, w))
    q = (T * d / tr.nnz + S / 120.0) / (T + S)
    assert abs(q.sum() - 1) < 1e-12
    live = q > 0
    assert np.array_equal(corr[live], (w * np.log(q[live])).astype(np.float32)) and not corr[~live].any()
  assert np.all(su.correction(tr, 256, 0, 1.0)[d == 0] == 0)


def test_the_float32_restatement_stays_beside_float64():
  tr, _ = bpr_util.planted()
  rng = np.random.RandomState(4)
  Eu, Ei = (0.3 * rng.randn(200, 8)).astype(np.float32), (0.3 * rng.randn(120, 8)).astype(np.float32)
  users, pos, _ = bpr_util.sample(tr, 1, 0, 64)
  cand = su.candidates(pos, 1, 0, 16, 120)
  corr = su.correction(tr, 64, 16, 1.0)
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  l64, c64 = su.step(tr, s64, 2, users, pos, cand, 0.05, 1e-3, 0.2, True, corr)
  l32, c32 = su.step(tr, s32, 2, users, pos, cand, 0.05, 1e-3, 0.2, True, corr, np.float32)
  assert c64 == c32 == 64 and np.allclose(l64, l32, rtol=0, atol=1e-4)
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      assert s32[key][side].dtype == np.float32 and np.abs(s32[key][side] - s64[key][side]).max() < 1e-4


# ------------------------------------------------------------------ memory
def test_required_bytes_adds_the_workspace_the_candidates_and_two_sorts_to_lightgcn():
  from recoder_amd import lightgcn, ssm
  base = (1000, 500, 64, 20000, 256)
  need = ssm.required_bytes(*base, num_negatives=100)
  C = 356
  assert need == lightgcn.required_bytes(*base) + ssm.grad_workspace_bytes(256, 100, 64) + C * 64 * 4 + 2 * C * 4 + \
      500 * 4 + 12 + 2 * (256 + C) * 16
  assert ssm.required_bytes(*base, num_negatives=101) > need > ssm.required_bytes(*base)
  assert ssm.required_bytes(*base, num_negatives=100, allocate_state=False) == need - 3 * 1500 * 64 * 4
  assert ssm.check_memory(*base, num_negatives=100, free_bytes=1 << 30) == need
  with pytest.raises(ValueError, match="SSM needs 1 <= batch_size <= 4096 and 1 <= h <= 512 \\(got 4097, 64\\)"):
    ssm.check_memory(10, 10, 64, 10, 4097, free_bytes=1 << 30)
  with pytest.raises(ValueError, match="SSM over 1000 users x 500 items at h = 64 with 20000 entries and batches "
                                       "of 256 needs %d bytes of device memory, 1000 are free" % need):
    ssm.check_memory(*base, num_negatives=100, free_bytes=1000)
  assert ssm.check_data(1000, 10, 5, 256) == 4
  with pytest.raises(ValueError, match="train_ssm needs at least one stored entry"):
    ssm.check_data(0, 10, 1, 256)


# ------------------------------------------------------------------ refusals
def _no_gpu(monkeypatch):
  import recoder_amd.ssm  # noqa: F401
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
  return not rec._Recoder__model_initialized and rec.ssm_state is None and rec.ssm_history == [] and \
      rec.lightgcn_state is None and rec.directau_state is None and rec.optimizer is None


def test_train_ssm_exists_with_the_signature_of_the_contract():
  from recoder_amd.model import Recoder
  sig = inspect.signature(Recoder.train_ssm)
  assert list(sig.parameters) == ["self", "train_dataset", "num_layers", "num_epochs", "batch_size", "lr", "reg",
                                  "temperature", "num_negatives", "similarity", "logq_weight", "normalize", "seed",
                                  "resume"]
  d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
  assert d == dict(DEFAULTS, similarity="cosine", logq_weight=0.0, normalize=False, seed=0, resume=False)
  rec = Recoder(model=_mf(4))
  assert rec.ssm_state is None and rec.ssm_history == []


def test_check_config_accepts_the_contract_and_no_layer():
  from recoder_amd import ssm
  assert ssm.check_config(_mf(4), 2, 3, 256, 0.01, 1e-4, 0.5, 7, "dot", 1.0, 1, 0) == \
      (2, 3, 256, 0.01, 1e-4, 0.5, 7, "dot", 1.0, True, 0)
  assert ssm.check_config(_mf(512), np.int64(0), 0, ssm.MAX_BATCH, np.float32(0.5), 0, np.float32(0.25), ssm.MAX_NEGATIVES,
                          "cosine", 0, False, -7) == (0, 0, 4096, 0.5, 0.0, 0.25, 4096, "cosine", 0.0, False, -7)
  assert ssm.MAX_BATCH == 4096 and ssm.MAX_NEGATIVES == 4096


def test_train_ssm_refuses_before_any_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  _no_gpu(monkeypatch)
  cases = [
    (DynamicAutoencoder(hidden_layers=[8]), {}, "train_ssm trains a MatrixFactorization, not DynamicAutoencoder"),
    (ShallowAutoencoder(), {}, "train_ssm trains a MatrixFactorization, not ShallowAutoencoder"),
    (_mf(4, activation_type="tanh"), {}, "train_ssm needs activation_type='none' \\(got 'tanh'\\)"),
    (_mf(4, dropout_prob=0.5), {}, "train_ssm needs dropout_prob == 0"),
    (_mf(0), {}, "train_ssm supports embedding sizes 1..512 \\(got 0\\)"),
    (_mf(513), {}, "train_ssm supports embedding sizes 1..512 \\(got 513\\)"),
    (_mf(4), {"num_layers": -1}, "num_layers must be an integer in 0..8 \\(got -1\\)"),
    (_mf(4), {"num_layers": 9}, "num_layers must be an integer in 0..8 \\(got 9\\)"),
    (_mf(4), {"lr": 0}, "lr must be finite and > 0"),
    (_mf(4), {"reg": -1e-9}, "reg must be finite and >= 0"),
    (_mf(4), {"batch_size": 0}, "batch_size must be an integer in 1..4096 \\(got 0\\)"),
    (_mf(4), {"batch_size": 4097}, "batch_size must be an integer in 1..4096 \\(got 4097\\)"),
    (_mf(4), {"num_epochs": -1}, "num_epochs must be an integer >= 0"),
    (_mf(4), {"num_negatives": -1}, "num_negatives must be an integer in 0..4096 \\(got -1\\)"),
    (_mf(4), {"num_negatives": 4097}, "num_negatives must be an integer in 0..4096 \\(got 4097\\)"),
    (_mf(4), {"num_negatives": 8.0}, "num_negatives must be an integer in 0..4096"),
    (_mf(4), {"temperature": 0}, "temperature must be finite and > 0"),
    (_mf(4), {"temperature": -0.1}, "temperature must be finite and > 0"),
    (_mf(4), {"temperature": float("inf")}, "temperature must be finite and > 0"),
    (_mf(4), {"temperature": float("nan")}, "temperature must be finite and > 0"),
    (_mf(4), {"temperature": 1e-320}, "temperature must be finite and > 0"),
    (_mf(4), {"logq_weight": -0.5}, "logq_weight must be finite and >= 0"),
    (_mf(4), {"logq_weight": float("inf")}, "logq_weight must be finite and >= 0"),
    (_mf(4), {"similarity": "euclid"}, "similarity must be one of 'cosine', 'dot' \\(got 'euclid'\\)"),
    (_mf(4), {"similarity": None}, "similarity must be one of"),
    (_mf(4), {"seed": True}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"seed": 2 ** 63}, "seed must be an integer that fits 64 bits"),
    (_mf(4), {"resume": True}, "resume=True needs the state of an earlier train_ssm"),
  ]
  for model, kw, message in cases:
    rec = Recoder(model=model)
    with pytest.raises(ValueError, match=message):
      rec.train_ssm(_dataset(), **kw)
    assert _uninitialised(rec), message
  from recoder_amd import ssm
  state = {"num_layers": 2, "E0": (torch.zeros(40, 4), torch.zeros(40, 4))}
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 0\\)"):
    ssm.check_resume(state, 0)
  with pytest.raises(ValueError, match="do not match the model's"):
    ssm.check_resume(state, 2, ((40, 4), (41, 4)))
  ssm.check_resume(state, 2, ((40, 4), (40, 4)))
  rec = Recoder(model=_mf(4))                                  # (another method's state is not this one's)
  rec.lightgcn_state = rec.directau_state = state
  with pytest.raises(ValueError, match="resume=True needs the state of an earlier train_ssm"):
    rec.train_ssm(_dataset(), resume=True)


def test_train_ssm_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="train_ssm runs on one GPU"):
    rec.train_ssm(_dataset())
  assert _uninitialised(rec)


# ------------------------------------------------------------------ quality
def test_the_float64_restatement_at_the_defaults_ranks_above_popularity_on_the_planted_matrix():
  """The condition tests/test_ssm.py asserts of the kernels, met by the reference alone: the defaults of
  ``Recoder.train_ssm`` (h = 16, the start of tests/test_ssm.py) on ``bpr_util.planted()``."""
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)[:2]
  d = DEFAULTS
  P, Q, _, hist = su.fit(tr, *start, d["num_layers"], d["num_epochs"], d["batch_size"], d["lr"], d["reg"],
                         d["temperature"], d["num_negatives"], seed=0)
  got, pop = su.recall_at(P, Q, tr, ho), su.popularity_recall(tr, ho)
  cos = su.recall_at(su.unit_rows(P), su.unit_rows(Q), tr, ho)
  print("planted: Recall@20 of the float64 restatement %.4f (ranked by the cosine %.4f), popularity %.4f, untrained "
        "%.4f; history %s" % (got, cos, pop, su.recall_at(*start, tr, ho), hist))
  assert hist[-1][0] < hist[0][0] and got > pop
