"""CPU: the built library's rk_als_ncf_* names and argument checks, its host-arithmetic queries against their Python
restatements (also at the limits), what train_ncf and the model refuse before any GPU work, and the pin of the numpy
restatement (tests/ncf_util.py): its gradients against central finite differences in float64, ``torch_forward`` against
its score, the float32 restatement's own error, and a checkpoint round trip of the model on the host."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import ncf_util as nu
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

NEW = ["rk_als_ncf_dense_adam", "rk_als_ncf_dense_count", "rk_als_ncf_item_part", "rk_als_ncf_lds_bytes",
       "rk_als_ncf_scores", "rk_als_ncf_step", "rk_als_ncf_workspace_bytes"]
LARGEST_L3 = nu.LARGEST_L3                                    # (among dg = dm = 128 and three equal widths)


def test_the_library_exports_exactly_the_declared_ncf_names(built):
  from recoder_amd import _als_lib
  assert [s for s in exports(built.ALS_LIB) if s.startswith("rk_als_ncf_")] == NEW
  header = os.path.join(INC, "recoder_als.h")
  assert sorted(n for n in declared([header]) if n.startswith("rk_als_ncf_")) == NEW
  assert all(name in _als_lib.SIGNATURES for name in NEW)
  lib = _als_lib.load()
  assert all(hasattr(lib, name) for name in NEW)


def test_the_library_checks_its_arguments_before_any_launch(built):
  from recoder_amd import _als_lib
  lib = _als_lib.load()
  p = ctypes.c_void_p(16)                                    # (never dereferenced: the checks come first)
  err = lambda: lib.rk_als_last_error().decode()

  def step(T=8, R=4, step=0, n_items=5, ldpg=8, ldqm=8, dims=(8, 8, 2, 8, 4, 0), users=p, slabs=p):
    return lib.rk_als_ncf_step(users, p, T, R, 0, step, 5, n_items, p, ldpg, p, 8, p, 8, p, ldqm, p, *dims, p, p, p, p,
                               slabs, None)
  assert step(ldpg=4) == -2 and "ldpg, ldqg >= dg" in err() and err().startswith("rk_als_ncf_step: ")
  assert step(ldqm=4) == -2 and "ldpm, ldqm >= dm" in err()
  for dims in ((8, 8, 0, 8, 4, 0), (8, 8, 4, 8, 4, 4), (6, 8, 1, 8, 0, 0), (8, 132, 1, 8, 0, 0), (8, 8, 2, 8, 2, 0),
               (128, 128, 3, 128, 128, 128)):
    assert step(dims=dims) == -2 and "1 <= L <= 3" in err(), dims
  for kw in (dict(T=0), dict(T=4097), dict(R=0), dict(R=1025), dict(T=4096, R=1024)):
    assert step(**kw) == -2 and "T (1 + R) <= 2^22" in err(), kw
  assert step(n_items=0) == -2 and "n_users, n_items >= 1" in err()
  assert step(step=-1) == -2 and "step >= 0" in err()
  assert step(users=None) == -2 and "null pointer" in err()
  assert step(slabs=None) == -2 and "null pointer" in err()

  def adam(tiles=2, entries=40, t=1, reg=0.0, beta1=0.9, loss=p):
    return lib.rk_als_ncf_dense_adam(p, p, p, p, tiles, entries, 8, 8, 2, 8, 4, 0, 0.1, reg, beta1, 0.999, 1e-8, t,
                                     loss, None)
  assert adam(tiles=3) == -2 and "tiles = ceil(entries / 32)" in err() and err().startswith("rk_als_ncf_dense_adam: ")
  assert adam(entries=0, tiles=0) == -2 and "1 <= entries" in err()
  assert adam(t=0) == -2 and "t >= 1" in err()
  assert adam(reg=-1.0) == -2 and "reg finite and >= 0" in err()
  assert adam(beta1=1.0) == -2 and "0 <= beta1, beta2 < 1" in err()
  assert adam(loss=None) == -2 and "null pointer" in err()

  def part(ld=8, dm=8, d1=8, n=5, A=p):
    return lib.rk_als_ncf_item_part(p, ld, n, p, dm, d1, A, None)
  assert part(ld=4) == -2 and "ldqm >= dm" in err() and err().startswith("rk_als_ncf_item_part: ")
  assert part(d1=6) == -2 and part(n=0) == -2 and "n_items >= 1" in err()
  assert part(A=None) == -2 and "null pointer" in err()

  def scores(B=3, lo=0, hi=5, n_items=5, ld=5, ldpm=8, out=p):
    return lib.rk_als_ncf_scores(p, B, 5, lo, hi, n_items, p, 8, p, 8, p, ldpm, p, p, 8, 8, 2, 8, 4, 0, p, out, ld, None)
  assert scores(B=0) == -2 and "1 <= B" in err() and err().startswith("rk_als_ncf_scores: ")
  for kw in (dict(lo=-1), dict(lo=5), dict(hi=6), dict(ld=4)):
    assert scores(**kw) == -2 and "0 <= lo < hi <= n_items, ld >= hi - lo" in err(), kw
  assert scores(ldpm=4) == -2 and "ldpm >= dm" in err()
  assert scores(out=None) == -2 and "null pointer" in err()


def test_the_queries_equal_their_restatements_also_at_the_limits(built):
  from recoder_amd import _als_lib, ncf
  lib = _als_lib.load()
  wide3 = (128, 128, (128, 128, 128))
  for sizes in (nu.SMALL, nu.MID, nu.WIDE, (32, 32, (64, 32, 16)), LARGEST_L3, wide3, (4, 128, (128, 4))):
    d = ncf.dims(sizes)
    assert lib.rk_als_ncf_dense_count(*d) == ncf.layout(sizes)[3] == len(nu.weight_mask(sizes))
    assert lib.rk_als_ncf_lds_bytes(*d, 0) == ncf.lds_bytes(sizes)
    assert lib.rk_als_ncf_lds_bytes(*d, 1) == ncf.lds_bytes(sizes, True)
    for T, R in ((1, 1), (65, 4), (4096, 1023), (4092, 1024)):
      assert lib.rk_als_ncf_workspace_bytes(T, R, *d) == ncf.workspace_bytes(T, R, sizes) > 0
    for T, R in ((0, 1), (4097, 1), (8, 0), (8, 1025), (4093, 1024)):
      assert lib.rk_als_ncf_workspace_bytes(T, R, *d) == -2 == ncf.workspace_bytes(T, R, sizes)
  for d in ((8, 8, 0, 8, 0, 0), (8, 8, 4, 8, 8, 8), (8, 8, 1, 132, 0, 0), (8, 8, 1, 6, 0, 0), (0, 8, 1, 8, 0, 0)):
    assert lib.rk_als_ncf_dense_count(*d) == lib.rk_als_ncf_lds_bytes(*d, 0) == lib.rk_als_ncf_workspace_bytes(8, 1, *d) == -2
  # the limit: the widest single layer fits, LARGEST_L3 fits and its next width does not, and the kernels refuse it
  need = lambda s: max(ncf.lds_bytes(s), ncf.lds_bytes(s, True))
  assert need(nu.WIDE) <= ncf.LDS_LIMIT == 160 * 1024 and need(LARGEST_L3) <= ncf.LDS_LIMIT
  first_out = (128, 128, (80, 80, 80))
  assert need(first_out) > ncf.LDS_LIMIT and need(wide3) > ncf.LDS_LIMIT
  assert ncf.check_sizes(*LARGEST_L3) == LARGEST_L3
  with pytest.raises(ValueError, match="bytes of LDS"):
    ncf.check_sizes(*first_out)
  p = ctypes.c_void_p(16)
  assert lib.rk_als_ncf_step(p, p, 8, 1, 0, 0, 5, 5, p, 128, p, 128, p, 128, p, 128, p, *ncf.dims(first_out), p, p, p,
                             p, p, None) == -2 and "must fit the LDS" in lib.rk_als_last_error().decode()


# ------------------------------------------------------------ configuration
def _dataset(n_users=6, n_items=9):
  from recoder_amd.data import RecommendationDataset
  m = sp.csr_matrix((np.random.RandomState(0).rand(n_users, n_items) < 0.4).astype(np.float32))
  ds = RecommendationDataset.__new__(RecommendationDataset)
  ds.interactions_matrix, ds.users, ds.items = m, np.arange(n_users), np.arange(n_items)
  return ds


@pytest.fixture
def no_gpu(monkeypatch):
  from recoder_amd import model as model_mod

  def refuse():
    raise AssertionError("GPU work was reached")
  monkeypatch.setattr(model_mod, "require_gpu", refuse)


@pytest.mark.parametrize("kw,match", [
    (dict(mlp_layers=()), "1..3 layer widths"), (dict(mlp_layers=(8, 8, 8, 8)), "1..3 layer widths"),
    (dict(mlp_layers=(8, 6)), "multiple of 4"), (dict(mlp_layers=(132,)), "multiple of 4"),
    (dict(embedding_size=2), "embedding_size"), (dict(mlp_embedding_size=130), "mlp_embedding_size"),
    (dict(embedding_size=128, mlp_embedding_size=128, mlp_layers=(128, 128, 128)), "bytes of LDS")])
def test_the_model_refuses_bad_sizes(kw, match):
  from recoder_amd.nn import NeuralMatrixFactorization
  with pytest.raises(ValueError, match=match):
    NeuralMatrixFactorization(**kw)
  m = NeuralMatrixFactorization()
  for k, v in kw.items():
    setattr(m, k, v)
  with pytest.raises(ValueError, match=match):
    m.init_model(5, 5)


@pytest.mark.parametrize("kw,match", [
    (dict(num_negatives=0), "num_negatives"), (dict(num_negatives=1025), "num_negatives"),
    (dict(batch_size=0), "batch_size"), (dict(batch_size=4097), "batch_size"), (dict(lr=0.0), "lr"),
    (dict(lr=float("nan")), "lr"), (dict(reg=-1.0), "reg"), (dict(seed=2 ** 63), "seed"), (dict(seed=1.5), "seed"),
    (dict(num_epochs=-1), "num_epochs"), (dict(batch_size=4096, num_negatives=1024), "at most 4194304"),
    (dict(resume=True), "resume=True needs the state")])
def test_train_ncf_refuses_bad_configurations_before_any_gpu_work(no_gpu, kw, match):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import NeuralMatrixFactorization
  rec = Recoder(NeuralMatrixFactorization(8, 8, (8,)), use_cuda=True, user_based=True)
  with pytest.raises(ValueError, match=match):
    rec.train_ncf(_dataset(), **kw)
  assert rec.ncf_state is None and rec.ncf_history == []


def test_train_ncf_refuses_other_models_and_two_ranks(no_gpu, monkeypatch):
  from recoder_amd import als
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization, NeuralMatrixFactorization
  with pytest.raises(ValueError, match="train_ncf trains a NeuralMatrixFactorization, not MatrixFactorization"):
    Recoder(MatrixFactorization(8), use_cuda=True, user_based=True).train_ncf(_dataset())
  rec = Recoder(NeuralMatrixFactorization(8, 8, (8,)), use_cuda=True, user_based=True)

  def two_ranks(message):
    raise NotImplementedError(message)
  monkeypatch.setattr(als, "check_not_distributed", two_ranks)
  with pytest.raises(ValueError, match="train_ncf runs on one GPU"):
    rec.train_ncf(_dataset())
  with pytest.raises(ValueError, match="fold_in serves a MatrixFactorization, not NeuralMatrixFactorization"):
    rec.fold_in(_dataset().interactions_matrix)


def test_train_points_at_train_ncf(no_gpu):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import NeuralMatrixFactorization
  rec = Recoder(NeuralMatrixFactorization(), use_cuda=True, user_based=True)
  with pytest.raises(ValueError, match=r"call train_ncf\(train_dataset\)"):
    rec.train(_dataset())


# -------------------------------------------------------------- restatement
def _case(sizes, T=5, R=3, seed=2):
  p = nu.params(sizes, 7, 11, seed)
  rng = np.random.RandomState(seed)
  users, pos = rng.randint(0, 7, T).astype(np.int32), rng.randint(0, 11, T).astype(np.int32)
  negs = nu.draws(3, 0, T, R, 11)
  users[1], negs[0, 1] = users[0], pos[0]                      # (a repeated user; the positive drawn as a negative)
  return p, users, pos, negs


@pytest.mark.parametrize("sizes", [nu.SMALL, nu.MID])
def test_the_restatements_gradients_equal_finite_differences(sizes):
  p32, users, pos, negs = _case(sizes)
  p = nu.cast(p32, np.float64)
  r = nu.step_grads(p, users, pos, negs)
  assert abs(r["loss"] - nu.loss_only(p, users, pos, negs)) <= 1e-12 * abs(r["loss"])
  th, eps = nu.theta(p), 1e-6
  rng = np.random.RandomState(0)
  for x in rng.choice(len(th), min(len(th), 40), replace=False):
    up, dn = th.copy(), th.copy()
    up[x] += eps
    dn[x] -= eps
    fd = (nu.loss_only(nu.unpack(p, up), users, pos, negs) - nu.loss_only(nu.unpack(p, dn), users, pos, negs)) / (2 * eps)
    assert abs(fd - r["dtheta"][x]) <= 1e-6 * max(1.0, abs(fd)), (x, fd, r["dtheta"][x])
  dg = sizes[0]
  for name, rows, key, col0 in (("Pg", r["GU"], r["u"], 0), ("Pm", r["GU"], r["u"], dg), ("Qg", r["GI"], r["i"], 0),
                                ("Qm", r["GI"], r["i"], dg)):
    G = np.zeros_like(p[name])
    np.add.at(G, key, rows[:, col0:col0 + p[name].shape[1]])
    for _ in range(6):
      a, b = rng.randint(p[name].shape[0]), rng.randint(p[name].shape[1])
      q = dict(p)
      vals = []
      for sgn in (1, -1):
        q[name] = p[name].copy()
        q[name][a, b] += sgn * eps
        vals.append(nu.loss_only(q, users, pos, negs))
      fd = (vals[0] - vals[1]) / (2 * eps)
      assert abs(fd - G[a, b]) <= 1e-6 * max(1.0, abs(fd)), (name, a, b)


def test_torch_forward_and_a_checkpoint_round_trip_on_the_host(tmp_path):
  from recoder_amd import ncf
  from recoder_amd.nn import NeuralMatrixFactorization
  m = NeuralMatrixFactorization(*nu.MID)
  m.init_seed = 5
  m.init_model(11, 7)
  assert abs(float(m.Pg.std()) - 0.01) < 0.003 and not m.b0.any() and not any(c.any() for c in m.mlp_biases)
  again = NeuralMatrixFactorization(*nu.MID)
  again.init_seed = 5
  again.init_model(11, 7)
  assert all(torch.equal(a, b) for a, b in zip(m.parameters(), again.parameters()))
  p = nu.params(nu.MID, 7, 11, 3)
  U = torch.tensor(np.concatenate([p["Pg"], p["Pm"]], 1))
  I = torch.tensor(np.concatenate([p["Qg"], p["Qm"]], 1))
  ncf.unpack(m, U, I, torch.tensor(nu.theta(p)))
  assert torch.equal(ncf.pack(m)[2], torch.tensor(nu.theta(p)))
  users = torch.tensor([3, 0, 3, 6])
  want = nu.scores(nu.cast(p, np.float64), users.numpy(), 0, 11)
  got = m.double().torch_forward(None, input_users=users).detach().numpy()
  assert nu.rel(got, want) <= 1e-12
  sub = m.torch_forward(None, input_users=users, target_items=torch.tensor([4, 1])).detach().numpy()
  assert nu.rel(sub, want[:, [4, 1]]) <= 1e-12
  m = m.float()
  path = str(tmp_path / "ncf.model")
  torch.save({"model_params": m.model_params(), "model": m.state_dict()}, path)
  st = torch.load(path, weights_only=False)
  fresh = NeuralMatrixFactorization()
  fresh.load_model_params(st["model_params"])
  assert fresh.sizes() == nu.MID
  fresh.init_model(11, 7)
  fresh.load_state_dict(st["model"])
  assert torch.equal(fresh.forward(None, input_users=users), m.forward(None, input_users=users))


def test_the_float32_restatements_own_error_is_what_the_bounds_assume():
  """The f32 restatement's error against float64 on the GPU cases' kind of inputs: 4 x these is what tests/test_ncf.py
  allows.  Measured here from the restatement alone: scores 1.0e-07 .. 4.4e-07, step sums up to 1.2e-06."""
  for sizes in (nu.SMALL, nu.MID):
    p32, users, pos, negs = _case(sizes, T=65, R=4)
    p64 = nu.cast(p32, np.float64)
    e = nu.rel(nu.scores(p32, np.arange(7), 0, 11), nu.scores(p64, np.arange(7), 0, 11))
    assert 2.0 ** -26 <= e <= 2e-6, e
    r32, r64 = nu.step_grads(p32, users, pos, negs), nu.step_grads(p64, users, pos, negs)
    for k in ("loss", "GU", "GI", "dtheta"):
      assert nu.rel(r32[k], r64[k]) <= 5e-6, (sizes, k, nu.rel(r32[k], r64[k]))
