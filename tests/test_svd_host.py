"""CPU: what train_svd and svd.check_config refuse before any GPU work, and the numpy restatement's own
pins (tests/svd_util.py): against scipy's svds on a planted matrix, and, on the ML-20M slice, that the
inputs of the GPU test are well chosen (the float32 restatement stays close to the float64 one there) and
that PureSVD beats popularity by a clear margin."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg
import torch

from tests import svd_util


def _no_gpu(monkeypatch):
  import recoder_amd.svd  # noqa: F401
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


def test_check_config_accepts_the_contract():
  from recoder_amd import svd
  assert svd.check_config(_mf(4), 16, 6, 0) == (4, 20)
  assert svd.check_config(_mf(200), 16, 0, -3) == (200, 216)
  assert svd.check_config(_mf(512), 0, np.int64(2), np.int64(5)) == (512, 512)


def test_check_config_rejects_each_bad_argument():
  from recoder_amd import svd
  from recoder_amd.nn import DynamicAutoencoder, ShallowAutoencoder
  for model in (DynamicAutoencoder(hidden_layers=[8]), ShallowAutoencoder()):
    with pytest.raises(ValueError, match="MatrixFactorization"):
      svd.check_config(model, 16, 6, 0)
  with pytest.raises(ValueError, match="activation_type"):
    svd.check_config(_mf(4, activation_type="tanh"), 16, 6, 0)
  with pytest.raises(ValueError, match="dropout_prob"):
    svd.check_config(_mf(4, dropout_prob=0.5), 16, 6, 0)
  for h in (0, -1, 2.0):
    with pytest.raises(ValueError, match="embedding size"):
      svd.check_config(_mf(h), 16, 6, 0)
  for oversample in (-1, 1.5, None, True):
    with pytest.raises(ValueError, match="oversample"):
      svd.check_config(_mf(4), oversample, 6, 0)
  with pytest.raises(ValueError, match="at most 512"):
    svd.check_config(_mf(500), 13, 6, 0)
  for q in (-1, 2.0, None, True):
    with pytest.raises(ValueError, match="num_power_iterations"):
      svd.check_config(_mf(4), 16, q, 0)
  for seed in (1.0, None, "0"):
    with pytest.raises(ValueError, match="seed"):
      svd.check_config(_mf(4), 16, 6, seed)


def test_train_svd_rejects_bad_arguments_before_gpu_work(monkeypatch):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  _no_gpu(monkeypatch)
  with pytest.raises(ValueError, match="MatrixFactorization"):
    Recoder(model=ShallowAutoencoder()).train_svd(_dataset())
  with pytest.raises(ValueError, match="oversample"):
    Recoder(model=_mf(4)).train_svd(_dataset(), oversample=-2)
  with pytest.raises(ValueError, match="num_power_iterations"):
    Recoder(model=_mf(4)).train_svd(_dataset(), num_power_iterations=1.5)
  rec = Recoder(model=_mf(4))
  with pytest.raises(ValueError, match="seed"):
    rec.train_svd(_dataset(), seed=0.5)
  assert rec.model.bias is None and rec.svd_info is None


def test_train_svd_rejects_a_sketch_wider_than_the_matrix(monkeypatch):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_mf(30))
  with pytest.raises(ValueError, match=r"= 46 exceeds min\(users, items\) = 40"):
    rec.train_svd(_dataset(40))                       # l = 30 + 16 > 40
  assert rec.model.bias is None
  from recoder_amd.data import RecommendationDataset
  wide = RecommendationDataset(sp.csr_matrix(np.ones((10, 100), np.float32)))
  with pytest.raises(ValueError, match=r"= 20 exceeds min\(users, items\) = 10"):
    Recoder(model=_mf(4)).train_svd(wide)


def test_train_svd_is_single_gpu(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError, match="train_svd"):
    Recoder(model=_mf(4)).train_svd(_dataset())


def test_memory_check_raises_without_touching_a_device(monkeypatch):
  from recoder_amd import svd
  _no_gpu(monkeypatch)
  need = svd.required_bytes(138000, 20108, 80, 10 ** 7)
  assert need == 2 * (138000 + 20108) * 80 * 4 + 2 * 10 ** 7 * 8 + (138000 + 20108 + 2) * 8
  assert svd.required_bytes(10, 10, 216, 0) - svd.required_bytes(10, 10, 216, 0, with_data=False) == 0
  assert svd.required_bytes(10, 10, 216, 5) - svd.required_bytes(10, 10, 216, 5, with_data=False) == 40
  with pytest.raises(ValueError) as e:
    svd.check_memory(10 ** 9, 10 ** 6, 512, 0)
  assert "1000000000" in str(e.value) and "one device" in str(e.value)
  with pytest.raises(ValueError) as e:
    svd.check_memory(138000, 20108, 80, 10 ** 7, free_bytes=2 ** 20)
  assert str(need) in str(e.value)
  assert svd.check_memory(138000, 20108, 80, 10 ** 7, free_bytes=2 ** 32) == need


def test_eig_host_sign_rule_and_order():
  from recoder_amd import svd
  rng = np.random.RandomState(0)
  W = rng.randn(50, 7) * np.array([9, 1, 5, 3, 7, 2, 4.0])[None, :]
  sigma, S = svd.eig_host((W.T @ W).astype(np.float32), 4)
  assert sigma.shape == (4,) and S.shape == (7, 4) and np.all(np.diff(sigma) < 0)
  want = np.linalg.svd(W.astype(np.float64), compute_uv=False)[:4]
  assert np.abs(sigma - want).max() <= 1e-5 * want[0]
  big = np.abs(S).argmax(axis=0)
  assert np.all(S[big, np.arange(4)] > 0)
  assert np.abs(S.T @ S - np.eye(4)).max() <= 1e-12
  np.testing.assert_array_equal(S, svd_util.fix_signs(-S))


# ------------------------------------------------------- the restatement's own pins
def test_restatement_against_svds_on_the_planted_matrix():
  A = svd_util.planted()
  assert A.shape == (600, 400)
  want = np.sort(scipy.sparse.linalg.svds(A.astype(np.float64), k=9, return_singular_vectors=False))[::-1]
  assert want[7] > 2.5 * want[8], "the planted gap"
  sigma, V, U = svd_util.rsvd(A, 8, 16, 4, svd_util.omega(400, 24, 0), np.float64)
  rel = np.abs(sigma - want[:8]) / want[:8]
  print("planted: sigma %s, sigma_9 %.3f, max rel err vs svds %.3g" % (np.round(sigma, 3), want[8], rel.max()))
  assert rel.max() <= 1e-5
  assert np.abs(V.T @ V - np.eye(8)).max() <= 1e-12
  assert np.linalg.norm(U - A.astype(np.float64) @ V) <= 1e-10 * np.linalg.norm(U)


@pytest.fixture(scope="module")
def slice_runs():
  """{(h, q): (float64 result, float32 result)} on the slice with the Omega the GPU test injects."""
  x, y = svd_util.load_slice()
  out = {}
  for h, q in ((4, 6), (64, 6)):
    om = svd_util.omega(x.shape[1], h + 16, 0)
    out[(h, q)] = (svd_util.rsvd(x, h, 16, q, om, np.float64), svd_util.rsvd(x, h, 16, q, om, np.float32))
  return x, y, out


@pytest.mark.parametrize("h,q", [(4, 6), (64, 6)])
def test_gpu_test_inputs_are_well_chosen(slice_runs, h, q):
  """The float32 restatement stays close to the float64 one on the slice at the parameters tests/test_svd.py
  uses: a device result held to a small multiple of the float32 one is then held to something small."""
  x, y, runs = slice_runs
  r64, r32 = runs[(h, q)]
  st = svd_util.stats(x, r32, r64)
  l64 = svd_util.top_k(svd_util.scores(r64), x, 20)
  l32 = svd_util.top_k(svd_util.scores(r32), x, 20)
  differ = svd_util.top20_differ(l32, l64)
  rec64, rec32 = svd_util.recall_at(l64, y), svd_util.recall_at(l32, y)
  print("slice h=%d q=%d float32 vs float64: %s, top-20 differ %.4f %%, Recall@20 %.6f vs %.6f"
        % (h, q, {k: "%.3g" % v for k, v in st.items()}, 100 * differ, rec32, rec64))
  assert st["e_sub"] <= 1e-4
  assert differ <= 1e-3
  assert abs(rec32 - rec64) <= 1e-4


def test_puresvd_beats_popularity_on_the_slice(slice_runs):
  x, y, runs = slice_runs
  r64, _ = runs[(4, 6)]
  rec = svd_util.recall_at(svd_util.top_k(svd_util.scores(r64), x, 20), y)
  pop = svd_util.popularity_recall(x, y)
  print("slice Recall@20: PureSVD h=4 q=6 float64 %.4f, popularity %.4f" % (rec, pop))
  assert rec >= pop + 0.01
