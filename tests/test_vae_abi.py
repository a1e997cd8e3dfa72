"""CPU: librecoder_vae.so is built beside the other three libraries and exports exactly what
include/recoder_vae.h declares (each bound in _vae_lib.SIGNATURES); the other libraries' exports are
unchanged; VariationalAutoencoder and Recoder reject what the fused VAE step does not cover before any GPU
work; model_params round-trips; the float64 restatement the GPU tests use is itself consistent."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import vae_util
from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAE_HEADER = os.path.join(ROOT, "include", "recoder_vae.h")


def test_vae_library_exports_exactly_its_header(built):
  from recoder_amd import _vae_lib
  assert os.path.exists(built.VAE_LIB)
  assert declared([VAE_HEADER]) == ["rk_vae_last_error", "rk_vae_sample", "rk_vae_sample_bwd", "rk_vae_version"]
  lib = _vae_lib.load()
  # argument checks are host-side: no device needed
  assert lib.rk_vae_sample(None, 4, 8, 0, None, 0, 0, None, 0, None, 0, None, 0.0, None, None, None, None) == -2
  assert b"required" in lib.rk_vae_last_error()
  assert lib.rk_vae_sample_bwd(None, None, None, 4, 0, 1.0, None, 0, None, 0.0, None, None) == -2


def test_no_new_header_under_csrc():
  """Every csrc/*.h is a dependency of the training library (build.py, test_abi.py)."""
  csrc = os.path.join(ROOT, "recoder_amd", "csrc")
  hs = sorted(f for f in os.listdir(csrc) if f.endswith(".h"))
  assert not any("vae" in h for h in hs), hs


# ------------------------------------------------------------------ validation
def _vae(**kw):
  from recoder_amd.nn import VariationalAutoencoder
  args = dict(hidden_layers=[16, 8], activation_type="tanh", noise_prob=0.5, kl_cap=0.2, anneal_steps=10)
  args.update(kw)
  return VariationalAutoencoder(**args)


@pytest.mark.parametrize("kw", [
  dict(hidden_layers=[16]), dict(hidden_layers=[]), dict(kl_cap=-0.1), dict(anneal_steps=-1),
  dict(activation_type="softplus"), dict(activation_type="nope"), dict(hidden_layers=[18, 8]),
  dict(noise_prob=1.0),
])
def test_constructor_rejects(kw):
  with pytest.raises(ValueError):
    _vae(**kw)


def _dataset():
  from recoder_amd.data import RecommendationDataset
  return RecommendationDataset(sp.csr_matrix(np.eye(8, dtype=np.float32)))


@pytest.mark.parametrize("kw", [
  dict(optimizer_type="sgd"), dict(optimizer_type="adagrad"),
  dict(loss="mse", loss_params={"confidence": 1.0, "other": 2}),
  dict(loss="logistic", loss_params={"pos_weight": torch.ones(8)}),
  dict(loss=torch.nn.MSELoss()), dict(loss=torch.nn.BCEWithLogitsLoss(reduction="mean")),
  dict(loss="hinge"),
])
def test_recoder_rejects_before_gpu_work(kw):
  from recoder_amd.model import Recoder
  args = dict(loss="logloss", optimizer_type="adam")
  args.update(kw)
  rec = Recoder(model=_vae(), **args)
  with pytest.raises(ValueError):
    rec.train(_dataset(), batch_size=4)
  assert rec.model.num_items is None          # (init_model never ran: nothing was put on a device)


@pytest.mark.parametrize("env", [{"RK_FORCE_DP": "1"}, {"RK_PARALLEL": "items"}])
def test_recoder_rejects_parallel_runs(env, monkeypatch):
  from recoder_amd.model import Recoder
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  rec = Recoder(model=_vae(), loss="logloss", optimizer_type="adam")
  with pytest.raises(ValueError, match="users-DP or item-parallel"):
    rec.train(_dataset(), batch_size=4)


def test_recoder_rejects_injected_parallel_runs():
  from recoder_amd.model import Recoder
  rec = Recoder(model=_vae(), loss="logloss", optimizer_type="adam")
  rec._dp_override = object()
  with pytest.raises(ValueError):
    rec.train(_dataset(), batch_size=4)


def test_model_params_round_trip():
  from recoder_amd.nn import VariationalAutoencoder
  m = _vae(hidden_layers=[32, 16, 8], activation_type="relu", noise_prob=0.25, sparse=True, kl_cap=0.5,
           anneal_steps=123)
  m.anneal_step = 77
  p = m.model_params()
  assert p == {"hidden_layers": [32, 16, 8], "activation_type": "relu", "noise_prob": 0.25, "sparse": True,
               "kl_cap": 0.5, "anneal_steps": 123, "anneal_step": 77}
  n = VariationalAutoencoder()             # (the sizes come from the checkpoint)
  with pytest.raises(ValueError):
    n.init_model(10)
  n.load_model_params(p)
  assert n.model_params() == p
  with pytest.raises(ValueError):
    n.load_model_params(dict(p, kl_cap=-1.0))


def test_beta_schedule():
  m = _vae(kl_cap=0.2, anneal_steps=10)
  assert [m.beta(g) for g in (0, 5, 10, 20)] == [0.0, 0.2 * 0.5, 0.2, 0.2]
  m.anneal_step = 4
  assert m.beta() == 0.2 * 0.4
  assert _vae(kl_cap=0.3, anneal_steps=0).beta(0) == 0.3


def test_state_dict_keys_and_init_follow_dynamic_autoencoder():
  """DynamicAutoencoder's key names, the head Linear(h_{L-2}, 2d) last; same init scheme and order (the
  encoder side of a DynamicAutoencoder whose last size is 2d draws the same numbers)."""
  from recoder_amd.nn import DynamicAutoencoder, VariationalAutoencoder
  torch.manual_seed(3)
  v = VariationalAutoencoder([16, 12, 8])
  v.init_model(20)
  torch.manual_seed(3)
  a = DynamicAutoencoder([16, 12, 16])
  a.init_model(20)
  kv, ka = v.state_dict(), a.state_dict()
  assert list(kv) == list(ka)
  assert tuple(kv["encoding_layers.1.weight"].shape) == (16, 12)
  assert tuple(kv["decoding_layers.0.weight"].shape) == (12, 8)
  for k in ("en_embedding_layer.weight", "encoding_layers.0.weight", "encoding_layers.1.weight"):
    assert torch.equal(kv[k], ka[k]), k
  assert all(float(kv[k].abs().sum()) == 0.0 for k in kv if k.endswith("bias"))


def test_vae_is_not_a_dynamic_autoencoder():
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, fused_supported
  m = _vae()
  assert not isinstance(m, DynamicAutoencoder)
  assert fused_supported(m)
  assert Recoder(model=m)._fused_kind() == "ae"


def test_restatement_gradients_match_finite_differences():
  """The float64 restatement's KL term and sample: its autograd gradient of the head's output against
  central differences of its own objective."""
  torch.manual_seed(0)
  from recoder_amd.nn import VariationalAutoencoder
  m = VariationalAutoencoder([8, 4], activation_type="tanh")
  m.init_model(12)
  ref = vae_util.VaeRef(dict(m.named_parameters()), [8, 4], loss="logloss", kl_cap=0.7, anneal_steps=0)
  rng = np.random.RandomState(1)
  csr = sp.random(5, 12, density=0.4, random_state=rng, format="csr", dtype=np.float64)
  csr.data[:] = 1.0
  x, items = vae_util.batch(csr, np.arange(5))
  eps = rng.randn(5, 4)
  p = ref.params["encoding_layers.0.bias"]
  loss = ref.objective(x, items, None, eps)[0]
  g, = torch.autograd.grad(loss, p)
  for j in range(p.numel()):
    with torch.no_grad():
      p[j] += 1e-6
      up = ref.objective(x, items, None, eps)[0].item()
      p[j] -= 2e-6
      dn = ref.objective(x, items, None, eps)[0].item()
      p[j] += 1e-6
    assert abs((up - dn) / 2e-6 - g[j].item()) < 1e-6 * max(1.0, abs(g[j].item()))
