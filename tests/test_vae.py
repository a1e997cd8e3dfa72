"""GPU: VariationalAutoencoder (Mult-VAE) on the HIP step against the float64 restatement (tests/vae_util.py).

  - rk_vae_sample / rk_vae_sample_bwd through ctypes against numpy float64, the counter RNG's statistics and
    invariances;
  - one and ten steps of Recoder.train with injected input-dropout masks and eps (Recoder.mask_hook / eps_hook);
  - graph replay against the eagerly enqueued steps, bitwise;
  - evaluation (predict / recommend_array / validation loss), checkpoint resume, and learning on the
    ML-20M slice.

Bars as tests/test_hip_parity.py: losses within 1e-5 relative; gradients and parameters by close_stats /
tight_stats (restated here)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import vae_util

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
DEV = "cuda"


def close_stats(a, b, rtol, atol):
  a = np.asarray(a, dtype=np.float64)
  b = np.asarray(b, dtype=np.float64)
  err = np.abs(a - b)
  bad = err > atol + rtol * np.abs(b)
  return float(bad.mean()), float(err.max()), float(np.abs(b).max())


def tight_stats(a, b):
  a = np.asarray(a, dtype=np.float64)
  b = np.asarray(b, dtype=np.float64)
  err = np.abs(a - b)
  bad = err > 2e-7 + 1e-5 * np.abs(b)
  big = np.abs(b) > 1e-3
  mx_rel = float((err[big] / np.abs(b[big])).max()) if big.any() else 0.0
  return float(bad.mean()), mx_rel


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def synth_csr(n_users, n_items, mean_deg, seed):
  rng = np.random.RandomState(seed)
  pop = 1.0 / np.arange(1, n_items + 1) ** 0.8
  pop /= pop.sum()
  deg = np.clip(rng.lognormal(np.log(mean_deg) - 0.5, 1.0, n_users).astype(int), 1, n_items // 4)
  rows = np.repeat(np.arange(n_users), deg)
  cols = rng.choice(n_items, size=int(deg.sum()), p=pop)
  m = sp.coo_matrix((np.ones(len(cols), np.float32), (rows, cols)), shape=(n_users, n_items)).tocsr()
  m.sum_duplicates()
  m.data[:] = 1.0
  m.sort_indices()
  return m


# ------------------------------------------------------------------ kernels
def _sample(E, B, d, train, eps=None, users=None, row_off=0, rng_step=7, seed=0x5eed, beta=0.3, kl=True,
            cursor=None, off=0, table=None):
  from recoder_amd import _vae_lib
  lib = _vae_lib.load()
  z = torch.full((B, d), float("nan"), device=DEV)
  eo = torch.full((B, d), float("nan"), device=DEV)
  part = torch.full((B,), float("nan"), device=DEV) if kl else None
  _vae_lib.check(lib.rk_vae_sample(_p(E), B, d, train, _p(eps), seed, rng_step, _p(users), row_off, _p(cursor), off,
                                   _p(table), beta, _p(z), _p(eo) if train else None, _p(part), _stream()),
                 "rk_vae_sample")
  torch.cuda.synchronize()
  return z, eo, part


def _rand_e(B, d, seed):
  g = torch.Generator().manual_seed(seed)
  mu = torch.randn(B, d, generator=g)
  lv = torch.rand(B, d, generator=g) * 4.0 - 3.0
  return torch.cat([mu, lv], 1).to(DEV).contiguous()


@pytest.mark.parametrize("B,d", [(1, 1), (37, 200), (500, 200), (64, 65)])
def test_sample_and_backward_against_float64(B, d):
  from recoder_amd import _vae_lib
  E = _rand_e(B, d, B + d)
  eps = torch.randn(B, d, generator=torch.Generator().manual_seed(1)).to(DEV)
  beta = 0.37
  z, eo, part = _sample(E, B, d, 1, eps=eps, beta=beta)
  e64 = E.double().cpu().numpy()
  mu, lv = e64[:, :d], e64[:, d:]
  ep = eps.double().cpu().numpy()
  sig = np.exp(0.5 * lv)
  zr = mu + ep * sig
  assert torch.equal(eo, eps)
  u = np.finfo(np.float32).eps
  assert np.all(np.abs(z.double().cpu().numpy() - zr) <= 4 * u * (np.abs(mu) + np.abs(ep * sig)) + 1e-30)
  terms = np.exp(lv) + mu * mu - 1.0 - lv
  klr = beta * 0.5 * terms.sum(1)
  bound = (d + 4) * u * beta * 0.5 * (np.exp(lv) + mu * mu + 1.0 + np.abs(lv)).sum(1)
  assert np.all(np.abs(part.double().cpu().numpy() - klr) <= bound)
  # eval mode: z = mu bitwise, the same KL partials bitwise
  z0, _, part0 = _sample(E, B, d, 0, beta=beta)
  assert torch.equal(z0, E[:, :d])
  assert torch.equal(part0, part)
  # backward
  lib = _vae_lib.load()
  dz = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(DEV) * 1e-3
  inv = float(np.float32(1.0) / np.float32(B))
  dE = torch.full((B, 2 * d), float("nan"), device=DEV)
  _vae_lib.check(lib.rk_vae_sample_bwd(_p(E), _p(eo), _p(dz), B, d, inv, None, 0, None, beta, _p(dE), _stream()),
                 "rk_vae_sample_bwd")
  g = dz.double().cpu().numpy()
  bi = beta * inv
  dmu = g + bi * mu
  dlv = 0.5 * (g * ep * sig + bi * (np.exp(lv) - 1.0))
  got = dE.double().cpu().numpy()
  assert np.all(np.abs(got[:, :d] - dmu) <= 4 * u * (np.abs(g) + np.abs(bi * mu)) + 1e-30)
  assert np.all(np.abs(got[:, d:] - dlv) <= 6 * u * (np.abs(g * ep * sig) + np.abs(bi * np.exp(lv)) + bi) + 1e-30)


def test_rng_eps_statistics_and_invariance():
  B, d = 5000, 200
  E = torch.zeros(B, 2 * d, device=DEV)             # mu = 0, lv = 0: z = eps
  users = torch.arange(10_000, 10_000 + B, dtype=torch.int64, device=DEV) * 7
  z, eo, _ = _sample(E, B, d, 1, users=users, rng_step=11, kl=False)
  assert torch.equal(z, eo)
  x = eo.double().cpu().numpy().ravel()
  n = x.size
  assert n >= 1_000_000 and np.all(np.isfinite(x))
  mean, var = x.mean(), x.var()
  print("eps over %d draws: mean %.3e var %.5f" % (n, mean, var))
  assert abs(mean) < 5.0 / np.sqrt(n)
  assert abs(var - 1.0) < 5.0 * np.sqrt(2.0 / n)
  # a user's eps is the same whatever its row, the batch size or row_off
  perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
  sub = perm[:123]
  z2, _, _ = _sample(E[:123].contiguous(), 123, d, 1, users=torch.cat([users[:5], users[sub]]), row_off=5,
                     rng_step=11, kl=False)
  assert torch.equal(z2, eo[sub])
  # repeatable; another step gives other draws
  z3, _, _ = _sample(E, B, d, 1, users=users, rng_step=11, kl=False)
  assert torch.equal(z3, z)
  z4, _, _ = _sample(E, B, d, 1, users=users, rng_step=12, kl=False)
  assert not torch.equal(z4, z)


def test_cursor_takes_step_users_and_beta_from_the_device():
  """With a step cursor the kernel derives rng_step = cursor[0] + off + 1, the rows' users at
  (cursor[0] - cursor[1] + off) * B and beta from the table: bitwise the host-argument form."""
  B, d = 16, 24
  E = _rand_e(B, d, 5)
  cursor = torch.tensor([40, 30], dtype=torch.int64, device=DEV)     # global step 40, the epoch began at 30
  table = torch.arange(32, dtype=torch.float32, device=DEV) * 0.01
  off = 2                                                              # local step 12, global 42
  users_c = torch.arange(100 + 12 * B, 100 + 13 * B, dtype=torch.int64, device=DEV)
  order = torch.cat([torch.zeros(12 * B, dtype=torch.int64, device=DEV), users_c])
  zc, ec, pc = _sample(E, B, d, 1, users=order, cursor=cursor, off=off, table=table, rng_step=999, beta=5.0)
  zh, eh, ph = _sample(E, B, d, 1, users=users_c, rng_step=43, beta=float(table[12]))
  assert torch.equal(ec, eh) and torch.equal(zc, zh) and torch.equal(pc, ph)


# ------------------------------------------------------------ training steps
def _rec(h, loss="logloss", conf=0.0, sparse=False, noise=0.5, kl_cap=0.2, anneal_steps=4, seed=0):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import VariationalAutoencoder
  torch.manual_seed(seed)
  m = VariationalAutoencoder(hidden_layers=list(h), activation_type="tanh", noise_prob=noise, sparse=sparse,
                             kl_cap=kl_cap, anneal_steps=anneal_steps)
  return Recoder(model=m, loss=loss, loss_params={"confidence": conf} if loss == "mse" else None,
                 optimizer_type="adam")


class Hooks:
  """Injected user order, input-dropout masks and eps; the restatement reads the same arrays."""

  def __init__(self, csr, B, d, p, seed=0, start=0):
    self.csr, self.B, self.d, self.p, self.seed = csr, B, d, p, seed
    self.k = start                       # step counter (survives a checkpoint / a second train())
    self.log = []                        # (users, keep per entry, eps) of every step

  def order(self, epoch, n):
    return np.random.RandomState(self.seed * 1000 + self.k).permutation(n).astype(np.int64)

  def mask(self, step, users):
    rng = np.random.RandomState(10_000 + self.seed * 1000 + self.k)
    nnz = int(self.csr[np.asarray(users)].nnz)
    keep = (rng.rand(nnz) >= self.p).astype(np.uint8)
    self._keep = keep
    return torch.from_numpy(keep).to(DEV), None

  def eps(self, step, users):
    rng = np.random.RandomState(20_000 + self.seed * 1000 + self.k)
    e = rng.randn(len(users), self.d).astype(np.float32)
    self.log.append((np.asarray(users).copy(), self._keep, e))
    self.k += 1
    return e

  def install(self, rec):
    rec.user_order_hook, rec.mask_hook, rec.eps_hook = self.order, self.mask, self.eps


def _ref_of(rec, init, lr, wd=0.0):
  m = rec.model
  loss = rec.loss
  return vae_util.VaeRef(init, m.hidden_layers, act=m.activation_type, noise_prob=m.noise_prob, sparse=m.sparse,
                         loss=loss, loss_params=rec.loss_params, lr=lr, weight_decay=wd, kl_cap=m.kl_cap,
                         anneal_steps=m.anneal_steps, anneal_step=m.anneal_step)


def _ref_steps(ref, csr, log, keep_p):
  out = []
  for users, keep, eps in log:
    x, items = vae_util.batch(csr, users)
    kp = vae_util.dense_keep(csr, users, items, keep) if keep_p > 0 else None
    out.append(ref.step(x, items, kp, eps))
  return np.asarray(out), items


def _init(rec, ds, lr, wd=0.0):
  rec._Recoder__init_training(ds, lr, wd)
  return {k: v.detach().cpu().clone() for k, v in rec.model.named_parameters()}


def _check_close(name, got, want, rtol=1e-4):
  scale = float(np.abs(np.asarray(want)).max()) if np.size(want) else 0.0
  frac, mx, _ = close_stats(got, want, rtol, 1e-5 * max(scale, 1e-12))
  print("  %-52s bad %.2e max err %.3e (scale %.3e)" % (name, frac, mx, scale))
  assert frac < 2e-3, (name, frac, mx, scale)
  assert mx < 5e-3 * max(1e-12, scale), (name, mx, scale)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("loss,conf", [("logloss", 0.0), ("mse", 0.0), ("mse", 3.0), ("logistic", 0.0)])
@pytest.mark.parametrize("h", [[600, 200], [64, 32, 16]])
def test_steps_match_restatement(h, loss, conf, sparse):
  """Two steps with injected masks and eps: losses, every gradient of the second step, the parameters after
  it."""
  from recoder_amd.data import RecommendationDataset
  B, lr = 48, 1e-3
  csr = synth_csr(2 * B, 1500, 14, seed=len(h) * 10 + int(conf) + sparse)
  rec = _rec(h, loss, conf, sparse, noise=0.5, kl_cap=0.3, anneal_steps=1)
  ds = RecommendationDataset(csr)
  init = _init(rec, ds, lr)
  hk = Hooks(csr, B, h[-1], 0.5)
  hk.install(rec)
  rec.train(ds, batch_size=B, lr=lr, num_epochs=1, negative_sampling=True)
  got = rec.last_epoch_losses
  ref = _ref_of(rec, init, lr)
  ref.anneal_step = 0
  want, items = _ref_steps(ref, csr, hk.log, 0.5)
  rel = np.abs(got - want) / np.abs(want)
  print(h, loss, conf, sparse, "losses", got, want, "rel", rel)
  assert len(got) == 2 and rel.max() < LOSS_RTOL
  assert rec.model.anneal_step == 2
  eng = rec._Recoder__engine
  G = ref.last_grads
  n_b = len(items)
  t = torch.as_tensor(items)
  nl = len(h) - 1
  for i in range(nl):
    _check_close("encoding_layers.%d.weight grad" % i, eng.g_enc_w[i].cpu(), G["encoding_layers.%d.weight" % i])
    _check_close("encoding_layers.%d.bias grad" % i, eng.g_enc_b[i].cpu(), G["encoding_layers.%d.bias" % i])
    _check_close("decoding_layers.%d.weight grad" % i, eng.g_dec_w[i].cpu(), G["decoding_layers.%d.weight" % i])
    _check_close("decoding_layers.%d.bias grad" % i, eng.g_dec_b[i].cpu(), G["decoding_layers.%d.bias" % i])
  _check_close("en bias grad", eng.encoder_bias_grad().cpu(), G[vae_util.EN_B])
  _check_close("de bias grad", eng.decoder_bias_grad(n_b).cpu(), G[vae_util.DE_B][t])
  _check_close("de rows grad", eng.decoder_row_grad(n_b).cpu(), G[vae_util.DE_W][t])
  _check_close("en rows grad", eng.encoder_row_grad(n_b).cpu(), G[vae_util.EN_W][t])
  for k, v in rec.model.named_parameters():
    w = ref.params[k].detach().numpy()
    frac, mx, scale = close_stats(v.detach().cpu().numpy(), w, 1e-4, 2e-6)
    tfrac, trel = tight_stats(v.detach().cpu().numpy(), w)
    print("  %-52s bad %.2e max err %.3e | beyond 1e-5 rel %.2e, max rel %.2e" % (k, frac, mx, tfrac, trel))
    assert frac < 2e-3 and mx < 5e-3 * max(1.0, scale), k
    assert tfrac < 2e-2, k


def _train_ref_epochs(h, loss, kl_cap, anneal_steps, epochs, B, n, milestones=None, sparse=False, seed=1):
  from recoder_amd.data import RecommendationDataset
  lr = 2e-3
  csr = synth_csr(n, 900, 10, seed=seed)
  rec = _rec(h, loss, sparse=sparse, noise=0.5, kl_cap=kl_cap, anneal_steps=anneal_steps, seed=seed)
  ds = RecommendationDataset(csr)
  init = _init(rec, ds, lr)
  hk = Hooks(csr, B, h[-1], 0.5, seed=seed)
  hk.install(rec)
  rec.train(ds, batch_size=B, lr=lr, num_epochs=epochs, negative_sampling=True, lr_milestones=milestones)
  got = np.concatenate(rec.loss_history)
  return rec, init, hk, csr, got, lr


def test_ten_steps_with_milestone_and_anneal_ramp():
  B, spe = 32, 5
  rec, init, hk, csr, got, lr = _train_ref_epochs([64, 32, 16], "logloss", 0.2, 5, 2, B, B * spe, milestones=[2])
  ref = _ref_of(rec, init, lr)
  ref.anneal_step = 0
  want = []
  for i, (users, keep, eps) in enumerate(hk.log):
    if i == spe:
      ref.set_lr(lr * 0.1)
    x, items = vae_util.batch(csr, users)
    want.append(ref.step(x, items, vae_util.dense_keep(csr, users, items, keep), eps))
  want = np.asarray(want)
  rel = np.abs(got - want) / np.abs(want)
  print("10 steps", got, want, rel.max())
  assert len(got) == 10 and rel.max() < LOSS_RTOL
  assert rec.model.anneal_step == 10 and ref.beta() == 0.2


def test_kl_cap_zero_switches_the_kl_term_off():
  B = 32
  rec, init, hk, csr, got, lr = _train_ref_epochs([64, 16], "logloss", 0.0, 3, 1, B, 4 * B, seed=2)
  losses = {}
  for cap in (0.0, 5.0):
    ref = _ref_of(rec, init, lr)
    ref.kl_cap, ref.anneal_step = cap, 0
    losses[cap] = _ref_steps(ref, csr, hk.log, 0.5)[0]
  rel0 = np.abs(got - losses[0.0]) / losses[0.0]
  rel5 = np.abs(got - losses[5.0]) / losses[5.0]
  print("kl_cap 0:", rel0.max(), "against kl_cap 5:", rel5[1:].min())
  assert rel0.max() < LOSS_RTOL
  assert rel5[1:].min() > 20 * LOSS_RTOL           # (step 0 has beta = 0 either way)


# ---------------------------------------------------------- graph replay
def _run_counter_rng(sparse, graph, monkeypatch):
  from recoder_amd.data import RecommendationDataset
  monkeypatch.setenv("RK_GRAPH", "1" if graph else "0")
  B = 32
  csr = synth_csr(20 * B + 7, 1200, 12, seed=5)
  rec = _rec([64, 32, 16], "logloss", sparse=sparse, noise=0.5, kl_cap=0.2, anneal_steps=30, seed=4)
  orders = [np.random.RandomState(e).permutation(csr.shape[0]).astype(np.int64) for e in range(3)]
  rec.user_order_hook = lambda epoch, n: orders[epoch]
  rec.train(RecommendationDataset(csr), batch_size=B, lr=1e-3, num_epochs=2, negative_sampling=True)
  eng = rec._Recoder__engine
  st = {k: (v.detach().clone(), eng.states[k].m.clone(), eng.states[k].v.clone())
        for k, v in rec.model.named_parameters()}
  return rec, np.concatenate(rec.loss_history), st


@pytest.mark.parametrize("sparse", [False, True])
def test_graph_replay_is_bitwise_the_eager_steps(sparse, monkeypatch):
  rec_g, lg, sg = _run_counter_rng(sparse, True, monkeypatch)
  assert getattr(rec_g, "_graph_stepper", None) is not None, "the graph path did not run"
  rec_e, le, se = _run_counter_rng(sparse, False, monkeypatch)
  rec_g2, lg2, sg2 = _run_counter_rng(sparse, True, monkeypatch)
  assert rec_g.model.anneal_step == rec_e.model.anneal_step == 42
  assert np.all(np.isfinite(lg))
  print("losses", lg[:3], lg[-3:])
  assert np.array_equal(lg, le), np.abs(lg - le).max()
  assert np.array_equal(lg, lg2)
  for k in sg:
    for a, b, c in zip(sg[k], se[k], sg2[k]):
      assert torch.equal(a, b), k
      assert torch.equal(a, c), k


# ------------------------------------------------------------- evaluation
def test_predict_recommend_and_validation_loss():
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  B = 32
  rec, init, hk, csr, got, lr = _train_ref_epochs([64, 32, 16], "logloss", 0.2, 4, 1, B, 3 * B, seed=6)
  ref = _ref_of(rec, init, lr)
  ref.anneal_step = 0
  _ref_steps(ref, csr, hk.log, 0.5)
  for k, v in rec.model.named_parameters():        # (the evaluation compares the forward, not the training)
    ref.params[k].data.copy_(v.detach().cpu().double())
  users = np.arange(40)
  ui = UsersInteractions(users, csr[users])
  out, _ = rec.predict(ui)
  x = torch.as_tensor(np.asarray(csr[users].todense()), dtype=torch.float64)
  want = ref.scores(x).numpy()
  _check_close("predict scores", out.cpu().numpy(), want)
  k = 10
  recs = rec.recommend_array(ui, k)
  mine = out.cpu().numpy().copy()
  mine[np.asarray(csr[users].todense()) > 0] = -np.inf
  assert np.array_equal(recs, np.argsort(-mine, axis=1, kind="stable")[:, :k])
  wm = want.copy()
  wm[np.asarray(csr[users].todense()) > 0] = -np.inf
  agree = np.mean([np.array_equal(a, b) for a, b in zip(recs, np.argsort(-wm, axis=1, kind="stable")[:, :k])])
  print("top-%d rows equal to the restatement's: %.3f" % (k, agree))
  assert agree >= 0.9
  # dense forward of the module in eval mode: z = mu
  rec.model.eval()
  dense = rec.model(torch.as_tensor(np.asarray(csr[users].todense()), dtype=torch.float32, device=DEV))
  _check_close("model.forward(dense)", dense.cpu().numpy(), want)
  # validation loss: z = mu, beta of the next step, mean over the batches of the validation order
  vorder = np.random.RandomState(9).permutation(csr.shape[0]).astype(np.int64)
  rec.user_order_hook = lambda epoch, n: vorder
  from recoder_amd.data import RecommendationDataLoader
  vl = rec._validate(RecommendationDataLoader(RecommendationDataset(csr), batch_size=B, negative_sampling=True))
  want_v = []
  beta = ref.beta()
  assert beta == rec.model.beta()
  for off in range(0, csr.shape[0], B):
    xb, items = vae_util.batch(csr, vorder[off:off + B])
    want_v.append(ref.objective(xb, items, None, None, beta=beta)[0].item())
  print("validation loss", vl, np.mean(want_v))
  assert abs(vl - np.mean(want_v)) <= LOSS_RTOL * abs(np.mean(want_v))


def test_embeddings_index_reads_the_vae_tables():
  from recoder_amd.embedding import ExactEmbeddingsIndex
  rec, *_ = _train_ref_epochs([64, 16], "logloss", 0.2, 2, 1, 32, 64, seed=7)
  for layer, table in (("encoder", rec.model.en_embedding_layer), ("decoder", rec.model.de_embedding_layer)):
    ix = ExactEmbeddingsIndex.from_recoder(rec, layer=layer)
    assert torch.equal(torch.as_tensor(ix.embeddings).cpu(), table.weight.detach().cpu())
    nn = ix.get_nns_by_id(3, 5) if hasattr(ix, "get_nns_by_id") else None
    assert nn is None or len(nn) == 5


# ------------------------------------------------------------- checkpoint
def test_checkpoint_resume_equals_one_run(tmp_path):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import VariationalAutoencoder
  B, lr = 32, 1e-3
  csr = synth_csr(6 * B, 800, 10, seed=8)
  ds = RecommendationDataset(csr)

  def fresh():
    return _rec([64, 32, 16], "logloss", noise=0.5, kl_cap=0.2, anneal_steps=9, seed=3)

  one = fresh()
  hk1 = Hooks(csr, B, 16, 0.5, seed=8)
  hk1.install(one)
  one.train(ds, batch_size=B, lr=lr, num_epochs=2, negative_sampling=True)
  want = np.concatenate(one.loss_history)

  a = fresh()
  hk2 = Hooks(csr, B, 16, 0.5, seed=8)
  hk2.install(a)
  a.train(ds, batch_size=B, lr=lr, num_epochs=1, negative_sampling=True)
  path = a.save_state(str(tmp_path / "vae"))
  b = Recoder(model=VariationalAutoencoder(), optimizer_type="adam", loss="logloss")
  b.init_from_model_file(path)
  assert b.model.anneal_step == 6 and b.model.model_params() == a.model.model_params()
  hk3 = Hooks(csr, B, 16, 0.5, seed=8, start=hk2.k)
  hk3.install(b)
  b.train(ds, batch_size=B, lr=lr, num_epochs=1, negative_sampling=True)
  got = np.concatenate(a.loss_history + b.loss_history)
  print("12-step run", want, "resumed", got)
  assert len(got) == 12 and np.array_equal(got, want)
  assert b.model.anneal_step == one.model.anneal_step == 12
  for (k, v), (_, w) in zip(b.model.named_parameters(), one.model.named_parameters()):
    assert torch.equal(v, w), k


# ---------------------------------------------------------------- learning
def test_learns_on_the_ml20m_slice():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  x, y = vae_util.load_slice()
  rec = _rec([600, 200], "logloss", noise=0.5, kl_cap=0.2, anneal_steps=200, seed=0)
  rec.train(RecommendationDataset(x), batch_size=500, lr=1e-3, num_epochs=15, negative_sampling=True)
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(20), Recall(50), NDCG(100)], batch_size=500)
  vals = {str(m): float(np.nanmean(np.asarray(v, dtype=np.float64))) for m, v in res.items()}
  pop = vae_util.popularity_recall(x, y, 20)
  print("VAE [600, 200] logloss on the ML-20M slice: %s; popularity Recall@20 %.4f" % (vals, pop))
  assert vals["Recall@20"] > pop
