"""Float64 restatement of VariationalAutoencoder training (Mult-VAE, Liang et al. 2018) in torch autograd on
the CPU, independent of recoder_amd: what tests/test_vae.py compares the HIP step against.

It is fed explicit batches: the users' rows of a CSR, the negative-sampled item set (np.unique of the rows'
columns, as the collation builds it), the input-dropout keep mask per stored entry and eps.  Conventions are
the project's (and the reference's): one optimizer group per tensor, weight decay on everything but biases,
optim.Adam on dense tensors and optim.SparseAdam on sparse embedding tables, loss / rows."""
import os
from collections import OrderedDict

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))

EN_W = "en_embedding_layer.weight"
EN_B = "_DynamicAutoencoder__en_linear_embedding_layer.bias"
DE_W = "de_embedding_layer.weight"
DE_B = "_DynamicAutoencoder__de_linear_embedding_layer.bias"


def batch(csr, users, negative_sampling=True):
  """(dense [rows, n_b] float64 input, item ids int64 [n_b] or None) of `users`' rows."""
  rows = csr[np.asarray(users, dtype=np.int64)]
  if negative_sampling:
    items = np.unique(rows.indices).astype(np.int64)
    return torch.as_tensor(np.asarray(rows[:, items].todense()), dtype=torch.float64), items
  return torch.as_tensor(np.asarray(rows.todense()), dtype=torch.float64), None


def dense_keep(csr, users, items, keep_nnz):
  """A keep flag per stored entry (row-major, columns ascending) -> [rows, n_b] 0/1 (1 off the support)."""
  rows = csr[np.asarray(users, dtype=np.int64)].tocoo()
  n_b = csr.shape[1] if items is None else len(items)
  m = np.ones((rows.shape[0], n_b))
  col = rows.col if items is None else np.searchsorted(items, rows.col)
  order = np.lexsort((col, rows.row))
  m[rows.row[order], col[order]] = np.asarray(keep_nnz, dtype=np.float64)
  return torch.as_tensor(m)


def _act(x, act):
  return x if act == "none" else getattr(torch, act)(x)


def beta_of(kl_cap, anneal_steps, g):
  return float(kl_cap) if anneal_steps == 0 else float(kl_cap) * min(1.0, float(g) / float(anneal_steps))


class VaeRef:
  def __init__(self, state, hidden_layers, act="tanh", noise_prob=0.0, sparse=False, loss="logloss",
               loss_params=None, lr=1e-3, weight_decay=0.0, kl_cap=0.2, anneal_steps=0, anneal_step=0):
    self.h = list(hidden_layers)
    self.nl = len(self.h) - 1
    self.act, self.noise_prob, self.sparse = act, float(noise_prob), bool(sparse)
    self.loss, self.conf = loss, float((loss_params or {}).get("confidence", 0.0))
    self.kl_cap, self.anneal_steps, self.anneal_step = kl_cap, anneal_steps, int(anneal_step)
    self.params = OrderedDict((k, torch.nn.Parameter(torch.as_tensor(v).detach().clone().double()))
                              for k, v in state.items() if not k.endswith("embedding_layer.embedding_layer.weight"))
    sparse_names = [EN_W, DE_W] if self.sparse else []
    groups, sgroups = [], []
    for name, p in self.params.items():
      g = {"params": p, "weight_decay": 0 if "bias" in name else weight_decay}
      (sgroups if name in sparse_names else groups).append(g)
    self.opt = torch.optim.Adam(groups, lr=lr) if groups else None
    self.sopt = torch.optim.SparseAdam(sgroups, lr=lr) if sgroups else None
    self.last_grads = None

  def set_lr(self, lr):
    for g in self.opt.param_groups:
      g["lr"] = lr

  def beta(self):
    return beta_of(self.kl_cap, self.anneal_steps, self.anneal_step)

  def _head(self, x, items, keep):
    P = self.params
    z = F.normalize(x, p=2, dim=1)
    if keep is not None and self.noise_prob > 0.0:
      z = z * keep / (1.0 - self.noise_prob)
    w = P[EN_W] if items is None else F.embedding(torch.as_tensor(items), P[EN_W], sparse=self.sparse)
    a = _act(F.linear(z, w.t(), P[EN_B]), self.act)
    for i in range(self.nl):
      a = F.linear(a, P["encoding_layers.%d.weight" % i], P["encoding_layers.%d.bias" % i])
      if i < self.nl - 1:
        a = _act(a, self.act)
    d = self.h[-1]
    return a[:, :d], a[:, d:]

  def _decode(self, z, items):
    P = self.params
    for i in range(self.nl):
      z = _act(F.linear(z, P["decoding_layers.%d.weight" % i], P["decoding_layers.%d.bias" % i]), self.act)
    if items is None:
      return F.linear(z, P[DE_W], P[DE_B])
    t = torch.as_tensor(items)
    return F.linear(z, F.embedding(t, P[DE_W], sparse=self.sparse), P[DE_B].index_select(0, t))

  def _rec_loss(self, out, t):
    if self.loss == "mse":
      return ((1 + self.conf * (t > 0).double()) * (out - t) ** 2).sum()
    if self.loss == "logloss":
      return (-t * F.log_softmax(out, dim=1)).sum()
    return F.binary_cross_entropy_with_logits(out, t, reduction="sum")

  def objective(self, x, items, keep=None, eps=None, beta=None):
    """(loss, mu, logvar, z): eps None -> z = mu (evaluation)."""
    mu, lv = self._head(x, items, keep)
    z = mu if eps is None else mu + torch.as_tensor(eps, dtype=torch.float64) * torch.exp(0.5 * lv)
    out = self._decode(z, items)
    kl = 0.5 * (torch.exp(lv) + mu * mu - 1.0 - lv).sum()
    b = self.beta() if beta is None else beta
    return (self._rec_loss(out, x) + b * kl) / x.shape[0], mu, lv, z

  def step(self, x, items, keep=None, eps=None):
    """One training step; returns the loss (float) and keeps the gradients in last_grads."""
    for o in (self.opt, self.sopt):
      if o is not None:
        o.zero_grad()
    loss = self.objective(x, items, keep, eps)[0]
    loss.backward()
    g = {}
    for k, p in self.params.items():
      if p.grad is None:
        continue
      g[k] = p.grad.to_dense().clone() if p.grad.is_sparse else p.grad.clone()
    self.last_grads = g
    for o in (self.opt, self.sopt):
      if o is not None:
        o.step()
    self.anneal_step += 1
    return float(loss.item())

  @torch.no_grad()
  def scores(self, x):
    """Evaluation scores (z = mu) of dense full-catalogue rows against every item."""
    mu, _ = self._head(x, None, None)
    return self._decode(mu, None)

  def adam_state(self, name):
    p = self.params[name]
    for o in (self.opt, self.sopt):
      if o is not None and p in o.state:
        st = o.state[p]
        return st["exp_avg"], st["exp_avg_sq"]
    return None


def popularity_recall(x_csr, y_csr, k):
  """Mean normalised Recall@k of ranking every user's unseen items by their training popularity."""
  pop = np.asarray(x_csr.sum(axis=0)).ravel().astype(np.float64)
  order = np.argsort(-pop, kind="stable")
  out = []
  for u in range(x_csr.shape[0]):
    tgt = set(y_csr.indices[y_csr.indptr[u]:y_csr.indptr[u + 1]].tolist())
    if not tgt:
      continue
    seen = set(x_csr.indices[x_csr.indptr[u]:x_csr.indptr[u + 1]].tolist())
    rec = [i for i in order[:k + len(seen)] if i not in seen][:k]
    out.append(len(tgt.intersection(rec)) / min(k, len(tgt)))
  return float(np.mean(out))


def load_slice():
  z = np.load(os.path.join(HERE, "golden", "real_ml20m_slice.npz"))
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")
