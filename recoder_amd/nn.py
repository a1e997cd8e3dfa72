"""Factorization models with the reference's public contract (recoder/nn.py).

``FactorizationModel`` (nn.py:12-65), ``DynamicAutoencoder`` (nn.py:68-253),
``LinearEmbedding`` (nn.py:256-280) and ``MatrixFactorization`` (nn.py:283-362)
keep their constructor arguments, the four-method model contract, the RNG
consumption order of ``init_model`` and -- because checkpoints are exchanged
with the reference (model.py:193-224) -- the exact ``state_dict`` key names,
including the name-mangled private sub-modules.

The modules are parameter containers: ``forward`` does not run torch ops, it
hands the tensors to the HIP kernels (recoder_amd.engine); training goes through
``Recoder`` which drives the fused step.
"""
import torch
from torch import nn

import torch.nn.functional as F

_ACTS = ("none", "tanh", "sigmoid", "relu", "selu", "elu")


def _activate(x, act):
  return x if act == "none" else getattr(torch, act)(x)


def _embedding_linear(table, bias, ids, x, input_based, sparse):
  """LinearEmbedding (nn.py:269-280) in torch ops: a linear layer whose weight is the
  row subset ``ids`` of an embedding table (all rows when ids is None)."""
  w = table.weight if ids is None else F.embedding(ids, table.weight, sparse=sparse)
  if input_based:
    return F.linear(x, w.t(), bias)
  b = bias if ids is None or bias is None else bias.index_select(0, ids)
  return F.linear(x, w, b)


class FactorizationModel(nn.Module):
  """Base class: subclasses implement the four methods below (nn.py:18-65)."""

  def init_model(self, num_items=None, num_users=None):
    raise NotImplementedError

  def model_params(self):
    raise NotImplementedError

  def load_model_params(self, model_params):
    raise NotImplementedError

  def forward(self, input, input_users=None, input_items=None, target_users=None,
              target_items=None):
    raise NotImplementedError


class LinearEmbedding(nn.Module):
  """A linear layer whose weight matrix is (a row subset of) an embedding
  table (nn.py:256-280).  Holds the bias; the table is shared."""

  def __init__(self, embedding_layer, input_based=True, bias=True):
    super().__init__()
    self.embedding_layer = embedding_layer
    self.input_based = input_based
    n, d = embedding_layer.num_embeddings, embedding_layer.embedding_dim
    self.in_features = n if input_based else d
    self.out_features = d if input_based else n
    self.bias = nn.Parameter(torch.zeros(self.out_features)) if bias else None


def _check_act(act):
  """The reference takes 'none' or the name of any ``torch.<name>`` function (nn.py:6-9).  The
  fused HIP kernels implement _ACTS; every other name trains through the generic torch-autograd
  path on the GPU (recoder_amd/generic.py) -- unknown names fail here, as early as possible."""
  if act not in _ACTS and not callable(getattr(torch, str(act), None)):
    raise AttributeError("module 'torch' has no attribute %r (activation_type)" % (act,))


def fused_supported(model):
  """True when the HIP kernels cover this model instance: a fused activation and 16-byte
  embedding rows (hidden_layers[0] / embedding_size a multiple of 4)."""
  h0 = (model.hidden_layers[0] if isinstance(model, (DynamicAutoencoder, VariationalAutoencoder))
        else model.embedding_size)
  return model.activation_type in _ACTS and h0 % 4 == 0


class DynamicAutoencoder(FactorizationModel):
  """Autoencoder over variable item subsets (nn.py:68-253).

  Args mirror the reference: hidden_layers, activation_type, is_constrained,
  dropout_prob, noise_prob, sparse.
  """

  def __init__(self, hidden_layers=None, activation_type="tanh", is_constrained=False,
               dropout_prob=0.0, noise_prob=0.0, sparse=False):
    super().__init__()
    self.activation_type = activation_type
    self.is_constrained = is_constrained
    self.hidden_layers = hidden_layers
    self.dropout_prob = dropout_prob
    self.noise_prob = noise_prob
    self.sparse = sparse
    self.num_items = None
    self.num_embeddings = None
    # kept for attribute compatibility (nn.py:141-143); the fused kernels own
    # the dropout arithmetic
    self.noise_layer = None
    self.dropout_layer = None

  # -- the four-method contract ------------------------------------------
  def init_model(self, num_items=None, num_users=None):
    _check_act(self.activation_type)
    self.num_items = num_items
    self.num_embeddings = num_items
    h = self.hidden_layers
    # encoder side first, then decoder side: same RNG consumption order as
    # nn.py:179-212 (Embedding N(0,1) draw, Linear default draws, xavier draws)
    self.en_embedding_layer = nn.Embedding(num_items, h[0], sparse=self.sparse)
    self.__en_linear_embedding_layer = LinearEmbedding(self.en_embedding_layer, input_based=True)
    self.encoding_layers = nn.Sequential(*self._coding_layers(h))
    nn.init.xavier_uniform_(self.en_embedding_layer.weight)
    nn.init.constant_(self.__en_linear_embedding_layer.bias, 0)

    dec = self._coding_layers(list(reversed(h)))
    if self.is_constrained:
      for layer in dec:
        del layer.weight          # only the biases stay registered (nn.py:192-196)
      self.de_embedding_layer = self.en_embedding_layer
    else:
      self.de_embedding_layer = nn.Embedding(num_items, h[0], sparse=self.sparse)
    self.decoding_layers = nn.Sequential(*dec)
    self.__de_linear_embedding_layer = LinearEmbedding(self.de_embedding_layer, input_based=False)
    nn.init.xavier_uniform_(self.de_embedding_layer.weight)
    nn.init.constant_(self.__de_linear_embedding_layer.bias, 0)

    self.noise_layer = nn.Dropout(p=self.noise_prob) if self.noise_prob > 0.0 else None
    self.dropout_layer = nn.Dropout(p=self.dropout_prob) if self.dropout_prob > 0.0 else None

  @staticmethod
  def _coding_layers(sizes):
    layers = []
    for i in range(1, len(sizes)):
      lin = nn.Linear(sizes[i - 1], sizes[i])
      nn.init.xavier_uniform_(lin.weight)
      nn.init.constant_(lin.bias, 0)
      layers.append(lin)
    return layers

  def model_params(self):
    return {
      "hidden_layers": self.hidden_layers,
      "activation_type": self.activation_type,
      "is_constrained": self.is_constrained,
      "dropout_prob": self.dropout_prob,
      "noise_prob": self.noise_prob,
    }

  def load_model_params(self, model_params):
    self.hidden_layers = model_params["hidden_layers"]
    self.activation_type = model_params["activation_type"]
    self.is_constrained = model_params["is_constrained"]
    self.dropout_prob = model_params["dropout_prob"]
    self.noise_prob = model_params["noise_prob"]

  # -- accessors used by the engine ---------------------------------------
  @property
  def en_bias(self):
    return self.__en_linear_embedding_layer.bias

  @property
  def de_bias(self):
    return self.__de_linear_embedding_layer.bias

  def forward(self, input, input_users=None, input_items=None, target_users=None,
              target_items=None):
    """Dense-input forward (nn.py:228-253) on the HIP kernels; no autograd."""
    if not fused_supported(self):
      with torch.no_grad():
        return self.torch_forward(input, input_users, input_items, target_users, target_items)
    from .engine import ae_dense_forward
    return ae_dense_forward(self, input, input_items, target_items)

  def torch_forward(self, input, input_users=None, input_items=None, target_users=None,
                    target_items=None):
    """The same forward in differentiable torch ops (on the GPU).  Only the generic
    path of Recoder uses it: nn.Module losses and the sgd/adagrad/rmsprop optimizers
    have no fused kernels and train through autograd (recoder_amd/generic.py)."""
    act, nl = self.activation_type, len(self.hidden_layers) - 1
    z = F.normalize(input, p=2, dim=1)
    if self.noise_layer is not None:
      z = self.noise_layer(z)
    z = _activate(_embedding_linear(self.en_embedding_layer, self.en_bias, input_items, z, True,
                                    self.sparse), act)
    for layer in self.encoding_layers:
      z = _activate(layer(z), act)
    if self.dropout_layer is not None:
      z = self.dropout_layer(z)
    for i, layer in enumerate(self.decoding_layers):
      w = self.encoding_layers[nl - 1 - i].weight.t() if self.is_constrained else layer.weight
      z = _activate(F.linear(z, w, layer.bias), act)
    return _embedding_linear(self.de_embedding_layer, self.de_bias, target_items, z, False,
                             self.sparse)


class MatrixFactorization(FactorizationModel):
  """Matrix factorization (nn.py:283-362): act(E_u[users]) . E_i[T]^T + b[T]."""

  def __init__(self, embedding_size, activation_type="none", dropout_prob=0, sparse=False):
    super().__init__()
    self.embedding_size = embedding_size
    self.activation_type = activation_type
    self.dropout_prob = dropout_prob
    self.sparse = sparse
    self.num_users = None
    self.num_items = None
    self.user_embedding_layer = None
    self.item_embedding_layer = None
    self.bias = None
    self.dropout_layer = None

  def init_model(self, num_items=None, num_users=None):
    _check_act(self.activation_type)
    self.num_users = num_users
    self.num_items = num_items
    self.user_embedding_layer = nn.Embedding(num_users, self.embedding_size, sparse=self.sparse)
    self.item_embedding_layer = nn.Embedding(num_items, self.embedding_size, sparse=self.sparse)
    self.bias = nn.Parameter(torch.zeros(num_items))
    self.dropout_layer = nn.Dropout(p=self.dropout_prob) if self.dropout_prob > 0.0 else None
    nn.init.xavier_uniform_(self.user_embedding_layer.weight)
    nn.init.xavier_uniform_(self.item_embedding_layer.weight)
    nn.init.constant_(self.bias, 0)

  def model_params(self):
    return {
      "embedding_size": self.embedding_size,
      "activation_type": self.activation_type,
      "dropout_prob": self.dropout_prob,
    }

  def load_model_params(self, model_params):
    self.embedding_size = model_params["embedding_size"]
    self.activation_type = model_params["activation_type"]
    self.dropout_prob = model_params["dropout_prob"]

  def forward(self, input, input_users=None, input_items=None, target_users=None,
              target_items=None):
    if not fused_supported(self):
      with torch.no_grad():
        return self.torch_forward(input, input_users, input_items, target_users, target_items)
    from .engine import mf_dense_forward
    return mf_dense_forward(self, input_users, target_items)

  def torch_forward(self, input, input_users=None, input_items=None, target_users=None,
                    target_items=None):
    """Differentiable torch-op forward for the generic path (see DynamicAutoencoder)."""
    u = _activate(self.user_embedding_layer(input_users), self.activation_type)
    if self.dropout_layer is not None:
      u = self.dropout_layer(u)
    if target_items is None:
      return F.linear(u, self.item_embedding_layer.weight, self.bias)
    return F.linear(u, self.item_embedding_layer(target_items),
                    self.bias.index_select(0, target_items))


class VariationalAutoencoder(FactorizationModel):
  """Mult-VAE (Liang et al. 2018, "Variational Autoencoders for Collaborative Filtering") over
  variable item subsets, trained on the fused HIP step.

  For ``hidden_layers = [h_0, ..., h_{L-1}]`` (L >= 2, d = h_{L-1}): the encoder of
  DynamicAutoencoder (L2-normalised input, input dropout ``noise_prob``, ``act(x . W_en[I] + b_en)``,
  Linear layers with ``act``) up to h_{L-2}, then a head ``Linear(h_{L-2}, 2d)`` without activation
  that gives ``[mu | logvar]``.  Training samples ``z = mu + eps * exp(0.5 logvar)``, evaluation takes
  ``z = mu``; the decoder is DynamicAutoencoder's for the reversed sizes (no tied weights, no bottleneck
  dropout).  The step's loss adds ``beta * KL`` with ``beta = kl_cap * min(1, anneal_step /
  anneal_steps)`` (``kl_cap`` when ``anneal_steps == 0``); ``anneal_step`` counts the training steps
  taken and travels in ``model_params()``.

  Not a DynamicAutoencoder subclass: every path that treats a DynamicAutoencoder as such would drop the
  KL term.  The state-dict keys are DynamicAutoencoder's (the LinearEmbedding biases included), the
  last ``encoding_layers`` entry being the head.
  """

  # (what the fused engine reads of an autoencoder: this model has neither)
  is_constrained = False
  dropout_prob = 0.0

  def __init__(self, hidden_layers=None, activation_type="tanh", noise_prob=0.0, sparse=False,
               kl_cap=0.2, anneal_steps=200000):
    super().__init__()
    self.hidden_layers = hidden_layers
    self.activation_type = activation_type
    self.noise_prob = noise_prob
    self.sparse = sparse
    self.kl_cap = kl_cap
    self.anneal_steps = anneal_steps
    self.anneal_step = 0
    self.num_items = None
    self.num_embeddings = None
    self.noise_layer = None
    if hidden_layers is not None:         # (None: the sizes come from load_model_params)
      self._validate()

  def _validate(self):
    h = self.hidden_layers
    if h is None or len(h) < 2:
      raise ValueError("VariationalAutoencoder needs hidden_layers with at least two sizes "
                       "([..., h_{L-2}, d]: the last is the latent size)")
    if any(int(x) < 1 for x in h):
      raise ValueError("hidden_layers must be positive sizes")
    if not float(self.kl_cap) >= 0.0:
      raise ValueError("kl_cap must be >= 0")
    if int(self.anneal_steps) < 0:
      raise ValueError("anneal_steps must be >= 0")
    if self.activation_type not in _ACTS:
      raise ValueError("VariationalAutoencoder trains on the fused HIP kernels only: activation_type must be "
                       "one of %s" % (_ACTS,))
    if int(h[0]) % 4 != 0:
      raise ValueError("hidden_layers[0] must be a multiple of 4 (16-byte embedding rows)")
    if not 0.0 <= float(self.noise_prob) < 1.0:
      raise ValueError("noise_prob must be in [0, 1)")

  def beta(self, step=None):
    """The KL weight of the training step after `step` steps (default: the next one)."""
    g = self.anneal_step if step is None else step
    if int(self.anneal_steps) == 0:
      return float(self.kl_cap)
    return float(self.kl_cap) * min(1.0, float(g) / float(self.anneal_steps))

  # -- the four-method contract ------------------------------------------
  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.num_embeddings = num_items
    h = list(self.hidden_layers)
    d = h[-1]
    # DynamicAutoencoder's scheme and order: the encoder side, then the decoder side
    self.en_embedding_layer = nn.Embedding(num_items, h[0], sparse=self.sparse)
    self._DynamicAutoencoder__en_linear_embedding_layer = LinearEmbedding(self.en_embedding_layer,
                                                                          input_based=True)
    self.encoding_layers = nn.Sequential(*DynamicAutoencoder._coding_layers(h[:-1] + [2 * d]))
    nn.init.xavier_uniform_(self.en_embedding_layer.weight)
    nn.init.constant_(self.en_bias, 0)
    dec = DynamicAutoencoder._coding_layers(list(reversed(h)))
    self.de_embedding_layer = nn.Embedding(num_items, h[0], sparse=self.sparse)
    self.decoding_layers = nn.Sequential(*dec)
    self._DynamicAutoencoder__de_linear_embedding_layer = LinearEmbedding(self.de_embedding_layer,
                                                                          input_based=False)
    nn.init.xavier_uniform_(self.de_embedding_layer.weight)
    nn.init.constant_(self.de_bias, 0)
    self.noise_layer = nn.Dropout(p=self.noise_prob) if self.noise_prob > 0.0 else None

  def model_params(self):
    return {
      "hidden_layers": self.hidden_layers,
      "activation_type": self.activation_type,
      "noise_prob": self.noise_prob,
      "sparse": self.sparse,
      "kl_cap": self.kl_cap,
      "anneal_steps": self.anneal_steps,
      "anneal_step": int(self.anneal_step),
    }

  def load_model_params(self, model_params):
    self.hidden_layers = model_params["hidden_layers"]
    self.activation_type = model_params["activation_type"]
    self.noise_prob = model_params["noise_prob"]
    self.sparse = model_params.get("sparse", self.sparse)
    self.kl_cap = model_params["kl_cap"]
    self.anneal_steps = model_params["anneal_steps"]
    self.anneal_step = int(model_params.get("anneal_step", 0))
    self._validate()

  # -- accessors used by the engine ---------------------------------------
  @property
  def en_bias(self):
    return self._DynamicAutoencoder__en_linear_embedding_layer.bias

  @property
  def de_bias(self):
    return self._DynamicAutoencoder__de_linear_embedding_layer.bias

  def forward(self, input, input_users=None, input_items=None, target_users=None,
              target_items=None):
    """Dense-input forward on the HIP kernels (z = mu in eval mode, a counter-RNG sample in
    training mode); no autograd."""
    from .engine import ae_dense_forward
    return ae_dense_forward(self, input, input_items, target_items)


def dense_to_csr(input, input_items, n):
  """The non-zeros of a dense [B, len(input_items)] batch as a CSR over the n items of the catalogue, in the
  layout the scores kernels read: int64 ``indptr``, int32 ``indices`` ascending inside each row (column c
  of ``input`` is item ``input_items[c]``; None: item c), f32 ``data``; an empty batch keeps a one-element
  ``indices``."""
  from types import SimpleNamespace
  nz = input.nonzero()
  rows, cols = nz[:, 0], nz[:, 1]
  vals = input[rows, cols].to(torch.float32)
  if input_items is not None:
    cols = input_items.to(torch.int64)[cols]
    order = torch.argsort(rows * n + cols)          # (ascending item ids inside a row)
    rows, cols, vals = rows[order], cols[order], vals[order]
  B = input.shape[0]
  indptr = torch.zeros(B + 1, dtype=torch.int64, device=input.device)
  indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=B), 0)
  indices = cols.to(torch.int32) if cols.numel() else torch.zeros(1, dtype=torch.int32, device=input.device)
  return SimpleNamespace(indptr=indptr, indices=indices.contiguous(), data=vals.contiguous(), shape=(B, n))


class CsrScoresModel(FactorizationModel):
  """A model without an encoder: a user's scores come from the user's CSR row alone.  ``Recoder.predict`` and
  ``Recoder.recommend_array`` hand such a model the batch's device CSR, strip by strip.  A class that
  ``Recoder.train`` cannot descend on names ``fit_method``, the ``Recoder`` method that fits it, and
  ``fit_sentence``, what ``train`` raises instead (``%s``: the method)."""
  fit_method = fit_sentence = None

  def forward(self, input, input_users=None, input_items=None, target_users=None,
              target_items=None):
    """The scores of a dense batch on the model's HIP scores kernel (``csr_scores`` over the input's non-zeros as a
    CSR over the catalogue, ascending); no autograd.  On the host (no device tensors) it is ``torch_forward``."""
    if not input.is_cuda:
      with torch.no_grad():
        return self.torch_forward(input, input_users, input_items, target_users, target_items)
    n = self.num_items
    csr = dense_to_csr(input, input_items, n)
    out = self.csr_scores(csr, 0, n, None, None, input.shape[0])
    return out if target_items is None else out.index_select(1, target_items.to(torch.int64))

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    """out[u, c] = the score of item lo + c for row u of ``csr``, for c < hi - lo and u < n_rows, ``out`` f32
    with row stride ``ld`` (None with ``out`` None: a new [n_rows, hi - lo] tensor); returns ``out``.  This
    is what ``Recoder.predict`` and ``Recoder.recommend_array`` call, whatever the class; the strips of one
    batch are calls with the same ``csr`` object."""
    raise NotImplementedError


class ItemItemModel(CsrScoresModel):
  """What the item-item models share: ``scores = input @ W`` for a fitted [num_items, num_items] W that a
  subclass stores in its own way.  A subclass gives ``csr_scores`` (its HIP scores kernel: out[u, c] =
  (row u of ``csr``) @ W[:, lo + c]) and ``_dense_w`` (W as a dense matrix, for ``torch_forward``)."""

  def _dense_w(self):
    raise NotImplementedError

  def torch_forward(self, input, input_users=None, input_items=None, target_users=None,
                    target_items=None):
    """The same forward in torch ops on the dense W (the generic engine's validation loss; host tensors)."""
    w = self._dense_w()
    if input_items is not None:
      w = w.index_select(0, input_items.to(torch.int64))
    if target_items is not None:
      w = w.index_select(1, target_items.to(torch.int64))
    return input.to(w.dtype) @ w


class ShallowAutoencoder(ItemItemModel):
  """EASE (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"): the linear item-item
  autoencoder ``scores = input @ item_weights`` with a zero diagonal, fitted in closed form by
  ``Recoder.train_ease`` (recoder_amd/ease.py) -- ``B = -P / diag(P)`` by columns,
  ``P = (X^T X + reg I)^-1``.

  One parameter, ``item_weights`` [num_items, num_items], zero until fitted; ``reg`` travels in
  ``model_params()``.  Gradient training would not keep the zero diagonal, so ``Recoder.train`` refuses
  this model and points at ``train_ease``.
  """
  fit_method = "train_ease"
  fit_sentence = ("a ShallowAutoencoder is fitted in closed form: call %s(train_dataset) "
                  "(gradient steps would not keep its zero diagonal)")

  def __init__(self, reg=500.0):
    super().__init__()
    self.reg = reg
    self.num_items = None
    self.item_weights = None
    self._validate()

  def _validate(self):
    if not float(self.reg) > 0.0 or float(self.reg) == float("inf"):
      raise ValueError("ShallowAutoencoder needs a finite reg > 0 (got %r)" % (self.reg,))

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.item_weights = nn.Parameter(torch.zeros(num_items, num_items), requires_grad=False)

  def model_params(self):
    return {"reg": float(self.reg)}

  def load_model_params(self, model_params):
    self.reg = float(model_params["reg"])
    self._validate()

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    from . import ease
    return ease.scores(csr, self.item_weights.data, lo, hi, out=out, ld=ld, n_rows=n_rows)     # (rk_ease_scores)

  def _dense_w(self):
    return self.item_weights


class GraphFilterModel(ItemItemModel):
  """GF-CF (Shen et al. 2021, "How Powerful is Graph Convolution for Recommendation?"): the closed-form
  graph-filter item model ``scores = input @ item_weights`` with
  ``W = Rn^T Rn + alpha * D_I^-1/2 V V^T D_I^1/2`` over the normalised user-item graph
  ``Rn = D_U^-1/2 R D_I^-1/2`` of the stored entries, V the top ``rank`` right singular vectors of Rn: a linear
  filter plus an ideal low-pass filter, fitted by ``Recoder.train_gfcf`` (recoder_amd/gfcf.py).  W is not
  symmetric and its diagonal is not zero (the masked top-k removes seen items anyway).

  One parameter, ``item_weights`` [num_items, num_items], zero until fitted; ``rank`` and ``alpha`` travel in
  ``model_params()``.  The defaults are the best Recall@20 of the float64 grid on the ML-20M slice
  (profiles/gfcf_quality.jsonl); the paper's are rank 256, alpha 0.3.  There is nothing to descend on:
  ``Recoder.train`` refuses this model and points at ``train_gfcf``.
  """
  fit_method = "train_gfcf"
  fit_sentence = ("a GraphFilterModel is fitted in closed form from the normalised interaction graph: call "
                  "%s(train_dataset)")

  def __init__(self, rank=128, alpha=3.0):
    super().__init__()
    self.rank = rank
    self.alpha = alpha
    self.num_items = None
    self.item_weights = None
    self._validate()

  def _validate(self):
    from .gfcf import check_params
    self.rank, self.alpha = check_params(self.rank, self.alpha)

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.item_weights = nn.Parameter(torch.zeros(num_items, num_items), requires_grad=False)

  def model_params(self):
    return {"rank": int(self.rank), "alpha": float(self.alpha)}

  def load_model_params(self, model_params):
    self.rank = int(model_params["rank"])
    self.alpha = float(model_params["alpha"])
    self._validate()

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    from . import ease
    return ease.scores(csr, self.item_weights.data, lo, hi, out=out, ld=ld, n_rows=n_rows)     # (rk_ease_scores)

  def _dense_w(self):
    return self.item_weights


class AdmmSlimModel(ItemItemModel):
  """ADMM-SLIM (Steck, Dimakis, Riabov & Jebara 2020, "ADMM SLIM: Sparse Recommendations for Many Users"): the
  item-item model ``scores = input @ item_weights`` that minimises SLIM's objective
  ``1/2 |X - X B|^2 + l2_reg/2 |B|^2 + l1_reg |B|_1`` with a zero diagonal (and ``B >= 0`` with ``nonneg``) over the
  whole matrix at once, by ``num_iterations`` ADMM iterations with penalty ``rho``, each a ridge step on EASE's
  inverse and a soft-threshold; fitted by ``Recoder.train_admm_slim`` (recoder_amd/admm.py).  With ``l1_reg`` 0 and
  ``nonneg`` False it converges to EASE at ``reg = l2_reg``; ``rho`` has to be of the order of ``l2_reg``.

  One parameter, ``item_weights`` [num_items, num_items], dense storage of the sparse iterate, zero until fitted; the
  five hyperparameters travel in ``model_params()``.  The defaults are the best Recall@20 on the ML-20M slice among
  the grid's cells read after 25 or 50 iterations, at the fewest iterations that reach it (profiles/admm_bench.jsonl;
  the reads after 10 iterations are still moving).  Gradient training would keep neither the zero diagonal nor the zeros:
  ``Recoder.train`` refuses this model and points at ``train_admm_slim``.
  """
  fit_method = "train_admm_slim"
  fit_sentence = ("an AdmmSlimModel is fitted by ADMM on the Gram matrix: call %s(train_dataset) "
                  "(gradient steps would keep neither its zero diagonal nor its zeros)")

  def __init__(self, l1_reg=0.25, l2_reg=2000.0, rho=2000.0, num_iterations=25, nonneg=False):
    super().__init__()
    self.l1_reg, self.l2_reg, self.rho, self.num_iterations, self.nonneg = l1_reg, l2_reg, rho, num_iterations, nonneg
    self.num_items = None
    self.item_weights = None
    self._validate()

  def _validate(self):
    from .admm import check_params
    self.l1_reg, self.l2_reg, self.rho, self.num_iterations, self.nonneg = check_params(
        self.l1_reg, self.l2_reg, self.rho, self.num_iterations, self.nonneg)

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.item_weights = nn.Parameter(torch.zeros(num_items, num_items), requires_grad=False)

  def model_params(self):
    return {"l1_reg": float(self.l1_reg), "l2_reg": float(self.l2_reg), "rho": float(self.rho),
            "num_iterations": int(self.num_iterations), "nonneg": bool(self.nonneg)}

  def load_model_params(self, model_params):
    self.l1_reg, self.l2_reg, self.rho = (float(model_params[k]) for k in ("l1_reg", "l2_reg", "rho"))
    self.num_iterations, self.nonneg = int(model_params["num_iterations"]), bool(model_params["nonneg"])
    self._validate()

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    from . import ease
    return ease.scores(csr, self.item_weights.data, lo, hi, out=out, ld=ld, n_rows=n_rows)     # (rk_ease_scores)

  def _dense_w(self):
    return self.item_weights


class LowRankShallowAutoencoder(CsrScoresModel):
  """ELSA (Vancura, Alves, Kasalicky & Kordik 2022, "Scalable Linear Shallow Autoencoder for Collaborative
  Filtering"): the EASE-like autoencoder ``scores = input @ (A A^T - I)`` whose item-item matrix is never formed: A
  [num_items, embedding_size] holds the rows of ``item_factors`` at unit length, ``A_j = W_j / max(|W_j|, 1e-12)``, so
  the diagonal of ``A A^T`` is 1 and the model is 4 n h bytes where EASE, GF-CF and ADMM-SLIM are 4 n^2.  Trained by
  ``Recoder.train_elsa`` (recoder_amd/elsa.py): mini-batch Adam steps on the cosine loss of the published code, computed
  from the h x h Gram ``A^T A`` without the batch x items prediction block.

  One parameter, ``item_factors`` [num_items, embedding_size], which is W, zero until fitted; ``embedding_size`` (1..512)
  travels in ``model_params()``.  A and its transpose are derived state: taken again after a fit and after a checkpoint
  is loaded, and not part of ``state_dict()``.  The defaults (embedding_size 256 here; 5 epochs, lr 0.03 and batches of
  1024 in ``train_elsa``) are the best Recall@20 of the float64 grid on the ML-20M slice, embedding_size {64, 256} x lr
  {0.03, 0.1, 0.3} read after 5, 10 and 20 epochs, at the fewest epochs that reach it: 0.1365, against 0.1357 after 10
  epochs and 0.1285 after 20 at the same cell, which overfits from there, and 0.1350 at lr 0.1 after 10
  (profiles/elsa_quality.jsonl; tools/elsa_bench.py --cpu-grid).  ``Recoder.train`` refuses this model and
  points at ``train_elsa``: its loss is not one of the fused epilogues, and its step is not the encoder-decoder one.
  """
  fit_method = "train_elsa"
  fit_sentence = ("a LowRankShallowAutoencoder is trained by its own mini-batch steps on the cosine loss, from the "
                  "Gram matrix of its factors: call %s(train_dataset)")

  def __init__(self, embedding_size=256):
    super().__init__()
    self.embedding_size = embedding_size
    self.num_items = None
    self.item_factors = None
    self._images = None            # (A, A^T) of item_factors, and what they were taken from
    self._batch = None             # (the csr of the last batch, its rows, Z = X_b A)
    self._validate()

  def _validate(self):
    from .elsa import check_embedding_size
    self.embedding_size = check_embedding_size(self.embedding_size)

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.item_factors = nn.Parameter(torch.zeros(num_items, self.embedding_size), requires_grad=False)
    self._weights_written()

  def model_params(self):
    return {"embedding_size": int(self.embedding_size)}

  def load_model_params(self, model_params):
    self.embedding_size = model_params["embedding_size"]
    self._validate()

  def _weights_written(self):
    """``item_factors`` was written: the normalised images and the last batch's Z are taken again on next use."""
    self._images = self._batch = None

  def _load_from_state_dict(self, *args, **kwargs):
    self._weights_written()
    return super()._load_from_state_dict(*args, **kwargs)

  def images(self):
    """(A [n, h], A^T [h, n]) of ``item_factors`` on its device (rk_ease_elsa_normalize), kept until the factors are
    written again."""
    from . import elsa
    W = self.item_factors.data
    key = (W.data_ptr(), W.device)               # (a move or a re-allocation; a write in place is _weights_written's to tell)
    if self._images is None or self._images[0] != key:
      At = torch.empty(W.shape[1], W.shape[0], dtype=torch.float32, device=W.device)
      A, _ = elsa.normalize(W.contiguous(), At=At)
      self._images, self._batch = (key, A, At), None
    return self._images[1:]

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    """Z = (the rows of ``csr``) @ A once per ``csr`` object (rk_ease_scores), then the strip Z @ A^T[:, lo:hi]
    (rk_ease_gemm) minus the strip's stored entries (rk_ease_csr_sub)."""
    from . import _ease_lib, ease, elsa
    from ._lib import ptr
    from .device import current_stream
    A, At = self.images()
    n, h = A.shape
    if out is None:
      ld = hi - lo if ld is None else ld
      out = torch.empty(n_rows, ld, dtype=torch.float32, device=A.device)
    ld = out.stride(0) if ld is None else ld
    if n_rows == 0:
      return out
    b = self._batch
    if b is None or b[0] is not csr or b[1] != n_rows:
      b = self._batch = (csr, n_rows, ease.scores(csr, A, 0, h, n_rows=n_rows))
    Z = b[2]
    _ease_lib.check(_ease_lib.load().rk_ease_gemm(ptr(Z), h, At.data_ptr() + 4 * lo, n, None, 0, ptr(out), ld, n_rows,
                                                  hi - lo, h, 1.0, 0.0, 0, n_rows, current_stream()), "rk_ease_gemm")
    return elsa.csr_sub(csr, lo, hi, out, ld, n_rows)

  def torch_forward(self, input, input_users=None, input_items=None, target_users=None,
                    target_items=None):
    """The same forward in torch ops (the generic engine's validation loss; host tensors)."""
    W = self.item_factors
    A = W / W.norm(dim=1, keepdim=True).clamp_min(1e-12)
    x = input.to(A.dtype)
    if input_items is not None:
      full = torch.zeros(x.shape[0], A.shape[0], dtype=A.dtype, device=x.device)
      full[:, input_items.to(torch.int64)] = x
      x = full
    out = (x @ A) @ A.t() - x
    return out if target_items is None else out.index_select(1, target_items.to(torch.int64))


class _NeighbourListModel(ItemItemModel):
  """An item-item model stored as neighbour lists: ``item_neighbours`` int32 [num_items, neighbours],
  ``item_weights`` f32 of the same shape and ``neighbour_counts`` int32 [num_items].  A subclass names
  ``fit_module``, the module of this package whose ``scores`` reads the lists, and says in
  ``lists_spell_columns`` which way round they spell W: row j of the tensors is row j of W,
  ``W[j, item_neighbours[j, s]] = item_weights[j, s]``, or (True) column j."""
  fit_module = None
  lists_spell_columns = False

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.allocate(self.neighbours, None)

  def allocate(self, neighbours, device):
    """(Re-)create the three tensors for ``neighbours`` entries per item: no neighbours, zero weights."""
    n, K = self.num_items, int(neighbours)
    self.neighbours = K
    self._buffers.pop("item_neighbours", None)
    self._buffers.pop("neighbour_counts", None)
    self.register_buffer("item_neighbours", torch.full((n, K), -1, dtype=torch.int32, device=device))
    self.item_weights = nn.Parameter(torch.zeros(n, K, device=device), requires_grad=False)
    self.register_buffer("neighbour_counts", torch.zeros(n, dtype=torch.int32, device=device))

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    from importlib import import_module
    fit = import_module("." + self.fit_module, __package__)     # (rk_rp3_scores / rk_slim_scores)
    return fit.scores(csr, self.item_neighbours, self.item_weights.data, self.neighbour_counts, lo, hi, out=out,
                      ld=ld, n_rows=n_rows)

  def dense_weights(self, dtype=torch.float32):
    """W [num_items, num_items]: the kept entries scattered into a dense matrix (small catalogues only)."""
    n, K = self.item_weights.shape
    W = torch.zeros(n, n, dtype=dtype, device=self.item_weights.device)
    ids = self.item_neighbours.to(torch.int64)
    live = torch.arange(K, device=ids.device)[None, :] < self.neighbour_counts.to(torch.int64)[:, None]
    own = torch.arange(n, device=ids.device)[:, None].expand(n, K)
    rows, cols = (ids, own) if self.lists_spell_columns else (own, ids)
    W[rows[live], cols[live]] = self.item_weights.data.to(dtype)[live]
    return W

  def _dense_w(self):
    return self.dense_weights()


class RandomWalkItemModel(_NeighbourListModel):
  """RP3beta (Paudel, Christoffel, Newell & Bernstein 2016): a sparse item-item model from three-step
  random walks on the user-item graph, ``scores = input @ W`` with
  ``W[i, j] = d_i^-alpha * (sum over the users v of i and j of r_v^-alpha) * d_j^-beta`` off the diagonal,
  every row cut to its ``neighbours`` largest entries, fitted by ``Recoder.train_rp3beta``
  (recoder_amd/rp3.py).  ``beta`` is the popularity penalty and matters: too large a value ranks by
  rarity alone.

  Three tensors, all in ``state_dict()``: ``item_neighbours`` int32 [num_items, neighbours] (the kept j
  of every row, ascending, -1 where a row has fewer), ``item_weights`` f32 of the same shape and
  ``neighbour_counts`` int32 [num_items]; empty until fitted.  ``alpha``, ``beta`` and ``neighbours``
  travel in ``model_params()``.  The fit is closed-form: ``Recoder.train`` refuses this model and points
  at ``train_rp3beta``.
  """
  fit_module = "rp3"
  fit_method = "train_rp3beta"
  fit_sentence = "a RandomWalkItemModel is fitted in closed form from the interaction graph: call %s(train_dataset)"

  def __init__(self, alpha=0.6, beta=0.3, neighbours=100):
    super().__init__()
    self.alpha = alpha
    self.beta = beta
    self.neighbours = neighbours
    self.num_items = None
    self.item_weights = None
    self._validate()

  def _validate(self):
    from .rp3 import check_params
    self.alpha, self.beta, self.neighbours = check_params(self.alpha, self.beta, self.neighbours)

  def model_params(self):
    return {"alpha": float(self.alpha), "beta": float(self.beta), "neighbours": int(self.neighbours)}

  def load_model_params(self, model_params):
    self.alpha = float(model_params["alpha"])
    self.beta = float(model_params["beta"])
    self.neighbours = int(model_params["neighbours"])
    self._validate()


class _ColumnListModel(_NeighbourListModel):
  """The neighbour-list models whose lists spell the COLUMNS of W: row j of the three tensors holds the kept k
  of column j, ``W[item_neighbours[j, s], j] = item_weights[j, s]`` (the layout rk_slim_scores reads)."""
  lists_spell_columns = True


class SparseLinearModel(_ColumnListModel):
  """SLIM (Ning & Karypis 2011): the learned sparse item-item model ``scores = input @ W``, column j of W
  the non-negative elastic-net regression of item j on the other items,
  ``min over w >= 0, w_j = 0 of 1/2 |x_j - X w|^2 + l2_reg/2 |w|^2 + l1_reg |w|_1``, cut to its ``neighbours``
  largest entries, fitted by coordinate descent on the Gram by ``Recoder.train_slim`` (recoder_amd/slim.py).
  ``l1_reg`` decides the sparsity (a pair of items fewer than ``l1_reg`` users share, weighted by their
  values, never gets a weight), ``l2_reg`` the shrinkage.  scikit-learn's ``ElasticNet(alpha, l1_ratio,
  positive=True)`` over U users is ``l1_reg = U * alpha * l1_ratio``, ``l2_reg = U * alpha * (1 - l1_ratio)``.

  Three tensors, all in ``state_dict()``, laid out as ``RandomWalkItemModel``'s but per COLUMN of W:
  ``item_neighbours`` int32 [num_items, neighbours] (the kept k of column j, ascending, -1 where a column
  has fewer), ``item_weights`` f32 of the same shape (``W[k, j]``) and ``neighbour_counts`` int32
  [num_items]; empty until fitted.  ``l1_reg``, ``l2_reg`` and ``neighbours`` travel in ``model_params()``, and
  so do ``candidates``, ``candidate_similarity`` and ``candidate_shrink`` after an fsSLIM fit
  (``train_slim(candidates=M)``; ``candidates`` is None otherwise and then none of the three is listed).
  ``Recoder.train`` refuses this model and points at ``train_slim``.
  """
  fit_module = "slim"
  fit_method = "train_slim"
  fit_sentence = "a SparseLinearModel is fitted by coordinate descent on the Gram matrix: call %s(train_dataset)"

  def __init__(self, l1_reg=1.0, l2_reg=1000.0, neighbours=200):
    super().__init__()
    self.l1_reg = l1_reg
    self.l2_reg = l2_reg
    self.neighbours = neighbours
    # (what the last ``train_slim`` restricted the columns to: None, or fsSLIM's candidate lists)
    self.candidates, self.candidate_similarity, self.candidate_shrink = None, "cosine", 0.0
    self.num_items = None
    self.item_weights = None
    self._validate()

  def _validate(self):
    from .slim import check_candidates, check_params
    self.l1_reg, self.l2_reg, self.neighbours = check_params(self.l1_reg, self.l2_reg, self.neighbours)[:3]
    self.candidates, self.candidate_similarity, self.candidate_shrink = check_candidates(
        self.candidates, self.candidate_similarity, self.candidate_shrink)

  def model_params(self):
    params = {"l1_reg": float(self.l1_reg), "l2_reg": float(self.l2_reg), "neighbours": int(self.neighbours)}
    if self.candidates is not None:
      params.update(candidates=int(self.candidates), candidate_similarity=self.candidate_similarity,
                    candidate_shrink=float(self.candidate_shrink))
    return params

  def load_model_params(self, model_params):
    self.l1_reg = float(model_params["l1_reg"])
    self.l2_reg = float(model_params["l2_reg"])
    self.neighbours = int(model_params["neighbours"])
    self.candidates = model_params.get("candidates")
    self.candidate_similarity = model_params.get("candidate_similarity", "cosine")
    self.candidate_shrink = model_params.get("candidate_shrink", 0.0)
    self._validate()


class ItemNeighbourhoodModel(_ColumnListModel):
  """ItemKNN (the shrunk item-neighbourhood baseline of Dacrema et al. 2019): ``scores = input @ W``, column j
  of W the ``neighbours`` items most similar to item j, ``W[i, j] = s_ij / (denominator + shrink)`` with
  ``s_ij = sum over the users v of i and j of a_vi a_vj``, fitted by ``Recoder.train_itemknn``
  (recoder_amd/itemknn.py).  ``similarity``: "cosine" (``|a_i| |a_j|``), "asymmetric" (Aiolli 2013:
  ``|a_j|^(2(1 - asymmetric_alpha)) |a_i|^(2 asymmetric_alpha)``), or, on the binary matrix, "tversky"
  (``s + tversky_alpha |i \\ j| + tversky_beta |j \\ i|``), "jaccard" (alpha = beta = 1) and "dice" (alpha = beta =
  1/2).  ``feature_weighting`` ("none", "tfidf", "bm25") re-weights the stored values for the two cosines.
  ``shrink`` **matters**: without it a pair that one user shares gets similarity 1 and the model ranks far
  below popularity on sparse data.

  Three tensors, all in ``state_dict()``, laid out as ``SparseLinearModel``'s, per COLUMN of W:
  ``item_neighbours`` int32 [num_items, neighbours] (the kept i of column j, ascending, -1 where a column has
  fewer), ``item_weights`` f32 of the same shape and ``neighbour_counts`` int32 [num_items]; empty until
  fitted.  The seven settings travel in ``model_params()``.  ``Recoder.train`` refuses this model and points
  at ``train_itemknn``.
  """
  fit_module = "itemknn"
  fit_method = "train_itemknn"
  fit_sentence = ("an ItemNeighbourhoodModel is fitted in closed form from the items' co-occurrences: call "
                  "%s(train_dataset)")
  _PARAMS = ("neighbours", "shrink", "similarity", "feature_weighting", "asymmetric_alpha", "tversky_alpha",
             "tversky_beta")

  def __init__(self, neighbours=200, shrink=300.0, similarity="cosine", feature_weighting="none",
               asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0):
    super().__init__()
    self.neighbours = neighbours
    self.shrink = shrink
    self.similarity = similarity
    self.feature_weighting = feature_weighting
    self.asymmetric_alpha = asymmetric_alpha
    self.tversky_alpha = tversky_alpha
    self.tversky_beta = tversky_beta
    self.num_items = None
    self.item_weights = None
    self._validate()

  def _validate(self):
    from .itemknn import check_params
    for name, v in zip(self._PARAMS, check_params(*(getattr(self, name) for name in self._PARAMS))):
      setattr(self, name, v)

  def model_params(self):
    return {name: getattr(self, name) for name in self._PARAMS}

  def load_model_params(self, model_params):
    for name in self._PARAMS:
      setattr(self, name, model_params[name])
    self._validate()


class UserNeighbourhoodModel(CsrScoresModel):
  """UserKNN: user-based cosine neighbourhoods over the training matrix X (recoder_amd/userknn.py).  A query's
  similarity to training user v is ``|H_q and H_v| / (sqrt(|H_q|) sqrt(|H_v|) + shrink)`` over the item SETS
  (values play no part), it keeps its ``neighbours`` most similar users (ties to the lower ids) and its scores
  are ``sum over them of sim * X[v, :]`` with the stored training values.  Neighbours are found at serving
  time from the history the caller passes, so users the fit has never seen are served like any other.  A
  training user identical to the query is not excluded: it takes one of the slots and contributes only
  items that the masked top-k removes.

  The model IS the training matrix, "fitted" by ``Recoder.train_userknn``: both of its CSRs
  (``user_indptr`` int64 [num_users + 1], ``user_indices`` int32 [nnz]; ``item_indptr`` int64
  [num_items + 1], ``item_indices`` int32 [nnz]) and ``user_norms`` f32 [num_users] are buffers and
  ``interaction_values`` f32 [nnz] (user-major order) is the one parameter, so all six are in
  ``state_dict()``; empty until fitted.  ``neighbours`` and ``shrink`` travel in ``model_params()``, with the
  sizes a checkpoint's tensors have.  ``Recoder.train`` refuses this model and points at ``train_userknn``.
  """
  fit_method = "train_userknn"
  fit_sentence = ("a UserNeighbourhoodModel is its training matrix, there is nothing to descend on: call "
                  "%s(train_dataset)")

  def __init__(self, neighbours=400, shrink=10.0):
    super().__init__()
    self.neighbours = neighbours
    self.shrink = shrink
    self.num_items = self.num_users = None
    self.nnz = 0
    self.interaction_values = None
    self.neighbour_passes = 0      # rk_rp3_user_neighbours calls so far (one per batch, whatever the strips)
    self._batch = None             # (the csr of the last batch, its rows, its neighbour lists, the workspace)
    self._validate()

  def _validate(self):
    from .userknn import check_params
    self.neighbours, self.shrink = check_params(self.neighbours, self.shrink)

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_items = num_items
    self.allocate(self.num_users if num_users is None else num_users, self.nnz, None)

  def allocate(self, num_users, nnz, device):
    """(Re-)create the six tensors for ``num_users`` users and ``nnz`` entries: an empty matrix."""
    U, n, nnz = int(num_users or 0), int(self.num_items), int(nnz)
    self.num_users, self.nnz, self._batch = U, nnz, None
    for name in ("user_indptr", "user_indices", "item_indptr", "item_indices", "user_norms"):
      self._buffers.pop(name, None)
    self.register_buffer("user_indptr", torch.zeros(U + 1, dtype=torch.int64, device=device))
    self.register_buffer("user_indices", torch.zeros(max(1, nnz), dtype=torch.int32, device=device))
    self.register_buffer("item_indptr", torch.zeros(n + 1, dtype=torch.int64, device=device))
    self.register_buffer("item_indices", torch.zeros(max(1, nnz), dtype=torch.int32, device=device))
    self.register_buffer("user_norms", torch.zeros(U, dtype=torch.float32, device=device))
    self.interaction_values = nn.Parameter(torch.zeros(max(1, nnz), device=device), requires_grad=False)

  def store(self, ucsr, icsr, un):
    """Copy the (user-major, item-major) device CSR pair of X and the users' norms into the tensors."""
    assert ucsr.shape == (self.num_users, self.num_items) and ucsr.nnz == self.nnz
    self.user_indptr.copy_(ucsr.indptr)
    self.item_indptr.copy_(icsr.indptr)
    self.user_indices.copy_(ucsr.indices)
    self.item_indices.copy_(icsr.indices)
    self.user_norms.copy_(un)
    if ucsr.data is None:
      self.interaction_values.data.fill_(1.0)
    else:
      self.interaction_values.data.copy_(ucsr.data)
    self._batch = None

  def model_params(self):
    return {"neighbours": int(self.neighbours), "shrink": float(self.shrink), "num_users": self.num_users,
            "nnz": int(self.nnz)}

  def load_model_params(self, model_params):
    self.neighbours = int(model_params["neighbours"])
    self.shrink = float(model_params["shrink"])
    self.num_users = model_params.get("num_users")
    self.nnz = int(model_params.get("nnz", 0))
    self._validate()

  def _load_from_state_dict(self, *args, **kwargs):
    self._batch = None
    return super()._load_from_state_dict(*args, **kwargs)

  def _csrs(self):
    from types import SimpleNamespace
    U, n = self.num_users, self.num_items
    return (SimpleNamespace(indptr=self.user_indptr, indices=self.user_indices, data=self.interaction_values.data,
                            shape=(U, n)),
            SimpleNamespace(indptr=self.item_indptr, indices=self.item_indices, data=None, shape=(n, U)))

  def batch_neighbours(self, csr, n_rows=None):
    """(ids, sim, count) of the rows of ``csr``: computed once per ``csr`` object (rk_rp3_user_neighbours) and
    kept until another batch arrives, so that the strips of one batch share them."""
    from . import userknn
    n_rows = csr.shape[0] if n_rows is None else n_rows
    b = self._batch
    if b is not None and b[0] is csr and b[1] == n_rows:
      return b[2]
    qn = userknn.query_norms(csr)
    *nbr, ws = userknn.neighbours(csr, self._csrs()[1], self.user_norms, self.neighbours, self.shrink, qn=qn,
                                  row_hi=n_rows, ws=None if b is None else b[3])
    self.neighbour_passes += 1
    self._batch = (csr, n_rows, tuple(nbr), ws)
    return self._batch[2]

  def csr_scores(self, csr, lo, hi, out, ld, n_rows):
    from . import userknn
    if not self.num_users:
      raise ValueError("the UserNeighbourhoodModel holds no training matrix: call train_userknn first")
    nbr = self.batch_neighbours(csr, n_rows)
    return userknn.scores(nbr, self._csrs()[0], lo, hi, out=out, ld=ld, n_rows=n_rows)    # (rk_rp3_user_scores)

  def torch_forward(self, input, input_users=None, input_items=None, target_users=None,
                    target_items=None):
    """The same model in torch ops on the dense X (small matrices only; host tensors): f32 similarities,
    a stable descending sort for the cut, a dense product for the scores."""
    U, n = self.num_users, self.num_items
    dev = input.device
    rows = torch.repeat_interleave(torch.arange(U, device=dev), self.user_indptr[1:] - self.user_indptr[:-1])
    cols = self.user_indices[:self.nnz].to(torch.int64)
    X = torch.zeros(U, n, dtype=torch.float32, device=dev)
    X[rows, cols] = self.interaction_values.data[:self.nnz].to(torch.float32)
    B = torch.zeros(U, n, dtype=torch.float32, device=dev)
    B[rows, cols] = 1.0
    H = torch.zeros(input.shape[0], n, dtype=torch.float32, device=dev)
    nz = (input != 0).to(torch.float32)
    if input_items is None:
      H[:, :nz.shape[1]] = nz
    else:
      H[:, input_items.to(torch.int64)] = nz
    qn = torch.sqrt(H.sum(1).double()).float()
    c = H @ B.t()
    sim = torch.where(c > 0, c / (qn[:, None] * self.user_norms[None, :] + self.shrink), torch.zeros_like(c))
    order = torch.sort(sim, dim=1, descending=True, stable=True)[1][:, :self.neighbours]
    kept = torch.zeros_like(sim).scatter_(1, order, sim.gather(1, order))
    out = kept @ X
    return out if target_items is None else out.index_select(1, target_items.to(torch.int64))


class NeuralMatrixFactorization(FactorizationModel):
  """NeuMF, the fusion of GMF and an MLP of Neural Collaborative Filtering (He, Liao, Zhang, Nie, Hu & Chua, WWW 2017):

      s(u, i) = w[:dg] . (Pg[u] o Qg[i]) + w[dg:] . phi_L + b0,  phi_0 = [Pm[u] ; Qm[i]],  phi_l = relu(W_l phi_{l-1} + c_l)

  the one model here whose score is neither a dot product nor a function of the user's row.  Parameters: the GMF tables
  ``Pg`` [users, dg] and ``Qg`` [items, dg] (dg = ``embedding_size``), the MLP tables ``Pm`` [users, dm] and ``Qm``
  [items, dm] (dm = ``mlp_embedding_size``), the layers ``mlp_weights[l]`` [d_l, d_{l-1}] (d_0 = 2 dm) and
  ``mlp_biases[l]`` [d_l] for the 1..3 widths of ``mlp_layers``, and the output layer ``w`` [dg + d_L], ``b0`` [1].
  Every size is a multiple of 4 in 4..128 and the layers' weights fit a workgroup's LDS together (``ncf.check_sizes``).
  ``init_model`` draws as the paper: N(0, 0.01) tables, Xavier-uniform W_l, zero biases, ``w`` as a [1, dg + d_L]
  linear layer -- on the host, from a ``torch.Generator`` seeded by ``init_seed`` (``Recoder.train_ncf`` sets it to the
  fit's ``seed`` before the model is initialised).  Trained by ``Recoder.train_ncf`` (recoder_amd/ncf.py), which
  ``Recoder.train`` points at.  Scores come from user ids: ``user_scores`` runs rk_als_ncf_scores over a strip, with the
  items' half of layer 1 (``A`` = Qm W_1[:, dm:]^T, rk_als_ncf_item_part) and the packed dense parameters kept until
  the parameters are written again (``_weights_written``).  ``forward`` on the host is the differentiable
  ``torch_forward``; on the device it is the scores kernel, without autograd."""
  fit_method = "train_ncf"
  fit_sentence = ("a NeuralMatrixFactorization is trained on sampled (user, item) pairs under the binary "
                  "cross-entropy, by its own HIP step: call %s(train_dataset)")

  def __init__(self, embedding_size=32, mlp_embedding_size=32, mlp_layers=(64, 32, 16)):
    super().__init__()
    self.embedding_size = embedding_size
    self.mlp_embedding_size = mlp_embedding_size
    self.mlp_layers = mlp_layers
    self.init_seed = 0
    self.num_users = self.num_items = None
    self.Pg = self.Qg = self.Pm = self.Qm = self.w = self.b0 = None
    self.mlp_weights = self.mlp_biases = None
    self._derived = None             # (A, theta) of the parameters as last written
    self._validate()

  def _validate(self):
    from .ncf import check_sizes
    self.embedding_size, self.mlp_embedding_size, self.mlp_layers = check_sizes(
        self.embedding_size, self.mlp_embedding_size, self.mlp_layers)

  def sizes(self):
    return (self.embedding_size, self.mlp_embedding_size, tuple(self.mlp_layers))

  def init_model(self, num_items=None, num_users=None):
    self._validate()
    self.num_users, self.num_items = num_users, num_items
    dg, dm, layers = self.sizes()
    gen = torch.Generator().manual_seed(int(self.init_seed) % (2 ** 63))

    def table(rows, d):
      return nn.Parameter(torch.empty(rows, d).normal_(0.0, 0.01, generator=gen), requires_grad=False)
    self.Pg, self.Qg = table(num_users, dg), table(num_items, dg)
    self.Pm, self.Qm = table(num_users, dm), table(num_items, dm)

    def xavier(rows, cols):                                    # (Xavier-uniform of a [rows, cols] linear layer)
      bound = (6.0 / (rows + cols)) ** 0.5
      return nn.Parameter((torch.rand(rows, cols, generator=gen) * 2 - 1) * bound, requires_grad=False)
    ws, cs, prev = [], [], 2 * dm
    for d in layers:
      ws.append(xavier(d, prev))
      cs.append(nn.Parameter(torch.zeros(d), requires_grad=False))
      prev = d
    self.mlp_weights, self.mlp_biases = nn.ParameterList(ws), nn.ParameterList(cs)
    self.w = nn.Parameter(xavier(1, dg + prev).data.reshape(-1), requires_grad=False)
    self.b0 = nn.Parameter(torch.zeros(1), requires_grad=False)
    self._weights_written()

  def model_params(self):
    return {"embedding_size": int(self.embedding_size), "mlp_embedding_size": int(self.mlp_embedding_size),
            "mlp_layers": [int(d) for d in self.mlp_layers]}

  def load_model_params(self, model_params):
    self.embedding_size = model_params["embedding_size"]
    self.mlp_embedding_size = model_params["mlp_embedding_size"]
    self.mlp_layers = tuple(model_params["mlp_layers"])
    self._validate()

  def _weights_written(self):
    """A parameter was written: the items' half of layer 1 and the packed dense parameters are taken again."""
    self._derived = None

  def _load_from_state_dict(self, *args, **kwargs):
    self._weights_written()
    return super()._load_from_state_dict(*args, **kwargs)

  def derived(self):
    """(A [items, d1], theta) on the parameters' device, kept until ``_weights_written``."""
    from . import ncf
    key = (self.Qm.data_ptr(), self.Qm.device)
    if self._derived is None or self._derived[0] != key:
      theta = ncf.pack(self)[2]
      self._derived = (key, ncf.item_part(self.Qm.data, theta, self.sizes()), theta)
    return self._derived[1:]

  def user_scores(self, users, lo, hi, out=None, ld=None):
    """out[b, c] = s(users[b], lo + c) for c < hi - lo, ``out`` f32 with row stride ``ld`` (None: a new [B, hi - lo]
    tensor); ``users`` are ids on the device, each in [0, num_users) -- the caller checks that."""
    from . import ncf
    A, theta = self.derived()
    users = users.to(torch.int32).contiguous()
    if out is None:
      ld = hi - lo if ld is None else ld
      out = torch.empty(users.shape[0], ld, dtype=torch.float32, device=A.device)
    ld = out.stride(0) if ld is None else ld
    if users.shape[0] == 0:
      return out
    return ncf.scores(users, lo, hi, self.Pg.data, self.Qg.data, self.Pm.data, A, theta, self.sizes(), out, ld)

  def forward(self, input, input_users=None, input_items=None, target_users=None,
              target_items=None):
    if not self.Pg.is_cuda:
      return self.torch_forward(input, input_users, input_items, target_users, target_items)
    out = self.user_scores(input_users, 0, self.num_items)
    return out if target_items is None else out.index_select(1, target_items.to(torch.int64))

  def torch_forward(self, input, input_users=None, input_items=None, target_users=None,
                    target_items=None):
    """The same scores in torch ops, differentiable: [B, items] (or [B, len(target_items)])."""
    u = input_users.to(torch.int64)
    items = torch.arange(self.Qg.shape[0], device=u.device) if target_items is None else target_items.to(torch.int64)
    dg = self.Pg.shape[1]
    gmf = (self.Pg[u] * self.w[:dg]) @ self.Qg[items].t()
    dm = self.Pm.shape[1]
    W1 = self.mlp_weights[0]
    x = (self.Pm[u] @ W1[:, :dm].t() + self.mlp_biases[0])[:, None, :] + (self.Qm[items] @ W1[:, dm:].t())[None, :, :]
    x = torch.relu(x)
    for W, c in zip(list(self.mlp_weights)[1:], list(self.mlp_biases)[1:]):
      x = torch.relu(x @ W.t() + c)
    return gmf + x @ self.w[dg:] + self.b0
