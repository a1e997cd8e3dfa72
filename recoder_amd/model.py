"""``Recoder``: the reference's trainer API (recoder/model.py:22-559) on the
MI355X hot path.

Same constructor, ``train`` signature, public attributes, checkpoint dict and
error behaviour as the reference; the body of the hot loop
(model.py:383-404) is ``FusedEngine.train_step`` (HIP kernels) over batches
collated on the device, with no per-step host synchronisation: the per-step
losses are left in a device buffer and read once per epoch.

Two hooks exist because a GPU cannot reproduce the reference's CPU RNG streams
(SURVEY section 7 "RNG parity"):
  ``user_order_hook(epoch, n_users) -> int64 array | None``  the user order of
      an epoch (default: the same draw ``RandomSampler`` makes from the global
      torch RNG, so noise-free runs reproduce the reference's order);
  ``mask_hook(step, users, nnz) -> (keep_noise | None, keep_drop | None)``
      explicit dropout keep-masks for a sampling group (default: counter RNG).
  ``eps_hook(step, users) -> float32 [rows, d] | None``  VariationalAutoencoder: the eps of the
      bottleneck sample of training step ``step`` whose rows are ``users`` (default: counter RNG).
Either hook turns the HIP-graph replay of the training steps off.
"""
import functools
import logging
import os

import numpy as np
import torch
import torch.optim as optim
from torch.optim.lr_scheduler import MultiStepLR

from . import __version__
from .data import (BatchCollator, RecommendationDataLoader, RecommendationDataset,
                   epoch_user_order)
from .device import Block, DeviceCSR, require_gpu
from .engine import FusedEngine
from .losses import MSELoss, MultinomialNLLLoss
from .metrics import RecommenderEvaluator
from .nn import (CsrScoresModel, DynamicAutoencoder, FactorizationModel, MatrixFactorization,
                 NeuralMatrixFactorization,
                 VariationalAutoencoder)
from .recommender import InferenceRecommender

log = logging.getLogger("recoder_amd")


def _default(value, model, name):
  """``value``, or the model's ``name`` where it is None.  On a model of another class, which may lack the
  attribute, that stays None: the fit module's check_config refuses the class before it looks at a number."""
  return getattr(model, name, None) if value is None else value


def _mf_tables(m):
  return m.user_embedding_layer.weight.data, m.item_embedding_layer.weight.data


def _top_sum(degrees, k):
  d = np.asarray(degrees)
  if len(d) <= k:
    return int(d.sum())
  return int(np.partition(d, len(d) - k)[len(d) - k:].sum())


class Recoder(object):
  """Trains / evaluates a :class:`recoder_amd.nn.FactorizationModel`
  (arguments as model.py:26-47)."""

  def __init__(self, model: FactorizationModel, num_items=None, num_users=None,
               optimizer_type="sgd", loss="mse", loss_params=None, use_cuda=False,
               user_based=True, item_based=True):
    self.model = model
    self.num_items = num_items
    self.num_users = num_users
    self.optimizer_type = optimizer_type
    self.loss = loss
    self.loss_params = loss_params if loss_params else {}
    self.use_cuda = use_cuda
    self.user_based = user_based
    self.item_based = item_based
    # this build has exactly one device: the MI355X PyTorch-ROCm exposes as
    # 'cuda'.  use_cuda is kept for signature compatibility.
    self.device = torch.device("cuda")
    self.optimizer = None
    self.sparse_optimizer = None
    self.current_epoch = 1
    self.items = None
    self.users = None
    self.user_order_hook = None
    self.mask_hook = None
    self.eps_hook = None
    # steps collated per side-stream hand-over (CollatePrefetcher)
    self.prefetch_group = 4
    # steps per replayed HIP graph (graph.py)
    self.graph_group = int(os.environ.get("RK_GRAPH_GROUP", "8"))
    # {global step index: callable}: called right before that step's collation is submitted and
    # its kernels are enqueued (the pipeline is cut there: nothing of the step is in flight yet);
    # returning True ends the training.  bench.py brackets its timed region with two of these.
    self.step_marks = {}
    self.last_epoch_losses = None
    self.loss_history = []      # per-epoch arrays of the per-step training losses
    self.als_history = []       # train_als: the ALS objective after each iteration
    self.ials_history = []      # train_ials: the iALS++ objective after each sweep
    self.bpr_history = []       # train_bpr: the mean loss per valid triple of each epoch
    self.warp_history = []      # train_warp: the mean loss per valid slot of each epoch
    self.warp_stats = []        # train_warp: (share of slots with a violator, their mean trials) of each epoch
    self.lightgcn_history = []  # train_lightgcn: the mean loss per valid triple of each epoch
    self.lightgcn_state = None  # train_lightgcn: base tables, Adam moments, step count, num_layers (device; not saved)
    self.simgcl_history = []    # train_simgcl: (mean BPR loss per valid triple, mean NCE per step) of each epoch
    self.simgcl_state = None    # train_simgcl: base tables, Adam moments, step count, num_layers (device; not saved)
    self.directau_history = []  # train_directau: (alignment, uniformity users, uniformity items) means of each epoch
    self.directau_state = None  # train_directau: base tables, Adam moments, step count, num_layers (device; not saved)
    self.ssm_history = []       # train_ssm: (mean loss, mean probability of the positive) per step, of each epoch
    self.ssm_state = None       # train_ssm: base tables, Adam moments, step count, num_layers (device; not saved)
    self.ultragcn_history = []  # train_ultragcn: (positive, negatives, neighbours) means per valid slot of each epoch
    self.ultragcn_state = None  # train_ultragcn: the tables, Adam moments and step count (device; not saved)
    self.ccl_history = []       # train_ccl: (positive term, negative term) means per valid slot of each epoch
    self.ccl_stats = []         # train_ccl: the mean share of live negatives of each epoch
    self.ccl_state = None       # train_ccl: base tables, Adam moments, step count, num_layers (device; not saved)
    self.simplex_history = []   # train_simplex: (positive term, negative term) means per valid slot of each epoch
    self.simplex_stats = []     # train_simplex: the mean share of live negatives of each epoch
    self.simplex_state = None   # train_simplex: P, Q, W, Adam moments, step count, gamma, max_history (device; not saved)
    # the iterative trainers' validation curve of the last fit (None: it had no val_dataset): {"metric", "k",
    # "values", "epochs", "best_epoch", "stopped_epoch"}; not saved
    self.fit_validation = None  # validation settings for the iterative fits called without a val_dataset (_validated)
    self.bpr_validation = self.warp_validation = self.lightgcn_validation = self.simgcl_validation = None
    self.directau_validation = self.ssm_validation = self.ultragcn_validation = self.ccl_validation = None
    self.simplex_validation = self.ials_validation = self.ncf_validation = None
    self.ncf_history = []       # train_ncf: the mean loss per entry of each epoch
    self.ncf_state = None       # train_ncf: [Pg | Pm], [Qg | Qm], theta, Adam moments, step count (device; not saved)
    self.svd_info = None        # train_svd: what the last PureSVD fit reported
    self.rp3_info = None        # train_rp3beta: what the last RP3beta fit reported
    self.slim_info = None       # train_slim: what the last SLIM fit reported
    self.userknn_info = None    # train_userknn: what the last UserKNN fit reported
    self.itemknn_info = None    # train_itemknn: what the last ItemKNN fit reported
    self.__model_initialized = False
    self.__optimizer_state_dict = None
    self.__sparse_optimizer_state_dict = None
    self.__engine = None
    self._dist = None        # (rank, world_size) when data parallel

  # ------------------------------------------------------------------ init
  def __init_model(self):
    if self.__model_initialized:
      return
    require_gpu()
    self.model.init_model(self.num_items, self.num_users)
    self.model = self.model.to(device=self.device)
    self.__model_initialized = True

  def _fused_kind(self):
    # (a VariationalAutoencoder runs the autoencoder's entry-by-entry step with its bottleneck: FusedEngine.vae)
    if isinstance(self.model, (DynamicAutoencoder, VariationalAutoencoder)):
      return "ae"
    if isinstance(self.model, MatrixFactorization):
      return "mf"
    return None

  def _check_vae(self):
    """A VariationalAutoencoder trains on the fused HIP step only (no generic torch path, no sharded step):
    what that step does not cover raises ValueError here, before any GPU work."""
    if not isinstance(self.model, VariationalAutoencoder):
      return
    self.model._validate()
    if self.optimizer_type != "adam":
      raise ValueError("VariationalAutoencoder trains with optimizer_type='adam' only (the fused HIP step)")
    if isinstance(self.loss, str):
      if self.loss not in ("mse", "logistic", "logloss"):
        raise ValueError("Unknown loss function {}".format(self.loss))
      extra = set(self.loss_params) - ({"confidence"} if self.loss == "mse" else set())
      if extra:
        raise ValueError("VariationalAutoencoder: loss_params %s are outside the fused loss epilogues" % sorted(extra))
    elif isinstance(self.loss, (MSELoss, MultinomialNLLLoss)):
      if self.loss.reduction != "sum":
        raise ValueError("VariationalAutoencoder: the fused loss epilogues compute reduction='sum' only")
    elif isinstance(self.loss, torch.nn.BCEWithLogitsLoss):
      if self.loss.reduction != "sum" or self.loss.weight is not None or self.loss.pos_weight is not None:
        raise ValueError("VariationalAutoencoder: BCEWithLogitsLoss with weights or a reduction other than "
                         "'sum' is outside the fused loss epilogues")
    else:
      raise ValueError("VariationalAutoencoder: the loss must be 'mse', 'logistic', 'logloss' or their modules")
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if (multi or os.environ.get("RK_FORCE_DP") == "1" or os.environ.get("RK_PARALLEL") == "items" or
        getattr(self, "_dp_override", None) is not None or getattr(self, "_ip_override", None) is not None):
      raise ValueError("VariationalAutoencoder has no users-DP or item-parallel step")

  def _use_generic(self):
    """True when the combination has no fused HIP step and trains through torch
    autograd on the GPU instead (recoder_amd/generic.py): user-defined
    FactorizationModel subclasses, arbitrary nn.Module losses, sgd/adagrad/rmsprop."""
    if self._fused_kind() is None or self.optimizer_type != "adam":
      return True
    if getattr(self, "_force_generic", None):
      return True
    from .nn import fused_supported
    if not fused_supported(self.model):
      if not getattr(self, "_warned_generic", False):
        self._warned_generic = True
        log.warning("activation %r / first hidden size are outside the fused HIP kernels "
                    "(activations none|tanh|sigmoid|relu|selu|elu, size %% 4 == 0): training through "
                    "torch autograd on the GPU instead", self.model.activation_type)
      return True
    if isinstance(self.loss, str):
      # named losses are built as <Loss>(reduction='sum', **loss_params) (model.py:87-99): the fused
      # epilogues implement the MSE confidence weight and nothing else a module can be given
      extra = set(self.loss_params) - ({"confidence"} if self.loss == "mse" else set())
      if extra and not getattr(self, "_warned_loss_params", False):
        self._warned_loss_params = True
        log.warning("loss_params %s are outside the fused loss epilogues: training through torch "
                    "autograd on the GPU instead", sorted(extra))
      return bool(extra)
    # loss MODULES: the fused epilogues compute the plain summed loss -- anything else a module
    # can be configured with (mean / none reduction, element or class weights) goes through torch
    if isinstance(self.loss, (MSELoss, MultinomialNLLLoss)):
      return self.loss.reduction != "sum"
    if isinstance(self.loss, torch.nn.BCEWithLogitsLoss):
      return self.loss.reduction != "sum" or self.loss.weight is not None or \
          self.loss.pos_weight is not None
    return True

  def __init_loss_module(self):
    """model.py:87-99 -- same names, same errors."""
    if issubclass(self.loss.__class__, torch.nn.Module):
      self.loss_module = self.loss
      if isinstance(self.loss, MSELoss):
        self._loss_name, self._loss_params = "mse", {"confidence": self.loss.confidence}
      elif isinstance(self.loss, MultinomialNLLLoss):
        self._loss_name, self._loss_params = "logloss", {}
      elif isinstance(self.loss, torch.nn.BCEWithLogitsLoss):
        self._loss_name, self._loss_params = "logistic", {}
      else:
        self._loss_name, self._loss_params = None, {}       # generic path only
    elif self.loss == "logistic":
      self._loss_name, self._loss_params = "logistic", dict(self.loss_params)
      self.loss_module = torch.nn.BCEWithLogitsLoss(reduction="sum", **self.loss_params)
    elif self.loss == "mse":
      self._loss_name, self._loss_params = "mse", dict(self.loss_params)
      self.loss_module = MSELoss(reduction="sum", **self.loss_params)
    elif self.loss == "logloss":
      self._loss_name, self._loss_params = "logloss", {}
      self.loss_module = MultinomialNLLLoss(reduction="sum")
    elif self.loss is None:
      raise ValueError("No loss function defined")
    else:
      raise ValueError("Unknown loss function {}".format(self.loss))

  def __init_optimizer(self, lr, weight_decay):
    """model.py:101-164: dense / sparse parameter split, one group per tensor,
    no weight decay on biases."""
    if self.optimizer is not None:
      self._engine().sync_optimizer_steps()
      self.__optimizer_state_dict = self.optimizer.state_dict()
    if self.sparse_optimizer is not None:
      self._engine().sync_optimizer_steps()
      self.__sparse_optimizer_state_dict = self.sparse_optimizer.state_dict()

    sparse_params_names = []
    sparse_modules = [torch.nn.Embedding, torch.nn.EmbeddingBag]
    for module_name, module in self.model.named_modules():
      if type(module) in sparse_modules and module.sparse:
        sparse_params_names.extend([module_name + "." + n for n, _ in module.named_parameters()])

    params, sparse_params = [], []
    for param_name, param in self.model.named_parameters():
      wd = 0 if "bias" in param_name else weight_decay
      group = {"params": param, "weight_decay": wd}
      (sparse_params if param_name in sparse_params_names else params).append(group)

    if self.optimizer_type == "adam":
      if len(params) > 0:
        self.optimizer = optim.Adam(params, lr=lr)
      if len(sparse_params) > 0:
        self.sparse_optimizer = optim.SparseAdam(sparse_params, lr=lr)
    elif self.optimizer_type in ("adagrad", "sgd", "rmsprop"):
      # model.py:140-154; these run through torch on the GPU (generic path)
      if len(sparse_params) > 0:
        raise ValueError("Sparse gradients optimization not supported with {}"
                         .format(self.optimizer_type))
      if self.optimizer_type == "adagrad":
        self.optimizer = optim.Adagrad(params, lr=lr)
      elif self.optimizer_type == "sgd":
        self.optimizer = optim.SGD(params, lr=lr, momentum=0.9)
      else:
        self.optimizer = optim.RMSprop(params, lr=lr, momentum=0.9)
    else:
      raise Exception("Unknown optimizer kind")

    if self.__optimizer_state_dict is not None and self.optimizer is not None:
      self.optimizer.load_state_dict(self.__optimizer_state_dict)
      self.__optimizer_state_dict = None
    if self.__sparse_optimizer_state_dict is not None and self.sparse_optimizer is not None:
      self.sparse_optimizer.load_state_dict(self.__sparse_optimizer_state_dict)
      self.__sparse_optimizer_state_dict = None
    self._engine().bind_optimizers(self.optimizer, self.sparse_optimizer)

  def _sync_ranges(self):
    """Decoder-weight bound of the split-fp16 GEMMs from the table itself (engine.ranges): at every
    public entry, because parameters may have been written from outside since the last call."""
    eng = self._engine()
    if hasattr(eng, "refresh_weight_range"):
      eng.refresh_weight_range()

  def _check_ranges(self):
    """The same bound, recomputed only when the table changed since it was last taken (its torch
    version counter / address: predict and recommend are called once per evaluation batch, and a
    full-table norm is ~800 MB of reads at 1 M items)."""
    eng = self._engine()
    if hasattr(eng, "_check_weight_range"):
      eng._check_weight_range()

  def _engine(self):
    if self.__engine is None:
      self._check_vae()
      self.__init_loss_module()
      if self._use_generic():
        from .generic import GenericEngine
        self.__engine = GenericEngine(self.model, self.loss_module, self.device)
      else:
        self.__engine = FusedEngine(self.model, self._fused_kind(), self._loss_name,
                                    self._loss_params, self.device)
    return self.__engine

  # ------------------------------------------------------------ checkpoint
  def init_from_model_file(self, model_file):
    """model.py:166-191."""
    log.info("Loading model from: {}".format(model_file))
    if not os.path.isfile(model_file):
      raise Exception("No state file found in {}".format(model_file))
    st = torch.load(model_file, map_location="cpu", weights_only=False)
    model_params = st["model_params"]
    self.current_epoch = st["last_epoch"]
    self.loss = st.get("loss", self.loss)
    self.loss_params = st.get("loss_params", self.loss_params)
    self.optimizer_type = st["optimizer_type"]
    self.items = st.get("items", None)
    self.users = st.get("users", None)
    self.num_items = st.get("num_items", None)
    self.num_users = st.get("num_users", None)
    self.__optimizer_state_dict = st["optimizer"]
    self.__sparse_optimizer_state_dict = st.get("sparse_optimizer", None)
    self.model.load_model_params(model_params)
    self.__init_model()
    self.model.load_state_dict(st["model"])
    if self.__engine is not None and hasattr(self.__engine, "_w_range_stale"):
      self.__engine._w_range_stale = True

  def save_state(self, model_checkpoint_prefix):
    """model.py:193-224 (same dict; like the reference the sparse optimizer's
    state is not written)."""
    checkpoint_file = "{}_epoch_{}.model".format(model_checkpoint_prefix, self.current_epoch)
    log.info("Saving model to {}".format(checkpoint_file))
    if self.__engine is not None:
      self.__engine.sync_optimizer_steps()
    current_state = {
      "recoder_version": __version__,
      "model_params": self.model.model_params(),
      "last_epoch": self.current_epoch,
      "model": self.model.state_dict(),
      "optimizer_type": self.optimizer_type,
      "optimizer": self.optimizer.state_dict(),
      "items": self.items,
      "users": self.users,
      "num_items": self.num_items,
      "num_users": self.num_users,
    }
    if type(self.loss) is str:
      current_state["loss"] = self.loss
      current_state["loss_params"] = self.loss_params
    # (no collective in here: a caller may save from one rank only.  The checkpoint train() writes
    # under data / item parallelism has one writer and a barrier -- see _epoch_end)
    torch.save(current_state, checkpoint_file)
    return checkpoint_file

  # --------------------------------------------------------------- training
  def __init_training(self, train_dataset, lr, weight_decay):
    """model.py:226-254."""
    if self.items is None:
      self.items = train_dataset.items
    else:
      self.items = np.unique(np.append(self.items, train_dataset.items))
    if self.users is None:
      self.users = train_dataset.users
    else:
      self.users = np.unique(np.append(self.users, train_dataset.users))

    if self.item_based and self.num_items is None:
      self.num_items = int(np.max(self.items)) + 1
    elif self.item_based:
      assert self.num_items >= int(np.max(self.items)) + 1, \
        "The largest item id should be smaller than number of items." \
        "If your model is not based on items, set item_based to False in Recoder constructor."
    if self.user_based and self.num_users is None:
      self.num_users = int(np.max(self.users)) + 1
    elif self.user_based:
      assert self.num_users >= int(np.max(self.users)) + 1, \
        "The largest user id should be smaller than number of users." \
        "If your model is not based on users, set user_based to False in Recoder constructor."

    self.__init_model()
    self.__init_loss_module()
    self.__init_optimizer(lr=lr, weight_decay=weight_decay)

  def train(self, train_dataset, val_dataset=None, lr=0.001, weight_decay=0, num_epochs=1,
            iters_per_epoch=None, batch_size=64, lr_milestones=None, negative_sampling=False,
            num_sampling_users=0, num_data_workers=0, model_checkpoint_prefix=None,
            checkpoint_freq=0, eval_freq=0, eval_num_recommendations=None, eval_num_users=None,
            metrics=None, eval_batch_size=None):
    """Trains the model (arguments as model.py:256-289)."""
    log.info("GPU Mode (MI355X / HIP)")
    for k, v in self.model.model_params().items():
      log.info("Model {}: {}".format(k, v))
    log.info("lr {} wd {} batch {} optimizer {} milestones {} loss {}".format(
        lr, weight_decay, batch_size, self.optimizer_type, lr_milestones, self.loss))

    self._check_vae()
    if getattr(self.model, "fit_method", None):       # (the closed-form models of nn.py say so themselves)
      raise ValueError(self.model.fit_sentence % self.model.fit_method)
    if num_sampling_users == 0:
      num_sampling_users = batch_size
    if eval_batch_size is None:
      eval_batch_size = batch_size
    assert num_sampling_users >= batch_size and num_sampling_users % batch_size == 0, \
      "number of sampling users should be a multiple of the batch size"

    self._pick_engine_for(train_dataset)
    self.__init_training(train_dataset=train_dataset, lr=lr, weight_decay=weight_decay)
    train_dataset = self._setup_data_parallel(train_dataset, negative_sampling, batch_size)
    if getattr(self, "_ip", None) is not None:
      # item parallel: every rank processes the whole global batch against its items
      batch_size *= self._ip.world
      num_sampling_users *= self._ip.world

    train_dataloader = RecommendationDataLoader(train_dataset, batch_size=batch_size,
                                                negative_sampling=negative_sampling,
                                                num_sampling_users=num_sampling_users,
                                                num_workers=num_data_workers)
    if val_dataset is not None:
      val_dataloader = RecommendationDataLoader(val_dataset, batch_size=batch_size,
                                                negative_sampling=negative_sampling,
                                                num_sampling_users=num_sampling_users,
                                                num_workers=num_data_workers)
    else:
      val_dataloader = None

    if lr_milestones is not None:
      _last_epoch = -1 if self.current_epoch == 1 else (self.current_epoch - 2)
      if _last_epoch != -1:
        for g in self.optimizer.param_groups:
          g.setdefault("initial_lr", lr)
      lr_scheduler = MultiStepLR(self.optimizer, milestones=lr_milestones, gamma=0.1,
                                 last_epoch=_last_epoch)
    else:
      lr_scheduler = None

    self._train(train_dataloader=train_dataloader, val_dataloader=val_dataloader,
                num_epochs=num_epochs, current_epoch=self.current_epoch,
                lr_scheduler=lr_scheduler, batch_size=batch_size,
                model_checkpoint_prefix=model_checkpoint_prefix,
                checkpoint_freq=checkpoint_freq, eval_freq=eval_freq, metrics=metrics,
                eval_num_recommendations=eval_num_recommendations,
                iters_per_epoch=iters_per_epoch, eval_num_users=eval_num_users,
                eval_batch_size=eval_batch_size)
    self._sync_user_rows()

  def _scores_from_csr_rows(self):
    """True for the models without an encoder (nn.CsrScoresModel: the item-item models, scores = the users' CSR
    rows times W, and the user-neighbourhood model): scores come from ``model.csr_scores``."""
    return isinstance(self.model, CsrScoresModel)

  def _scores_from_user_ids(self):
    """True for the model scored from user ids by a kernel of its own (nn.NeuralMatrixFactorization): scores come
    from ``model.user_scores``."""
    return isinstance(self.model, NeuralMatrixFactorization)

  def _user_ids(self, users_interactions):
    """The batch's user ids on the device (int32), each checked against [0, num_users) on the host."""
    ids = np.asarray(users_interactions.users).astype(np.int64).reshape(-1)
    n = self.model.Pg.shape[0]
    if len(ids) and (ids.min() < 0 or ids.max() >= n):
      raise ValueError("user ids must lie in [0, %d) (got %d .. %d)" % (n, ids.min(), ids.max()))
    return torch.as_tensor(ids, dtype=torch.int32).to(self.device)

  def _size_hints(self, train_dataset):
    """(num_users, num_items) before the model is initialised: from the dataset's ids where unknown."""
    n_users, n_items = self.num_users, self.num_items
    if n_users is None and len(train_dataset.users):
      n_users = int(np.max(train_dataset.users)) + 1
    if n_items is None and len(train_dataset.items):
      n_items = int(np.max(train_dataset.items)) + 1
    return n_users, n_items

  def _reset_optimizers(self):
    """A fresh optimizer at the next __init_training: Adam moments of an earlier train() do not describe
    the tables a closed-form fit leaves."""
    self.optimizer = self.sparse_optimizer = None
    self.__optimizer_state_dict = self.__sparse_optimizer_state_dict = None

  def _closed_form_fit(self, mod, train_dataset, keep, check, log_line, fit, hint_check=None, check_values=False,
                       store=None, place=None, size_check=None, csrs=None, copy=dict):
    """The one sequence behind the ``train_*`` methods below: ``mod`` is the fit module, the callables say
    what differs, ``cfg`` is what ``check`` returned and ``host()`` the dataset's host matrix, built at the step
    that first asks for it.  The order decides which exception wins, and a call that raises in A-D leaves the
    Recoder and the model as they were:
      A ``check(model)``: the module's check_config, the model's class first;  B ``check_not_distributed``;
      C ``hint_check(cfg, users, items, host)``: the sizes of ``_size_hints`` against one device's memory, before
        init_model allocates (a catalogue that cannot fit gets a ValueError, not an OOM);
      D ``mod.check_values(host())``;  E the log line;  F ``store(cfg)``: hyperparameters back into the model;
      G fresh optimizers;  H ``place(cfg, first, host)``: on first use (after require_gpu) the size init_model
        allocates, later a re-allocation when it changed;  I ``__init_training``;
      J ``size_check(cfg, host)``: the real sizes against what is free;  K the device CSRs (``csrs``);
      L ``fit(model, csrs, cfg)``, kept in ``self.<keep>``;  M ``_weights_written()``; returns ``copy`` of it."""
    from . import als
    cfg = check(self.model)
    mod.check_not_distributed()
    host = functools.lru_cache(maxsize=None)(lambda: als.host_matrix(train_dataset))
    if hint_check is not None:
      hint_check(cfg, *self._size_hints(train_dataset), host)
    if check_values:
      mod.check_values(host())
    log.info(*log_line(cfg))
    for name, value in (store(cfg) if store else {}).items():
      setattr(self.model, name, value)
    self._reset_optimizers()
    if place is not None:
      first = not self.__model_initialized
      if first:
        require_gpu()
      place(cfg, first, host)
    self.__init_training(train_dataset=train_dataset, lr=0.001, weight_decay=0)
    if size_check is not None:
      size_check(cfg, host)
    pair = (csrs or als.csr_pair)(host(), self.num_users, self.num_items, self.device)
    setattr(self, keep, fit(self.model, pair, cfg))
    self._weights_written()
    return copy(getattr(self, keep))

  def _neighbour_list_fit(self, mod, train_dataset, keep, check, k_at, log_line, store, check_values=False,
                          memory=lambda cfg: {}):
    """``_closed_form_fit`` for the three models stored as [n, K] neighbour lists, K = ``cfg[k_at]``: the same
    memory checks (``memory(cfg)``: what else ``mod.check_memory`` is told), the same tensors to (re-)allocate and
    to hand to ``mod.fit(csrs, *cfg, out=...)``."""
    def place(cfg, first, host):
      if first:
        self.model.neighbours = cfg[k_at]
      elif cfg[k_at] != self.model.item_weights.shape[1]:
        self.model.allocate(cfg[k_at], self.device)
    return self._closed_form_fit(
        mod, train_dataset, keep, check, log_line, store=store, place=place, check_values=check_values,
        hint_check=lambda c, u, n, host: n and mod.check_memory(u or 0, n, c[k_at], 0, free_bytes=float("inf"),
                                                                **memory(c)),
        size_check=lambda c, host: mod.check_memory(self.num_users, self.num_items, c[k_at], host().nnz,
                                                    allocate_model=False, **memory(c)),
        fit=lambda m, pair, c: mod.fit(pair, *c, out=(m.item_neighbours, m.item_weights.data, m.neighbour_counts))[-1])

  def train_als(self, train_dataset, num_iterations=10, reg=100.0, cg_steps=3):
    """Implicit-feedback alternating least squares for a MatrixFactorization with activation 'none'
    (recoder_amd/als.py): minimises the configured MSELoss(confidence=alpha, reduction='sum') over the
    whole user x item matrix plus reg (|X|^2 + |Y|^2), the bias held fixed, each row solved with
    ``cg_steps`` warm-started conjugate-gradient steps.  Builds a fresh optimizer of
    ``optimizer_type``, so that ``save_state`` and ``train`` work on the tables it leaves.  Returns
    (and keeps in ``als_history``) the objective after each iteration."""
    from . import als
    return self._closed_form_fit(
        als, train_dataset, "als_history", copy=list,
        check=lambda m: als.check_config(m, self.loss, self.loss_params, num_iterations, reg, cg_steps),
        log_line=lambda alpha: ("ALS: %d iterations, reg %g, confidence %g, %d CG steps", num_iterations, reg, alpha,
                                cg_steps),
        fit=lambda m, pair, alpha: als.fit(*_mf_tables(m), m.bias.data, *pair, alpha, float(reg), int(cg_steps),
                                           int(num_iterations)))

  def train_ials(self, train_dataset, num_sweeps=16, block_size=64, alpha0=0.03, reg=0.03, nu=1.0, init_std=None,
                 seed=0, val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500, eval_num_users=None,
                 patience=None, restore_best=False):
    """iALS++ (Rendle et al. 2021) on the iALS objective of Rendle et al. 2022 for a MatrixFactorization with
    activation 'none' (recoder_amd/ials.py): minimises sum over the stored entries of (x_u . y_i - 1)^2 + ``alpha0``
    times the sum over ALL pairs of (x_u . y_i)^2 + sum_u lam_u |x_u|^2 + sum_i mu_i |y_i|^2 with the frequency-scaled
    regularisers lam_u = ``reg`` (r_u + ``alpha0`` n_items)^``nu`` and mu_i = ``reg`` (d_i + ``alpha0`` n_users)^``nu``
    (r_u, d_i the row and column counts; ``nu = 0`` is one ``reg`` for every row).  A sweep visits the blocks of
    ``block_size`` (1..``ials.MAX_BLOCK``, cut to h) coordinates in ascending order, all users for a block and then all
    items, and solves every row's block exactly by Cholesky against a cache of the stored entries' predictions;
    ``block_size = h`` is exact ALS.  Embedding sizes up to ``ials.MAX_H``.  ``init_std`` None trains the tables as
    they stand (a warm start from any earlier fit, and how a later call continues: two calls of n sweeps are one of
    2 n, bit for bit); a float draws both from N(0, init_std^2 / h) with a generator seeded by ``seed`` (torch's
    global one is not touched).  The stored values and the configured ``loss`` play no part; the bias ends as 0.
    Builds a fresh optimizer of ``optimizer_type``, so that ``save_state``, ``train``, ``train_als``, ``fold_in`` and
    the embeddings index work on the tables it leaves.  A row whose block system is not positive definite (``reg = 0``
    only) is left unchanged, with one warning per call.  Returns (and keeps in ``ials_history``) L after each sweep.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``), once
    per sweep."""
    from . import ials
    vcheck, monitor, vkeep = self._validated("train_ials", "ials", train_dataset, (val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience, restore_best))

    def check(m):
      c = ials.check_config(m, num_sweeps, block_size, alpha0, reg, nu, init_std, seed)
      vcheck()
      return c

    def fit(m, pair, c):
      X, Y = _mf_tables(m)
      if c[5] is not None:
        ials.init_tables(X, Y, c[5], c[6])
      m.bias.data.zero_()
      hist = ials.fit(X, Y, pair, c[2], c[3], c[4], c[1], c[0], monitor=monitor())
      vkeep()
      return hist
    return self._closed_form_fit(
        ials, train_dataset, "ials_history", copy=list, csrs=ials.csr_pair, check=check, fit=fit,
        log_line=lambda c: ("iALS++: %d sweeps of blocks of %d, alpha0 %g, reg %g, nu %g, init_std %s, seed %d",) + c,
        hint_check=lambda c, u, n, host: u and n and ials.check_memory(u, n, self.model.embedding_size, 0, c[1],
                                                                       free_bytes=float("inf")),
        size_check=lambda c, host: ials.check_memory(self.num_users, self.num_items, self.model.embedding_size,
                                                     host().nnz, c[1], allocate_model=False))

  def _validated(self, method, prefix, train_dataset, args):
    """The validation keywords the iterative trainers share (recoder_amd/validation.py), ``args`` =
    (val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience, restore_best).  With a
    ``val_dataset`` (a dataset with an ``interactions_matrix`` to score from and a ``target_interactions_matrix``
    to hit) the fit evaluates ``eval_metric`` (None: Recall(20); one of Recall, NDCG, AveragePrecision) after every
    ``eval_freq`` epochs on the first ``eval_num_users`` users (None: all) in batches of ``eval_batch_size``, at
    the model a fit ending at that epoch would leave, scoring, top-k and metric on the device.  ``patience = p``
    stops the fit after p evaluations in a row without a new best (strictly greater; nan never is one);
    ``restore_best`` keeps a device copy of the best epoch and puts it back at the end, so that the model (and a
    graph method's ``<prefix>_state``) is what a fit of ``best_epoch`` epochs leaves.  The loss history keeps every
    epoch that ran; ``self.<prefix>_validation`` = {"metric", "k", "values", "epochs", "best_epoch",
    "stopped_epoch"} (None without a ``val_dataset``).  Nothing of this touches the fit's draws or arithmetic.
    ``train_ssm``, ``train_ultragcn`` and ``train_ccl`` keep the parameter lists their contracts pin, so they take the same settings
    from ``self.fit_validation``: a dict of these keywords (``val_dataset`` at least), set like the Recoder's other
    hooks and read by every one of these fits that is called without a ``val_dataset`` keyword, until it is set
    back to None.
    Returns (check, monitor, keep): ``check()`` raises the ValueErrors before any GPU work, ``monitor()`` builds the
    fit's ``validation.Monitor`` (None without validation) once the model is placed, ``keep()`` stores the result."""
    from . import validation
    box = {}

    def check():
      n_items = self._size_hints(train_dataset)[1]
      box["cfg"] = validation.check_config(method, *args, num_items=n_items)
      if box["cfg"] is None and self.fit_validation is not None:
        box["cfg"] = validation.check_config(method, **validation.check_settings(self.fit_validation), num_items=n_items)

    def monitor():
      cfg = box["cfg"]
      if cfg is not None:
        box["monitor"] = validation.Monitor(
            validation.Validator(self, cfg.dataset, cfg.metric, None, cfg.batch_size, cfg.num_users), cfg)
      return box.get("monitor")

    def keep():
      setattr(self, prefix + "_validation", box["monitor"].result() if "monitor" in box else None)
    return check, monitor, keep

  def train_bpr(self, train_dataset, num_epochs=40, batch_size=1024, lr=0.1, reg=0.01, seed=0, num_candidates=1,
                val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500,
                eval_num_users=None, patience=None, restore_best=True):
    """BPR-MF (Rendle et al. 2009) for a MatrixFactorization with activation 'none' (recoder_amd/bpr.py):
    pairwise ranking on sampled triples (user, a stored item, an item the user does not hold), loss
    softplus(-(x_ui - x_uj)), synchronous mini-batch SGD with learning rate ``lr`` and an L2 pull ``reg``
    on every row a triple touches, the bias trained with the item table.  An epoch is
    ceil(nnz / batch_size) steps of ``batch_size`` triples; the draws are a pure function of ``seed``,
    the step (counted from 0 in every call) and the slot, so a fixed seed gives the same bits.  The
    stored values and the configured ``loss`` play no part.  Builds a fresh optimizer of
    ``optimizer_type``, so that ``save_state``, ``train`` and ``train_als`` work on the tables it leaves.
    With ``num_candidates`` > 1 (up to 32) the negative is not the first item the user does not hold but the
    highest-scored of the first ``num_candidates`` such draws, at the tables as they stand at the start of the
    step (dynamic negative sampling, Zhang et al. 2013); everything else is unchanged.
    Returns (and keeps in ``bpr_history``) the mean loss per valid triple of each epoch.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``)."""
    from . import bpr
    vcheck, monitor, vkeep = self._validated("train_bpr", "bpr", train_dataset, (val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience, restore_best))

    def check(m):
      c = bpr.check_config(m, num_epochs, batch_size, lr, reg, seed) + (bpr.check_candidates(num_candidates),)
      vcheck()
      return c

    def fit(m, ucsr, c):
      hist = bpr.fit(*_mf_tables(m), m.bias.data, ucsr, *c[:5], num_candidates=c[5], monitor=monitor())
      vkeep()
      return hist
    return self._closed_form_fit(
        bpr, train_dataset, "bpr_history", copy=list, csrs=bpr.user_csr, check=check, fit=fit,
        log_line=lambda c: ("BPR: %d epochs of batches of %d, lr %g, reg %g, seed %d, %d candidate(s) per slot",) + c,
        size_check=lambda c, host: bpr.check_data(host().nnz, self.num_items, c[0], c[1]))

  def train_warp(self, train_dataset, num_epochs=10, batch_size=1024, lr=0.005, reg=0.05, margin=1.0,
                 max_draws=32, rank_weight="log", seed=0, val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500,
                 eval_num_users=None, patience=None, restore_best=True):
    """WARP (Weston et al. 2011; LightFM's loss) for a MatrixFactorization with activation 'none'
    (recoder_amd/warp.py): a slot is one of ``train_bpr``'s stored entries (u, i); items the user does not hold
    are drawn and scored until one violates the margin, (s_uj - s_ui) + ``margin`` > 0, and the update is BPR's
    with the weight of the rank that the number N of scored candidates estimates: ``rank_weight`` 'log' is
    log(max(1, (n_items - 1) // N)), 'harmonic' the harmonic number of (n_items - 1) // N.  A slot without a
    violator in ``max_draws`` (1..256) draws adds nothing.  Epochs, ``lr``, ``reg``, the seed and what the fitted
    tables plug into are as in ``train_bpr``; the users and stored items of a step are its draws for the same
    seed.  Returns (and keeps in ``warp_history``) the mean loss per valid slot of each epoch; ``warp_stats``
    keeps per epoch (the share of slots that found a violator, their mean N): as the model learns the share
    falls and N rises.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``)."""
    from . import warp
    vcheck, monitor, vkeep = self._validated("train_warp", "warp", train_dataset, (val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience, restore_best))

    def check(m):
      c = warp.check_config(m, num_epochs, batch_size, lr, reg, margin, max_draws, rank_weight, seed)
      vcheck()
      return c

    def fit(m, ucsr, c):
      hist, self.warp_stats = warp.fit(*_mf_tables(m), m.bias.data, ucsr, *c, monitor=monitor())
      vkeep()
      return hist
    return self._closed_form_fit(
        warp, train_dataset, "warp_history", copy=list, csrs=warp.bpr.user_csr, fit=fit, check=check,
        log_line=lambda c: ("WARP: %d epochs of batches of %d, lr %g, reg %g, margin %g, at most %d draws, %s "
                            "weights, seed %d",) + c,
        size_check=lambda c, host: warp.check_data(host().nnz, self.num_items, c[0], c[1]))

  def _graph_fit(self, mod, prefix, train_dataset, resume, log_format, *config,
                 validation=(None, None, 1, 500, None, None, True), hint_check=None):
    """``_closed_form_fit`` for the three methods that train base tables over the user-item graph (the driver of
    recoder_amd/lightgcn.py): ``mod.check_config(model, *config)``, then with ``resume`` the kept
    ``self.<prefix>_state`` checked and handed to ``mod.fit``; the history goes to ``self.<prefix>_history``.
    ``validation``: the arguments of ``_validated``, the fit's one hook at the epoch's end.  ``hint_check``:
    ``_closed_form_fit``'s, what the method checks of the host matrix before any GPU work."""
    vcheck, monitor, vkeep = self._validated("train_" + prefix, prefix, train_dataset, validation)

    def check(m):
      c = mod.check_config(m, *config)
      if resume:
        mod.check_resume(getattr(self, prefix + "_state"), c[0])
      vcheck()
      return c

    def fit(m, pair, c):
      # (a fresh state replaces the kept one only once the fit's own checks have passed)
      state, hist = mod.fit(*_mf_tables(m), m.bias.data, *pair, *c,
                            state=getattr(self, prefix + "_state") if resume else None, monitor=monitor())
      setattr(self, prefix + "_state", state)
      vkeep()
      return hist
    return self._closed_form_fit(
        mod, train_dataset, prefix + "_history", copy=list, check=check, fit=fit, hint_check=hint_check,
        log_line=lambda c: (log_format,) + c,
        size_check=lambda c, host: mod.check_data(host().nnz, self.num_items, c[1], c[2]))

  def train_lightgcn(self, train_dataset, num_layers=3, num_epochs=10, batch_size=1024, lr=0.01, reg=1e-3, seed=0,
                     resume=False, val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500,
                     eval_num_users=None, patience=None, restore_best=True):
    """LightGCN (He et al. 2020) for a MatrixFactorization with activation 'none' (recoder_amd/lightgcn.py): the
    final tables are the mean over ``num_layers`` + 1 layers of trainable base tables propagated over the
    symmetrically normalised user-item graph of the stored entries, trained on BPR's triples (the draws of
    ``train_bpr`` for the same seed, step and slot) with Adam at learning rate ``lr`` and the L2 term ``reg`` on
    the base rows a triple touches.  The base tables of a first call are the tables as they stand; they, both
    Adam moments, the step count and ``num_layers`` stay in ``lightgcn_state`` (device tensors, not part of a
    checkpoint), and ``resume=True`` continues from them with the draws, moments and step count one longer
    call would have had.  The model's tables end as the final tables and the bias as 0: ``save_state``,
    ``recommend``, ``evaluate``, ``train``, ``train_als`` and ``train_bpr`` take them as they are.  The stored
    values and the configured ``loss`` play no part.  Returns (and keeps in ``lightgcn_history``) the mean
    loss per valid triple of each epoch.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``)."""
    from . import lightgcn
    return self._graph_fit(lightgcn, "lightgcn", train_dataset, resume,
                           "LightGCN: %d layers, %d epochs of batches of %d, lr %g, reg %g, seed %d",
                           num_layers, num_epochs, batch_size, lr, reg, seed,
                           validation=(val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience,
                                       restore_best))

  def train_simgcl(self, train_dataset, num_layers=2, num_epochs=10, batch_size=1024, lr=0.002, reg=1e-3,
                   cl_weight=0.1, cl_eps=0.2, cl_temperature=0.2, seed=0, resume=False, val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500,
                   eval_num_users=None, patience=None, restore_best=True):
    """SimGCL (Yu et al. 2022) for a MatrixFactorization with activation 'none' (recoder_amd/simgcl.py):
    LightGCN's propagation with the mean over the layers 1..``num_layers`` (layer 0 is left out), trained on
    BPR's triples (the draws of ``train_bpr`` and ``train_lightgcn`` for the same seed, step and slot) plus
    ``cl_weight`` times an InfoNCE term at temperature ``cl_temperature`` between two views of the batch's
    distinct users and of its distinct positive items; a view adds a random vector of length ``cl_eps``, in the
    orthant of the row, to every row after every layer.  No graph is augmented.  Adam at learning rate ``lr``,
    the L2 term ``reg`` on the base rows a triple touches; ``batch_size`` is at most ``simgcl.MAX_BATCH``.  The
    base tables of a first call are the tables as they stand; they, both Adam moments, the step count and
    ``num_layers`` stay in ``simgcl_state`` (device tensors, not part of a checkpoint), and ``resume=True``
    continues from them with the draws, noise, moments and step count one longer call would have had.  The
    model's tables end as the clean tables and the bias as 0: ``save_state``, ``recommend``, ``evaluate``,
    ``train``, ``train_als`` and ``train_bpr`` take them as they are.  The stored values and the configured
    ``loss`` play no part.  Returns (and keeps in ``simgcl_history``) one (mean BPR loss per valid triple, mean
    NCE_users + NCE_items per step) pair per epoch.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``)."""
    from . import simgcl
    return self._graph_fit(simgcl, "simgcl", train_dataset, resume,
                           "SimGCL: %d layers, %d epochs of batches of %d, lr %g, reg %g, cl_weight %g, eps %g, "
                           "temperature %g, seed %d",
                           num_layers, num_epochs, batch_size, lr, reg, cl_weight, cl_eps, cl_temperature, seed,
                           validation=(val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience,
                                       restore_best))

  def train_directau(self, train_dataset, num_layers=2, num_epochs=10, batch_size=1024, lr=0.01, reg=1e-3,
                     gamma=0.2, seed=0, resume=False, val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500,
                     eval_num_users=None, patience=None, restore_best=True):
    """DirectAU (Wang et al. 2022) for a MatrixFactorization with activation 'none' (recoder_amd/directau.py):
    no negatives are drawn.  A step takes the (user, stored item) pairs of BPR's draws (those of ``train_bpr``,
    ``train_lightgcn`` and ``train_simgcl`` for the same seed, step and slot), normalises their rows of the final
    tables to unit length and descends the mean squared distance of a pair (alignment) plus ``gamma`` / 2 times
    the uniformity -- the logarithm of the mean of exp(-2 distance^2) over the pairs of slots -- of the batch's
    user rows and of its item rows.  The final tables are LightGCN's mean over ``num_layers`` + 1 layers;
    ``num_layers = 0`` trains the tables themselves (DirectAU-MF) and propagates nothing.  Adam at learning rate
    ``lr``, the L2 term ``reg`` on the base rows a slot touches; ``batch_size`` is at most ``directau.MAX_BATCH``.
    The base tables of a first call are the tables as they stand; they, both Adam moments, the step count and
    ``num_layers`` stay in ``directau_state`` (device tensors, not part of a checkpoint), and ``resume=True``
    continues from them with the draws, moments and step count one longer call would have had.  The model's
    tables end as the final tables, un-normalised (a user scores by the plain dot product, as in the paper's
    code), and the bias as 0: ``save_state``, ``recommend``, ``evaluate``, ``train``, ``train_als`` and
    ``train_bpr`` take them as they are.  The stored values and the configured ``loss`` play no part.  Returns
    (and keeps in ``directau_history``) one (alignment, uniformity of the users, uniformity of the items) triple
    of per-step means per epoch.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``)."""
    from . import directau
    return self._graph_fit(directau, "directau", train_dataset, resume,
                           "DirectAU: %d layers, %d epochs of batches of %d, lr %g, reg %g, gamma %g, seed %d",
                           num_layers, num_epochs, batch_size, lr, reg, gamma, seed,
                           validation=(val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience,
                                       restore_best))

  def train_ssm(self, train_dataset, num_layers=2, num_epochs=10, batch_size=1024, lr=0.01, reg=1e-3,
                temperature=0.2, num_negatives=1024, similarity="cosine", logq_weight=0.0, normalize=False, seed=0,
                resume=False):
    """Sampled-softmax training (Wu et al. 2022; the in-batch softmax of Yi et al. 2019 and the mixed negatives of
    Yang et al. 2020) for a MatrixFactorization with activation 'none' (recoder_amd/ssm.py).  A step takes the
    (user, stored item) pairs of BPR's draws (those of ``train_bpr`` and ``train_lightgcn`` for the same seed,
    step and slot) and descends the mean of -log softmax of a pair's logit over ``batch_size`` +
    ``num_negatives`` candidates: the batch's own positives and ``num_negatives`` items drawn uniformly from the
    catalogue, shared by the batch (a function of seed, step and index; nothing is rejected, and of the items a
    user holds only a repeat of the pair's own positive is left out of its row).  The logit is the cosine
    (``similarity="dot"``: the dot product) of the rows of the final tables over ``temperature``, minus
    ``logq_weight`` times the logarithm of the share of the candidates the item is expected to hold (Yi et
    al.'s correction, on the positive as on the negatives; 0 switches it off).  The final tables are LightGCN's
    mean over ``num_layers`` + 1 layers; ``num_layers = 0`` trains the tables themselves and propagates nothing.
    Adam at learning rate ``lr``, the L2 term ``reg`` on the base rows a slot or a candidate touches;
    ``batch_size`` is at most ``ssm.MAX_BATCH`` and ``num_negatives`` at most ``ssm.MAX_NEGATIVES``.  The base
    tables of a first call are the tables as they stand; they, both Adam moments, the step count and
    ``num_layers`` stay in ``ssm_state`` (device tensors, not part of a checkpoint), and ``resume=True`` continues
    from them with the draws, moments and step count one longer call would have had.  The model's tables end as
    the final tables -- un-normalised, or with ``normalize=True`` row-normalised, so that the dot product of
    ``recommend`` ranks by the cosine the fit trained; the state's base tables are never normalised -- and the
    bias as 0: ``save_state``, ``recommend``, ``evaluate``, ``train``, ``train_als`` and ``train_bpr`` take them
    as they are.  The stored values and the configured ``loss`` play no part.  Returns (and keeps in
    ``ssm_history``) one (loss, probability of the positive) pair of per-step means per epoch.
    Validation during the fit and early stopping: ``self.fit_validation`` (``_validated``).  With
    ``normalize=True`` an evaluation scores the row-normalised tables, as the finished fit would."""
    from . import ssm
    return self._graph_fit(ssm, "ssm", train_dataset, resume,
                           "SSM: %d layers, %d epochs of batches of %d, lr %g, reg %g, temperature %g, %d shared "
                           "negatives, %s similarity, logq_weight %g, normalize %s, seed %d",
                           num_layers, num_epochs, batch_size, lr, reg, temperature, num_negatives, similarity,
                           logq_weight, normalize, seed)

  def train_ultragcn(self, train_dataset, num_epochs=20, batch_size=1024, lr=0.01, reg=1e-3, num_negatives=32,
                     negative_weight=8.0, neighbours=10, item_weight=1e-3, w=(1e-7, 1.0, 1e-7, 1.0), seed=0,
                     resume=False):
    """UltraGCN (Mao et al. 2021) for a MatrixFactorization with activation 'none' (recoder_amd/ultragcn.py): no
    message passing.  A step takes the (user, stored item) pairs of BPR's draws (those of ``train_bpr`` and
    ``train_lightgcn`` for the same seed, step and slot), draws ``num_negatives`` items per pair uniformly from the
    catalogue (a function of seed, step, slot and index, private to the slot; nothing is rejected) and descends the
    mean over the pairs of a pointwise log-loss with degree-derived weights -- (w1 + w2 beta) on the positive,
    ``negative_weight`` / ``num_negatives`` (w3 + w4 beta) on every negative, beta_ux = sqrt(r_u + 1) / r_u /
    sqrt(d_x + 1) -- plus ``item_weight`` times the log-loss of the user against the ``neighbours`` items most
    related to the positive in the item-item co-occurrence graph, weighted by the paper's omega.
    ``item_weight = 0`` or ``neighbours = 0`` is UltraGCN-base: no item graph (an items x items buffer) is built.
    Adam at learning rate ``lr``, the L2 term ``reg`` on the rows a pair touches as its user or its positive;
    ``batch_size`` is at most ``ultragcn.MAX_BATCH``, ``num_negatives`` at most ``ultragcn.MAX_NEGATIVES``,
    ``neighbours`` at most ``ultragcn.MAX_NEIGHBOURS`` and ``batch_size`` * (1 + ``num_negatives`` + ``neighbours``)
    at most ``ultragcn.MAX_ENTRIES``.  The tables, both Adam moments and the step count stay in ``ultragcn_state``
    (device tensors, not part of a checkpoint), and ``resume=True`` continues from them with the draws, moments and
    step count one longer call would have had.  The model's tables end as the trained tables and the bias as 0:
    ``save_state``, ``recommend``, ``evaluate``, ``train``, ``train_als`` and ``train_bpr`` take them as they are.  The
    stored values and the configured ``loss`` play no part.  Returns (and keeps in ``ultragcn_history``) one
    (positive, negatives, neighbours) triple of the three terms' means per valid pair per epoch.
    Validation during the fit and early stopping: ``self.fit_validation`` (``_validated``)."""
    from . import ultragcn
    return self._graph_fit(ultragcn, "ultragcn", train_dataset, resume,
                           "UltraGCN: %d layers, %d epochs of batches of %d, lr %g, reg %g, %d negatives a slot at "
                           "weight %g, %d neighbours at weight %g, w %s, seed %d",
                           num_epochs, batch_size, lr, reg, num_negatives, negative_weight, neighbours, item_weight, w,
                           seed)

  def train_ccl(self, train_dataset, num_layers=0, num_epochs=10, batch_size=1024, lr=0.01, reg=1e-3,
                num_negatives=64, negative_weight=16.0, margin=0.0, normalize=False, seed=0, resume=False):
    """SimpleX's cosine contrastive loss (Mao et al. 2021) for a MatrixFactorization with activation 'none'
    (recoder_amd/ccl.py).  A step takes the (user, stored item) pairs of BPR's draws (those of ``train_bpr`` and
    ``train_lightgcn`` for the same seed, step and slot), draws ``num_negatives`` items per pair uniformly from the
    catalogue (``train_ultragcn``'s draws for the same seed, step, slot and index; nothing is rejected) and descends
    the mean over the pairs of (1 - cos(u, i)) + ``negative_weight`` / ``num_negatives`` times the sum over the
    negatives of max(0, cos(u, j) - ``margin``), the cosines taken between rows of the final tables.  A negative
    below the margin is dead: it gets no gradient, and the item-side sum never reads it.  The final tables are
    LightGCN's mean over ``num_layers`` + 1 layers; ``num_layers = 0`` trains the tables themselves and propagates
    nothing.  This is SimpleX's loss alone: the pooling of the user's history is ``train_simplex``; the dropout and the
    attention poolings are not built.  Adam at learning rate ``lr``, the L2 term ``reg`` on the base rows a pair touches as its user
    or its positive; ``batch_size`` is at most ``ccl.MAX_BATCH``, ``num_negatives`` at most ``ccl.MAX_NEGATIVES``
    and ``batch_size`` * (1 + ``num_negatives``) at most ``ccl.MAX_ENTRIES``; ``margin`` lies in [-1, 1).  The base
    tables of a first call are the tables as they stand; they, both Adam moments, the step count and ``num_layers``
    stay in ``ccl_state`` (device tensors, not part of a checkpoint), and ``resume=True`` continues from them with
    the draws, moments and step count one longer call would have had.  The model's tables end as the final tables
    -- un-normalised, or with ``normalize=True`` row-normalised, so that the dot product of ``recommend`` ranks by
    the cosine the fit trained; the state's base tables are never normalised -- and the bias as 0: ``save_state``,
    ``recommend``, ``evaluate``, ``train``, ``train_als`` and ``train_bpr`` take them as they are.  The stored values
    and the configured ``loss`` play no part.  Returns (and keeps in ``ccl_history``) one (positive term, negative
    term) pair of means per valid pair per epoch; ``ccl_stats`` keeps the mean share of live negatives of each epoch.
    Validation during the fit and early stopping: ``self.fit_validation`` (``_validated``).  With
    ``normalize=True`` an evaluation scores the row-normalised tables, as the finished fit would."""
    from . import ccl
    hist = self._graph_fit(ccl, "ccl", train_dataset, resume,
                           "CCL: %d layers, %d epochs of batches of %d, lr %g, reg %g, %d negatives a slot at weight "
                           "%g, margin %g, normalize %s, seed %d",
                           num_layers, num_epochs, batch_size, lr, reg, num_negatives, negative_weight, margin,
                           normalize, seed)
    self.ccl_stats = list(self.ccl_state["live_share"])
    return hist

  def train_simplex(self, train_dataset, gamma=0.5, max_history=256, num_epochs=10, batch_size=1024, lr=0.01, reg=1e-3,
                    num_negatives=64, negative_weight=16.0, margin=0.0, normalize=False, seed=0, resume=False,
                    val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500, eval_num_users=None,
                    patience=None, restore_best=True):
    """SimpleX (Mao et al. 2021) for a MatrixFactorization with activation 'none' (recoder_amd/simplex.py):
    ``train_ccl``'s loss, slots, negatives, L2 term and Adam at user rows pooled from the users' histories.  The
    parameters are the tables P and Q and an h x h map W (the identity at the start of a fresh fit); a user's history
    is the whole stored row, or for a row longer than ``max_history`` (1..``simplex.MAX_HISTORY``) the ``max_history``
    entries at the positions floor(j r / max_history) of its stored order; the slot's own positive is not removed and
    the stored values play no part.  The final tables are X[u] = ``gamma`` P[u] + (1 - ``gamma``) W mean(Q[history of
    u]) and Y = Q, ``gamma`` in [0, 1].  A step pools the rows of its own ``batch_size`` slots only; history items and
    W take no L2 term.  With ``gamma = 1`` the pooling branch is not run and the fit is ``train_ccl(num_layers=0)``
    bit for bit.  ``batch_size`` * min(``max_history``, the longest stored row) is at most ``simplex.MAX_ENTRIES``.
    P, Q, W, their Adam moments, the step count, ``gamma`` and ``max_history`` stay in ``simplex_state`` (device
    tensors, not part of a checkpoint), and ``resume=True`` continues from them, at the same ``gamma`` and
    ``max_history``, with the draws, moments and step count one longer call would have had.  The model's tables end
    as X for every training user and Y -- un-normalised, or with ``normalize=True`` row-normalised, as in
    ``train_ccl`` -- and the bias as 0: ``save_state``, ``recommend``, ``evaluate``, ``train``, ``train_als`` and
    ``train_bpr`` take them as they are; ``simplex_encode`` gives the pooled row of any history.  Not built: SimpleX's
    embedding dropout, its attention poolings, LightGCN layers under the pooling and multi-GPU training.  Returns (and
    keeps in ``simplex_history``) one (positive term, negative term) pair of means per valid pair per epoch;
    ``simplex_stats`` keeps the mean share of live negatives of each epoch.
    ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``).  With
    ``normalize=True`` an evaluation scores the row-normalised tables, as the finished fit would."""
    from . import simplex

    def hint_check(c, users, items, host):
      if c[0][0] < 1.0:
        simplex.check_entries(c[2], simplex.entry_width(np.diff(host().indptr), c[0][1]))
    hist = self._graph_fit(simplex, "simplex", train_dataset, resume,
                           "SimpleX: (gamma, max_history) %s, %d epochs of batches of %d, lr %g, reg %g, %d negatives a "
                           "slot at weight %g, margin %g, normalize %s, seed %d",
                           gamma, max_history, num_epochs, batch_size, lr, reg, num_negatives, negative_weight, margin,
                           normalize, seed, hint_check=hint_check,
                           validation=(val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience,
                                       restore_best))
    self.simplex_stats = list(self.simplex_state["live_share"])
    return hist

  def train_ncf(self, train_dataset, num_epochs=10, batch_size=1024, lr=1e-3, reg=0.0, num_negatives=8, seed=0,
                resume=False, val_dataset=None, eval_metric=None, eval_freq=1, eval_batch_size=500,
                eval_num_users=None, patience=None, restore_best=True):
    """NeuMF (He et al. 2017) for a NeuralMatrixFactorization (recoder_amd/ncf.py): a step takes ``batch_size``
    (1..4096) of ``train_bpr``'s stored entries (u, i) with the label 1 and for each ``num_negatives`` (1..1024)
    uniformly drawn items with the label 0 -- the candidate round of ``train_ultragcn`` and ``train_ccl``, which rejects
    nothing: an item the user holds can come up -- and descends the mean binary cross-entropy of the logits over these
    ``batch_size * (1 + num_negatives)`` entries (at most ``ncf.MAX_ENTRIES``) by one Adam step with learning rate
    ``lr`` on the four tables (lazily: the L2 term ``reg`` reaches the rows the step touches) and on the dense
    parameters (decay ``reg`` on the weights, none on the biases).  Forward, loss and backward are one HIP launch; the
    draws are pure integer functions of (seed, step, slot), so a fixed seed gives the same bits.  A model that is not
    initialised yet draws its parameters from ``seed``.  The tables, the dense parameters, their Adam moments and the
    step count stay in ``ncf_state`` (device memory; not part of checkpoints) and ``resume=True`` continues from them:
    2 + 1 epochs are 3 epochs bit for bit.  Returns (and keeps in ``ncf_history``) the mean loss per entry of each
    epoch.  ``val_dataset`` and the keywords after it: validation during the fit and early stopping (``_validated``).
    The defaults (10 epochs, lr 1e-3, 8 negatives, the model's (32, 32, (64, 32, 16))) are the best Recall@20 of the
    float64 grid on the ML-20M slice (profiles/ncf_quality.jsonl): 0.1236; the fit overfits from there (0.1092 after 15).
    Not built: GMF-only and MLP-only models and pre-training from them, other activations, dropout, multi-GPU."""
    from . import bpr, ncf
    vcheck, monitor, vkeep = self._validated("train_ncf", "ncf", train_dataset, (val_dataset, eval_metric, eval_freq, eval_batch_size, eval_num_users, patience, restore_best))

    def check(m):
      c = ncf.check_config(m, num_epochs, batch_size, lr, reg, num_negatives, seed)
      if resume:
        ncf.check_resume(self.ncf_state, c[0])
      vcheck()
      return c

    def store(c):
      return {} if self.model.Pg is not None else {"init_seed": c[6]}

    def fit(m, ucsr, c):
      state, hist = ncf.fit(m, ucsr, *c[1:], state=self.ncf_state if resume else None, monitor=monitor())
      self.ncf_state = state
      vkeep()
      return hist
    return self._closed_form_fit(
        ncf, train_dataset, "ncf_history", copy=list, csrs=bpr.user_csr, check=check, fit=fit, store=store,
        log_line=lambda c: ("NeuMF: sizes %r, %d epochs of batches of %d, lr %g, reg %g, %d negatives, seed %d",) + c,
        size_check=lambda c, host: ncf.check_data(host().nnz, self.num_items, c[1], c[2]))

  def simplex_encode(self, interactions_matrix):
    """[B, h] on the device: the user rows (1 - gamma) W mean(Q[history]) that the last ``train_simplex`` gives the B
    histories (the rows of ``interactions_matrix``, a scipy matrix over the model's items), users the fit never saw
    included; an empty row gives the zero vector.  W, Q, ``gamma`` and the ``max_history`` rule are
    ``simplex_state``'s; the users' own table P plays no part, so after a fit with ``gamma = 0`` the training rows
    encode to the model's user table."""
    import scipy.sparse as sp
    from . import als, simplex
    if self.simplex_state is None:
      raise ValueError("simplex_encode needs the state of an earlier train_simplex on this Recoder (there is none)")
    m = als.canonical_csr(interactions_matrix)
    n_items = self.simplex_state["E0"][1].shape[0]
    if m.shape[1] > n_items:
      raise ValueError("interactions_matrix has %d columns, the fit has %d items" % (m.shape[1], n_items))
    m = sp.csr_matrix((m.data, m.indices, m.indptr), shape=(m.shape[0], n_items))
    return simplex.encode(als.AlsCSR(m, self.device), self.simplex_state)

  def fold_in(self, interactions_matrix, alpha=30.0, reg=100.0):
    """[B, h] f32 on the device: the user rows of the B histories (the rows of ``interactions_matrix``, a scipy
    matrix over the model's items), users no fit has seen included, for a MatrixFactorization with activation
    'none' left by any trainer (recoder_amd/foldin.py).  A row is the exact minimiser of the ALS user objective
    sum_i (1 + ``alpha`` [r_i > 0]) (r_i - x . y_i - b_i)^2 + ``reg`` |x|^2 over all items with the item table
    and the bias held as they stand, solved by Cholesky on the device (rk_als_foldin, embedding sizes up to
    ``foldin.MAX_H``).  ``alpha = 0, reg = 0`` after ``train_svd`` gives the model's own rows; after ``train_als``
    the loss's confidence and the fit's ``reg`` give the exact user half-step.  Nothing of the model is changed.
    ValueError: another model class or activation, a larger embedding size, ``alpha`` or ``reg`` below 0, a model
    not yet initialised, more than one rank, a matrix with more columns than the model has items.  A row whose
    system is not positive definite (``reg = 0`` only) is returned as zeros, with one warning per call."""
    from . import foldin
    return foldin.fold_in(self, interactions_matrix, alpha, reg)

  def recommend_folded(self, users_interactions, num_recommendations, alpha=30.0, reg=100.0):
    """``recommend_array`` with the batch's user rows folded in from their histories (``fold_in`` of
    ``users_interactions.interactions_matrix``) instead of looked up in the user table: [users, k] int64 item ids,
    the seen items masked, ties to the lower id.  ``users_interactions.users`` is ignored, so the users need not
    be the fit's."""
    rows = self.fold_in(users_interactions.interactions_matrix, alpha, reg)
    ids, _ = self._recommend_device(users_interactions, num_recommendations, user_rows=rows)
    return ids.cpu().numpy().copy()

  def recommend_filtered(self, users_interactions, num_recommendations, filter_seen=True, allow_items=None,
                         deny_items=None, user_allow=None, user_deny=None, return_scores=False, route="auto",
                         user_rows=None):
    """``recommend_array`` under item filters, with scores on request (recoder_amd/serve.py): [users, k] int64 ids
    and, with ``return_scores``, the f32 [users, k] values the ranking ranked.  Item c is eligible for row r when
    it is not a stored POSITIVE entry of the row (``filter_seen``), is in ``allow_items`` (None: all) and not in
    ``deny_items`` (1-D integer ids, duplicates allowed, or a boolean array over the items), is in row r of
    ``user_allow`` (None: all) and not in row r of ``user_deny`` (scipy sparse [users, n_items], only the pattern
    counts).  The eligible items come by (score descending, id ascending); a row with e < k of them returns its e
    items, then id -1 with score -inf.  With every filter at its default the ids are ``recommend_array``'s.
    ``route``: "mask" runs the filters as a bitmap through the strips of ``recommend`` (every model); "pairs"
    scores only the candidates of ``user_allow`` (a MatrixFactorization with activation 'none' on the fused engine,
    at most ``serve.PAIRS_MAX_ROW`` candidates a user); "auto" takes "pairs" whenever it is legal.  The two rank the
    same set by the same rule, but the strips multiply split fp16 planes and the pair kernel plain f32: their score
    bits, and on near-ties their ids, may differ.  ``user_rows``: ``fold_in``'s [users, h] device tensor, scored
    in place of the users' own rows.  ValueError: an id out of range, a wrong shape, k above ``rk_topk_max_k()`` or
    the number of items, the generic torch-autograd engine (there is no dense fallback), an illegal ``route``."""
    from . import serve
    return serve.recommend_filtered(self, users_interactions, num_recommendations, return_scores=return_scores,
                                    filter_seen=filter_seen, allow_items=allow_items, deny_items=deny_items,
                                    user_allow=user_allow, user_deny=user_deny, route=route, user_rows=user_rows)

  def rerank(self, users_interactions, candidates, num_recommendations, return_scores=False, route="auto"):
    """The best ``num_recommendations`` of every user's ``candidates`` (scipy sparse [users, n_items], the pattern):
    ``recommend_filtered(filter_seen=False, user_allow=candidates)``, seen items included when they are candidates."""
    return self.recommend_filtered(users_interactions, num_recommendations, filter_seen=False, user_allow=candidates,
                                   return_scores=return_scores, route=route)

  def explain(self, users_interactions, items, num_contributors=5, alpha=30.0, reg=100.0):
    """Why were these items served: for the batch's B users and the targets ``items`` (integer [B, J], J >= 1,
    typically what ``recommend_array``, ``recommend_filtered`` or ``rerank`` returned; -1 padding and duplicates are
    allowed) the ``num_contributors`` = m (1..64) items of each user's history that carry most of each target's
    score (recoder_amd/explain.py).  Returns an ``explain.Explanation`` of host numpy arrays:
    ``contributors`` int64 [B, J, m], history item ids by contribution, largest first, equal values to the smaller
    id, a NaN behind every number, -1 where the history has fewer than m entries or the target is -1;
    ``contributions`` f32 [B, J, m], their values, 0.0 at padding (a negative contribution is an ordinary value, kept
    when fewer than m larger ones exist); ``baseline`` f32 [B, J], the part of the score that belongs to no history
    item; ``total`` f32 [B, J], ALL of the history's contributions plus the baseline: the score being explained.
    Exact for both families that are linear in the history.  The item-item models (ShallowAutoencoder,
    GraphFilterModel, AdmmSlimModel, RandomWalkItemModel, SparseLinearModel, ItemNeighbourhoodModel): the contribution
    of history item i to target j is x_ui W[i, j], the baseline 0 and ``total`` ``predict``'s score.  A
    MatrixFactorization with activation 'none' and an embedding size up to ``foldin.MAX_H``: the user is ALWAYS the
    folded-in one (``fold_in`` with ``alpha`` and ``reg``, which are read for this model only), known and unseen users
    alike, so ``total`` is the score ``recommend_folded`` ranks by, NOT the score of the trained user row; the
    baseline is b_j - z . v.  A target that is itself in the history is explained like any other; a user with an
    empty history gets padding and total = baseline.  ValueError, naming the model's class, before any GPU work:
    any other model class, another activation, a larger embedding size, a model not yet fitted, more than one rank,
    an id outside [-1, n_items), ``items`` with another row count than the batch, m outside 1..64."""
    from . import explain
    return explain.explain(self, users_interactions, items, num_contributors, alpha, reg)

  def train_svd(self, train_dataset, num_power_iterations=6, oversample=16, seed=0):
    """PureSVD (Cremonesi, Koren & Turrin 2010) for a MatrixFactorization with activation 'none'
    (recoder_amd/svd.py): the item table becomes V, the top ``embedding_size`` right singular vectors of
    the dataset's interaction matrix A (values as stored), the user table U = A V, the bias 0, so that a
    user's scores are the row of ``A V V^T``.  V comes from a randomized SVD with a sketch of
    ``embedding_size + oversample`` columns and ``num_power_iterations`` power iterations, seeded by
    ``seed``; a fixed seed gives the same bits.  The configured ``loss`` plays no part.  Builds a fresh
    optimizer of ``optimizer_type``, so that ``save_state``, ``train`` and ``train_als`` work on the
    tables it leaves.  Returns (and keeps in ``svd_info``) h, l, nnz, the singular values, the
    milliseconds of the sparse products and of the orthonormalisations (HIP events), those of the host's
    eigendecomposition, and ``ritz_residual`` = max_k |A^T u_k - sigma_k^2 v_k| / sigma_1^2: flat spectra
    converge slowly, and this is the signal to raise ``num_power_iterations``."""
    from . import svd

    def sizes(l, n_users, n_items, nnz, **free):
      svd.check_rank(l, n_users or 0, n_items or 0)
      svd.check_memory(n_users, n_items, l, nnz, **free)

    def fit(m, pair, c):
      info = svd.fit(*_mf_tables(m), *pair, int(oversample), int(num_power_iterations), int(seed))
      m.bias.data.zero_()
      return info
    return self._closed_form_fit(
        svd, train_dataset, "svd_info", fit=fit,
        check=lambda m: svd.check_config(m, oversample, num_power_iterations, seed),               # c = (h, l)
        hint_check=lambda c, u, n, host: sizes(c[1], u, n, 0, free_bytes=float("inf")),
        size_check=lambda c, host: sizes(c[1], self.num_users, self.num_items, host().nnz),
        log_line=lambda c: ("PureSVD: h %d, l %d, %d power iterations, seed %d",) + c + (num_power_iterations, seed))

  def train_ease(self, train_dataset, reg=None):
    """The closed-form EASE fit of a ShallowAutoencoder (recoder_amd/ease.py): ``item_weights`` becomes
    ``-P / diag(P)`` by columns with a zero diagonal, ``P = (X^T X + reg I)^-1`` for the dataset's
    interaction matrix X (values as stored).  ``reg`` None takes the model's; an explicit value is stored
    back into the model, so that a checkpoint's ``model_params`` describe the weights it holds.  The
    configured ``loss`` plays no part: EASE minimises the squared error with an L2 penalty by
    construction.  Builds a fresh optimizer of ``optimizer_type`` so that ``save_state`` works.  Returns
    ``info``: n, nnz, reg and the milliseconds of the Gram, the inverse and finalize (HIP events)."""
    from . import ease
    return self._closed_form_fit(
        ease, train_dataset, "ease_info", copy=lambda info: {k: v for k, v in info.items() if k != "diag"},
        check=lambda m: ease.check_config(m, _default(reg, m, "reg")),
        hint_check=lambda c, u, n, host: n and ease.check_memory(n, free_bytes=float("inf")),
        log_line=lambda reg: ("EASE: reg %g", reg), store=lambda reg: {"reg": reg},
        # (first use: the parameter itself is the n x n matrix, and it has to fit what is free)
        place=lambda reg, first, host: first and ease.check_memory(self._size_hints(train_dataset)[1] or 1),
        fit=lambda m, pair, reg: ease.fit(pair, reg, out=m.item_weights.data)[-1])

  def train_gfcf(self, train_dataset, rank=None, alpha=None, oversample=16, num_power_iterations=6, seed=0):
    """The closed-form GF-CF fit of a GraphFilterModel (recoder_amd/gfcf.py): ``item_weights`` becomes
    ``W = Rn^T Rn + alpha * D_I^-1/2 V V^T D_I^1/2`` for ``Rn = D_U^-1/2 R D_I^-1/2``, R the dataset's interaction
    graph (the stored entries are the edges, as in ``train_rp3beta``; their values play no part in the fit,
    they weigh the user's history when scoring) and V its top ``rank`` right singular vectors, from the
    randomized SVD of ``train_svd`` with a sketch of ``rank + oversample`` columns (at most 512),
    ``num_power_iterations`` power iterations and ``seed``; a fixed seed gives the same bits.  ``None`` takes
    the model's value; explicit values are stored back into the model, so that a checkpoint's ``model_params``
    describe the weights it holds.  The n x n matrix has to fit the device (EASE's limit; ValueError
    otherwise).  The configured ``loss`` plays no part.  Builds a fresh optimizer of ``optimizer_type`` so that
    ``save_state`` works.  Returns (and keeps in ``gfcf_info``, there with ``V``, the device tensor of the
    singular vectors) n, nnz, rank, alpha, l, singular_values, ritz_residual (flat spectra converge slowly:
    the signal to raise ``num_power_iterations``) and gram_ms, svd_ms and filter_ms (HIP events)."""
    from . import gfcf, svd

    def sizes(c, n_users, n_items, nnz, **kw):
      gfcf.check_memory(n_users or 0, n_items, c[2], nnz, **kw)
      svd.check_rank(c[2], n_users or 0, n_items or 0)

    def place(c, first, host):
      # (first use: the parameter itself is the n x n matrix, and it has to fit what is free)
      if first:
        n_users, n_items = self._size_hints(train_dataset)
        gfcf.check_memory(n_users or 0, n_items or 1, c[2], host().nnz)
    return self._closed_form_fit(
        gfcf, train_dataset, "gfcf_info", copy=lambda info: {k: v for k, v in info.items() if k != "V"},
        check=lambda m: gfcf.check_config(m, _default(rank, m, "rank"), _default(alpha, m, "alpha"), oversample,
                                          num_power_iterations, seed),                      # c = (rank, alpha, l)
        hint_check=lambda c, u, n, host: n and sizes(c, u, n, 0, free_bytes=float("inf")),
        log_line=lambda c: ("GF-CF: rank %d, alpha %g, l %d, %d power iterations, seed %d",) + c
        + (num_power_iterations, seed),
        store=lambda c: {"rank": c[0], "alpha": c[1]}, place=place,
        size_check=lambda c, host: sizes(c, self.num_users, self.num_items, host().nnz, allocate_matrix=False),
        fit=lambda m, pair, c: gfcf.fit(pair, c[0], c[1], int(oversample), int(num_power_iterations), int(seed),
                                        out=m.item_weights.data)[-1])

  def train_admm_slim(self, train_dataset, l1_reg=None, l2_reg=None, rho=None, num_iterations=None, nonneg=None):
    """The ADMM-SLIM fit of an AdmmSlimModel (recoder_amd/admm.py): ``item_weights`` becomes the sparse iterate C
    after ``num_iterations`` iterations of ADMM with penalty ``rho`` on SLIM's objective ``1/2 |X - X B|^2 +
    l2_reg/2 |B|^2 + l1_reg |B|_1`` with a zero diagonal, over the dataset's interaction matrix X (values as stored;
    with ``nonneg``, B >= 0 and the values must be >= 0: ValueError otherwise).  Each iteration is a ridge step on
    ``(X^T X + (l2_reg + rho) I)^-1`` (EASE's Gram and inverse, one dense n^3 product) and a soft-threshold at
    ``l1_reg / rho``.  ``None`` takes the model's value; explicit values are stored back into the model, so that a
    checkpoint's ``model_params`` describe the weights it holds.  Five n x n matrices have to fit the device
    (ValueError otherwise).  The configured ``loss`` plays no part.  Builds a fresh optimizer of ``optimizer_type``
    so that ``save_state`` works.  Returns (and keeps in ``admm_info``) n, nnz, the hyperparameters, iterations,
    primal_residual and dual_residual (per iteration: |B - C|_F and rho |C - C_previous|_F), density (the share of
    non-zeros of C) and gram_ms, inverse_ms and admm_ms (HIP events)."""
    from . import admm
    m = self.model
    names = ("l1_reg", "l2_reg", "rho", "num_iterations", "nonneg")
    given = (l1_reg, l2_reg, rho, num_iterations, nonneg)
    return self._closed_form_fit(
        admm, train_dataset, "admm_info", check_values=_default(nonneg, m, "nonneg") is True,
        check=lambda m: admm.check_config(m, *(_default(v, m, k) for v, k in zip(given, names))),
        hint_check=lambda c, u, n, host: n and admm.check_memory(n, c[3], free_bytes=float("inf")),
        log_line=lambda c: ("ADMM-SLIM: l1_reg %g, l2_reg %g, rho %g, %d iterations, nonneg %s",) + c,
        store=lambda c: dict(zip(names, c)),
        # (first use: the parameter itself is one of the n x n matrices, and all have to fit what is free)
        place=lambda c, first, host: first and admm.check_memory(self._size_hints(train_dataset)[1] or 1, c[3]),
        size_check=lambda c, host: admm.check_memory(self.num_items, c[3], allocate_matrix=False),
        fit=lambda m, pair, c: admm.fit(pair, *c, out=m.item_weights.data)[-1])

  def train_elsa(self, train_dataset, num_epochs=None, batch_size=1024, lr=0.03, seed=0):
    """The ELSA fit of a LowRankShallowAutoencoder (recoder_amd/elsa.py): ``item_factors`` becomes W after
    ``num_epochs`` (None: ``elsa.DEFAULT_EPOCHS``) epochs of mini-batch Adam steps (betas 0.9 / 0.999, eps 1e-8, no weight
    decay) with learning rate ``lr`` on the cosine loss ``mse_loss(normalize(X_b A A^T - X_b), normalize(X_b))`` over
    batches of ``batch_size`` users of the dataset's interaction matrix X (values as stored), A the rows of W at unit
    length.  Loss and gradient come from the h x h Gram ``A^T A``, sparse products over the batch's stored entries and one
    n x h x h product; the batch x items block is never formed.  The start and every epoch's user order are drawn from
    ``seed`` on the host: a fixed seed gives the same bits.  The configured ``loss`` plays no part.  Builds a fresh
    optimizer of ``optimizer_type`` so that ``save_state`` works; the fit's own Adam moments are not kept.  Returns (and
    keeps in ``elsa_history``) the mean batch loss of each epoch."""
    from . import elsa
    return self._closed_form_fit(
        elsa, train_dataset, "elsa_history", copy=list,
        check=lambda m: elsa.check_config(m, elsa.DEFAULT_EPOCHS if num_epochs is None else num_epochs, batch_size, lr,
                                          seed),                       # c = (h, epochs, batch, lr, seed)
        hint_check=lambda c, u, n, host: n and elsa.check_memory(u or 0, n, c[0], c[2], 0, free_bytes=float("inf")),
        log_line=lambda c: ("ELSA: embedding size %d, %d epochs of batches of %d, lr %g, seed %d",) + c,
        # (first use: the parameter itself is one of the five [n, h] tables, and all have to fit what is free)
        place=lambda c, first, host: first and elsa.check_memory(
            self._size_hints(train_dataset)[0] or 0, self._size_hints(train_dataset)[1] or 1, c[0], c[2], host().nnz),
        size_check=lambda c, host: elsa.check_memory(self.num_users, self.num_items, c[0], c[2], host().nnz,
                                                     allocate_model=False),
        fit=lambda m, pair, c: elsa.fit(pair, *c, out=m.item_factors.data)[-1])

  def train_rp3beta(self, train_dataset, alpha=None, beta=None, neighbours=None):
    """The closed-form RP3beta fit of a RandomWalkItemModel (recoder_amd/rp3.py): every item keeps its
    ``neighbours`` largest ``W[i, j] = d_i^-alpha * (sum over the users v of i and j of r_v^-alpha) * d_j^-beta``
    over the dataset's interaction graph (the stored entries are the edges; their values play no part
    in the fit, they weigh the user's history when scoring).  ``None`` takes the model's value; explicit
    values are stored back into the model, so that a checkpoint's ``model_params`` describe the weights it
    holds, and another ``neighbours`` re-allocates the model's tensors.  The configured ``loss`` plays no
    part.  Builds a fresh optimizer of ``optimizer_type`` so that ``save_state`` works.  Returns
    ``info``: n, nnz, alpha, beta, neighbours, kept (entries kept over all rows) and fit_ms (HIP events)."""
    from . import rp3
    return self._neighbour_list_fit(
        rp3, train_dataset, "rp3_info", k_at=2,                                            # c = (alpha, beta, K)
        check=lambda m: rp3.check_config(m, _default(alpha, m, "alpha"), _default(beta, m, "beta"),
                                         _default(neighbours, m, "neighbours")),
        log_line=lambda c: ("RP3beta: alpha %g, beta %g, %d neighbours",) + c,
        store=lambda c: {"alpha": c[0], "beta": c[1]})

  def train_itemknn(self, train_dataset, neighbours=None, shrink=None, similarity=None, feature_weighting=None):
    """The closed-form ItemKNN fit of an ItemNeighbourhoodModel (recoder_amd/itemknn.py): column j of W keeps
    the ``neighbours`` largest ``s_ij / (denominator + shrink)``, ``s_ij = sum over the users v of i and j of
    a_vi a_vj`` over the dataset's interaction matrix (values as stored, finite and >= 0: ValueError
    otherwise; re-weighted by ``feature_weighting`` for the two cosines, taken as 1 by the set similarities).
    ``None`` takes the model's value; explicit values are stored back into the model, so that a checkpoint's
    ``model_params`` describe the weights it holds, and another ``neighbours`` re-allocates the model's
    tensors.  The alpha / beta values of the asymmetric and Tversky similarities are the model's.  The
    configured ``loss`` plays no part.  Builds a fresh optimizer of ``optimizer_type`` so that ``save_state``
    works.  Returns (and keeps in ``itemknn_info``) n, nnz, neighbours, shrink, similarity, feature_weighting,
    kept (entries kept over all columns) and fit_ms (HIP events)."""
    from . import itemknn
    return self._neighbour_list_fit(
        itemknn, train_dataset, "itemknn_info", k_at=0, check_values=True,  # c = (K, shrink, similarity, weighting, ...)
        check=lambda m: itemknn.check_config(
            m, _default(neighbours, m, "neighbours"), _default(shrink, m, "shrink"),
            _default(similarity, m, "similarity"), _default(feature_weighting, m, "feature_weighting")),
        log_line=lambda c: ("ItemKNN: %s similarity, feature weighting %s, %d neighbours, shrink %g", c[2], c[3], c[0],
                            c[1]),
        store=lambda c: {"shrink": c[1], "similarity": c[2], "feature_weighting": c[3]})

  def train_slim(self, train_dataset, l1_reg=None, l2_reg=None, neighbours=None, max_sweeps=50, tol=1e-5,
                 candidates=None, candidate_similarity="cosine", candidate_shrink=0.0):
    """The SLIM fit of a SparseLinearModel (recoder_amd/slim.py): column j of W becomes the non-negative
    elastic-net regression of item j on the other items over the dataset's interaction matrix X (values as
    stored, all >= 0: ValueError otherwise), ``min over w >= 0, w_j = 0 of 1/2 |x_j - X w|^2 + l2_reg/2 |w|^2 +
    l1_reg |w|_1``, by cyclic coordinate descent on the Gram, stopped after the first sweep that moves no
    weight by more than ``tol`` or after ``max_sweeps`` sweeps, and cut to its ``neighbours`` largest
    weights.  ``None`` takes the model's value; explicit values are stored back into the model, so that a
    checkpoint's ``model_params`` describe the weights it holds, and another ``neighbours`` re-allocates the
    model's tensors.  The configured ``loss`` plays no part.  With ``candidates`` None the n x n Gram has to fit
    the device (EASE's limit; ValueError otherwise).  ``candidates`` = M (fsSLIM, section 4.3 of the paper)
    regresses column j on the M items most similar to j only, by an ItemKNN fit with ``candidate_similarity`` and
    ``candidate_shrink`` over the stored values: no n x n buffer exists, and the catalogue is limited by the
    [n, M] lists.  The three are stored in the model (``candidates`` travels in ``model_params`` unless None).
    Builds a fresh optimizer of ``optimizer_type`` so that
    ``save_state`` works.  Returns (and keeps in ``slim_info``) n, nnz, l1_reg, l2_reg, neighbours, kept
    (entries kept over all columns), cut_columns (columns whose support was larger than ``neighbours``),
    unconverged_columns (columns that ran all ``max_sweeps`` sweeps), max_sweeps_run, gram_ms and fit_ms
    (HIP events); with ``candidates`` also candidates, candidate_ms (the ItemKNN fit) and mean_candidates (the
    mean number of a column's candidates that passed the l1 screen)."""
    from . import slim
    return self._neighbour_list_fit(
        slim, train_dataset, "slim_info", k_at=2, check_values=True,
        # c = (l1, l2, K, max_sweeps, tol, candidates, candidate_similarity, candidate_shrink)
        check=lambda m: slim.check_config(m, _default(l1_reg, m, "l1_reg"), _default(l2_reg, m, "l2_reg"),
                                          _default(neighbours, m, "neighbours"), max_sweeps, tol) +
        slim.check_candidates(candidates, candidate_similarity, candidate_shrink),
        log_line=lambda c: ("SLIM: l1_reg %g, l2_reg %g, %d neighbours, at most %d sweeps, tol %g",) + c[:5]
        if c[5] is None else
        ("SLIM: l1_reg %g, l2_reg %g, %d neighbours, at most %d sweeps, tol %g, %d candidates by %s, shrink %g",) + c,
        store=lambda c: {"l1_reg": c[0], "l2_reg": c[1], "candidates": c[5], "candidate_similarity": c[6],
                         "candidate_shrink": c[7]},
        memory=lambda c: {"candidates": c[5]})

  def train_userknn(self, train_dataset, neighbours=None, shrink=None):
    """The "fit" of a UserNeighbourhoodModel (recoder_amd/userknn.py): the model takes the dataset's
    interaction matrix X, as both CSRs with the values as stored, and the users' norms.  At serving time a
    query keeps its ``neighbours`` most similar training users by ``|H_q and H_v| / (sqrt(|H_q|) sqrt(|H_v|) +
    shrink)`` over the item sets and scores ``sum of sim * X[v, :]``; a training user identical to the query is
    not excluded.  ``None`` takes the model's value; explicit values are stored back into the model, so that
    a checkpoint's ``model_params`` describe it.  Another call replaces the matrix: that is how new
    interactions take effect.  The configured ``loss`` plays no part.  Builds a fresh optimizer of
    ``optimizer_type`` so that ``save_state`` works.  Returns (and keeps in ``userknn_info``) n_users, n, nnz,
    neighbours, shrink and fit_ms (HIP events)."""
    from . import userknn

    def place(c, first, host):
      m, nnz = self.model, int(host().nnz)
      if first:
        m.nnz = nnz
      elif (m.num_users, m.nnz) != (self.num_users, nnz):
        m.allocate(self.num_users, nnz, self.device)
    return self._closed_form_fit(
        userknn, train_dataset, "userknn_info", place=place,                               # c = (N, shrink)
        check=lambda m: userknn.check_config(m, _default(neighbours, m, "neighbours"),
                                             _default(shrink, m, "shrink")),
        hint_check=lambda c, u, n, host: u and n and userknn.check_memory(u, n, c[0], host().nnz,
                                                                          free_bytes=float("inf")),
        log_line=lambda c: ("UserKNN: %d neighbours, shrink %g",) + c,
        store=lambda c: {"neighbours": c[0], "shrink": c[1]},
        size_check=lambda c, host: userknn.check_memory(self.num_users, self.num_items, c[0], host().nnz),
        fit=lambda m, pair, c: userknn.fit(pair, *c, model=m)[-1])

  def _pick_engine_for(self, train_dataset):
    """Combinations the fused step does not cover train through the generic engine (torch autograd
    on the GPU, recoder_amd/generic.py) instead of raising -- the reference trains all of them
    (model.py:464-476, nn.py:191-202): tied weights with a separate target matrix."""
    has_target = getattr(train_dataset, "target_interactions_matrix", None) is not None or \
        (hasattr(train_dataset, "device_target_csr") and train_dataset.device_target_csr() is not None)
    tied = self._fused_kind() == "ae" and bool(getattr(self.model, "is_constrained", False))
    force = "tied weights with a separate target matrix" if (has_target and tied) else None
    if force != getattr(self, "_force_generic", None):
      self._force_generic = force
      if self.__engine is not None:
        # the engine is rebuilt for this call; the optimizers (and their state) stay
        if hasattr(self.__engine, "sync_optimizer_steps"):
          self.__engine.sync_optimizer_steps()
        self.__engine = None
      if force:
        log.warning("%s has no fused HIP step: training through torch autograd on the GPU", force)

  def _sync_user_rows(self):
    """Bring every replica up to date with the rows other ranks own -- parameters and
    Adam moments -- so that the result equals the single-process run with
    batch_size = N * B (called at the end of train(), before evaluation and before
    checkpoints).  Item parallel: item i's embedding rows / bias live on rank i % N.
    MatrixFactorization under data parallelism: a user's row only receives gradients
    on the rank that holds the user."""
    self._sync_owned_moments()
    ip = getattr(self, "_ip", None)
    if ip is not None:
      m = self.model
      if self._fused_kind() == "mf":
        params = [m.item_embedding_layer.weight, m.bias]     # user rows are replicated
      else:
        params = [m.en_embedding_layer.weight, m.de_bias]
        if not m.is_constrained:
          params.append(m.de_embedding_layer.weight)
      tensors = []
      for w in params:
        tensors.append(w.data)
        for opt in (self.optimizer, self.sparse_optimizer):
          st = opt.state.get(w) if opt is not None else None
          if st:
            tensors += [st["exp_avg"], st["exp_avg_sq"]]
      ip.sync_owned(tensors, self.num_items)
      self._weights_written()
      return
    if getattr(self, "_dp", None) is None or self._fused_kind() != "mf":
      return
    from .parallel import sync_owned_rows
    w = self.model.user_embedding_layer.weight
    tensors = [w.data]
    for opt in (self.optimizer, self.sparse_optimizer):
      st = opt.state.get(w) if opt is not None else None
      if st:
        tensors += [st["exp_avg"], st["exp_avg_sq"]]
    if self._dp_n_users < w.shape[0]:
      tensors = [t[:self._dp_n_users] for t in tensors]
    sync_owned_rows(tensors, self._dp_n_users, self._dp.group)
    self._weights_written()

  def _weights_written(self):
    """Parameters were written through `.data` (no torch version bump: owner-row syncs): the decoder
    weight bound of the split contractions and the evaluation images must be taken again."""
    eng = self._engine()
    if hasattr(eng, "_w_range_stale"):
      eng._w_range_stale = True
      eng._eval_img = None
    if hasattr(self.model, "_weights_written"):       # (a model with derived state of its own: nn.LowRankShallowAutoencoder)
      self.model._weights_written()

  def _setup_data_parallel(self, train_dataset, negative_sampling=True, batch_size=None):
    """Under an initialised torch.distributed group (one process per GPU, backend
    'nccl' = RCCL) the USERS are sharded over the ranks and the gradients are
    all-reduced (recoder_amd/parallel.DataParallel) -- north_star's partitioning and the
    default.  RK_PARALLEL=items shards the item dimension instead (parallel.ItemParallel).
    Returns this rank's shard."""
    import torch.distributed as dist
    self._dp = None
    self._ip = None
    self._dp_nnz_cap = {}                  # (keyed on id(matrix): never survives the matrix it was taken for)
    # (a previous data-parallel train() may have left the engine on owned-row Adam: a run that does not
    # reach _setup_owned_rows -- no group, the replicated fallback -- must get the one-call step back)
    eng0 = getattr(self, "_Recoder__engine", None)
    if eng0 is not None:
      eng0.owned_rows = False
      eng0.zero_adam = False
    if getattr(self, "_ip_override", None) is not None:
      # tests: several virtual ranks in one process, collectives injected
      return self._enable_item_parallel(self._ip_override, train_dataset)
    dp = getattr(self, "_dp_override", None)
    if dp is None:
      if not (dist.is_available() and dist.is_initialized()):
        return train_dataset
      if dist.get_world_size() == 1 and os.environ.get("RK_FORCE_DP") != "1":
        return train_dataset
    if self._use_generic() or train_dataset.device_target_csr() is not None:
      # no sharded formulation for these: every rank trains the same replica on the whole data
      # (identical results on every rank, no speed-up) instead of refusing to run
      log.warning("multi-GPU training covers the fused DynamicAutoencoder / MatrixFactorization step "
                  "without a separate target matrix: running this configuration replicated on "
                  "every rank")
      if dp is None:
        for p_ in self.model.parameters():        # identical replicas whatever each process seeded
          dist.broadcast(p_.data, src=0)
        self._weights_written()
      return train_dataset
    if dp is None:
      for p_ in self.model.parameters():          # identical replicas: rank 0's initial weights
        dist.broadcast(p_.data, src=0)
    mode = os.environ.get("RK_PARALLEL", "users")
    if mode == "auto":
      mode = "users"
    if mode == "items" and not negative_sampling:
      # without sampling every rank's block spans the whole catalogue, but an item shard only
      # holds its own columns' targets: the loss over the other columns would be wrong
      log.warning("RK_PARALLEL=items needs negative_sampling=True; sharding the users instead")
      mode = "users"
    if mode == "items" and dp is None:
      from .parallel import ItemParallel
      return self._enable_item_parallel(ItemParallel(), train_dataset)
    from .parallel import DataParallel, shard_range
    if dp is None:
      dp = DataParallel().prepare(self.device)
    dp.attach(self._engine())
    self._dp = dp
    self._setup_owned_rows(dp, train_dataset, negative_sampling, batch_size)
    self._setup_local_sets(dp, negative_sampling)
    self._setup_zero_adam(dp)
    n = len(train_dataset)
    lo, hi = shard_range(n, dp.rank, dp.world)
    dp.user_offset = lo
    self._dp_n_users = n
    if hasattr(train_dataset, "row_shard"):           # data.DeviceDataset: sliced in HBM
      shard = train_dataset.row_shard(lo, hi)
    elif getattr(train_dataset, "_dev", None) is not None:
      # a host dataset whose matrix is already resident (dataset.device_csr() was called): this
      # rank's rows are a device-side slice of it -- no host slicing, no second upload
      from .data import DeviceDataset
      shard = DeviceDataset(train_dataset._dev.row_slice(lo, hi))
    else:
      shard = RecommendationDataset(train_dataset.interactions_matrix[lo:hi])
    # every rank runs the same number of equally sized steps (collectives in lockstep)
    self._dp_users_per_epoch = n // dp.world
    return shard

  def _setup_owned_rows(self, dp, train_dataset, negative_sampling, batch_size):
    """Owned-row Adam (parallel.DataParallel): with SparseAdam embedding tables every item's rows -- and
    their moments -- belong to one rank; RK_DP_OWNED=0 keeps the replicated update.  The item-id ranges
    are balanced by the items' expected presence in a global batch, from the training matrix's column
    counts (the same on every rank: it is taken before the users are sharded)."""
    eng = self._engine()
    eng.owned_rows = False
    dp.owner_bounds = None
    sparse = bool(getattr(self.model, "sparse", False)) and self.sparse_optimizer is not None
    # RK_DP_OWNED: 0 = replicated update; 1 = owned rows with more than one rank; force = also with one rank
    # (tests); auto (default) = owned rows only where their price is paid back.  The replicated update
    # replays as HIP graphs with its collectives captured (every engine, round 5); the owned-row exchange
    # moves row counts only the host knows -- a device -> host read, ~25 launches enqueued one by one and the
    # received rows scattered into the tables per step: one forced rank, C4 0.266 vs 0.129 ms per step,
    # C5-shaped 1.43 vs 0.79 (profiles/r05_bench_c*_dp1_*.json).  What it saves is (1 - 1/N) of the
    # SparseAdam sweep over the union rows.
    mode = os.environ.get("RK_DP_OWNED", "auto")
    if not (sparse and negative_sampling and batch_size and (dp.world > 1 or mode == "force") and mode != "0"):
      return
    if dp.virtual and dp._gather_fn is None:
      return                                # (injected collectives without a gather: replicated update)
    dev = getattr(train_dataset, "_dev", None)
    n_items = int(self.num_items)
    if dev is not None:
      freq = torch.bincount(dev.indices[:dev.nnz].long(), minlength=n_items).cpu().numpy()
    else:
      freq = np.bincount(train_dataset.interactions_matrix.indices, minlength=n_items)
    from .parallel import DataParallel
    if mode == "auto":
      est = DataParallel.owned_rows_estimate(freq[:n_items], len(train_dataset), dp.world * int(batch_size),
                                             dp.world, int(eng.h[0]),
                                             1 if (eng.kind != "ae" or bool(self.model.is_constrained)) else 2)
      self._dp_owned_estimate = est
      if est["saved_us"] < 2.0 * est["cost_us"]:
        return
    dp.set_owner_bounds(DataParallel.balanced_bounds(freq[:n_items], len(train_dataset),
                                                     dp.world * int(batch_size), dp.world))
    eng.owned_rows = True

  def _setup_local_sets(self, dp, negative_sampling):
    """RK_DP_ITEMSETS = union (default) | local.  `local` (opt-in, NOT the reference's single-process semantics):
    every rank samples its negatives from the items of ITS OWN B users -- what the reference's trainer would do
    under conventional DDP -- instead of the union over all ranks' users (data.py:216-223 read as one shared item
    set).  The contractions then stop growing with the number of ranks (C2: 7.8 k items per rank instead of 18.4 k
    at 8 ranks) and no stamp exchange precedes the collation; the ranks' compact columns differ, so the gradients
    travel laid out by item id (dense Adam tables of the one-call autoencoder step only).  Its oracle is
    oracle.recoder_oracle.OracleRecoder.train_step_ddp (gradient accumulation over the ranks' batches)."""
    eng = self._engine()
    dp.local_sets = False
    if os.environ.get("RK_DP_ITEMSETS", "union") != "local":
      return
    if getattr(eng, "generic", False) or getattr(eng, "owned_rows", False) or not eng.c_step_eligible():
      return
    if bool(getattr(self.model, "sparse", False)) or self.optimizer is None or not negative_sampling:
      return
    if dp.virtual and dp._gather_fn is None:
      return
    dp.local_sets = True

  def _setup_zero_adam(self, dp):
    """Sharded dense Adam (parallel.DataParallel, "ZeRO-1"): with optim.Adam on the embedding tables of the
    one-call autoencoder step every rank owns an equal range of table rows -- gradient rows reduce-scattered,
    the sweep over 1/N of the rows, the updated rows all-gathered; the moments of a row are kept up to date on
    its owner only and gathered before checkpoints / validation (_sync_owned_moments).  RK_DP_ZERO = 0 (default) |
    1 (with more than one rank) | force (also with one rank: tests, the one-rank bench line).  OPT-IN: the
    exchange then moves the DENSE layout (every row of the tables, = the capacity-sized exchange of a replayed
    step) where the replicated update's moves the union rows, and by tools/dp_model.py the saved (1 - 1/N) of
    the sweep only pays for that at 8 ranks, by 1-3 % (C2 282 vs 290, C3 624 vs 627 us per step at 1 TB/s per
    rank; 2 and 4 ranks lose 5-15 %) -- a model: no run on more than one GPU exists, and a path that has never
    met a second RCCL rank is not what the first 8-GPU run should take by default."""
    eng = self._engine()
    eng.zero_adam = False
    dp.zero = None
    mode = os.environ.get("RK_DP_ZERO", "0")
    if not ((mode == "1" and dp.world > 1) or mode == "force"):
      return
    if getattr(eng, "generic", False) or getattr(eng, "owned_rows", False) or not eng.c_step_eligible():
      return
    if bool(getattr(self.model, "sparse", False)) or self.optimizer is None:
      return                                # (SparseAdam tables: the replicated or the owned-row update)
    if dp.virtual and dp._gather_fn is None:
      return
    dp.setup_zero(int(self.num_items))
    eng.zero_adam = True

  def _sync_owned_moments(self):
    """The Adam moments of the owned rows live on their owners: every replica gets them (checkpoints,
    the end of train(), a later single-process continuation)."""
    dp = getattr(self, "_dp", None)
    eng = self._engine()
    if dp is not None and getattr(eng, "zero_adam", False) and dp.zero is not None:
      # (sharded dense Adam: the moments of rows [lo_r, hi_r) are current on rank r only)
      names = ["en_embedding_layer.weight"] + ([] if self.model.is_constrained else ["de_embedding_layer.weight"])
      for name in names:
        st = eng.states[name]
        dp.sync_owned_moments([st.m, st.v], bounds=dp.zero_bounds())
      return
    if dp is None or not getattr(eng, "owned_rows", False):
      return
    for name, _ in eng._sparse_tables():
      st = eng.states[name]
      dp.sync_owned_moments([st.m, st.v])

  def _enable_item_parallel(self, ip, train_dataset):
    from .parallel import ItemParallel
    full = train_dataset.interactions_matrix
    dev = getattr(train_dataset, "_dev", None)
    on_device = dev is not None and (full is None or dev.implicit)
    if on_device:
      # the matrix is resident in HBM (a DeviceDataset has no host copy at all): the row statistics
      # and this rank's column shard are taken there (implicit feedback: exactly the host's numbers)
      ip.user_norm_dev = ItemParallel.user_norms_dev(dev)
      ip.user_tsum_dev = ItemParallel.user_target_sums_dev(dev)
    else:
      ip.user_norm_dev = torch.from_numpy(ItemParallel.user_norms(full)).to(self.device)
      ip.user_tsum_dev = torch.from_numpy(ItemParallel.user_target_sums(full)).to(self.device)
    ip.prepare(self.device)
    self._engine().item_parallel = ip
    self._ip = ip
    if on_device:
      from .data import DeviceDataset
      return DeviceDataset(ip.shard_device_csr(dev))
    return RecommendationDataset(ip.shard_csr(full))

  def _make_block(self, dcsr, S, negative_sampling, train=False):
    """train: a block of the (sharded) training matrix; validation / target blocks are
    collated from unsharded matrices and get the plain capacity."""
    nnz_cap = max(1, _top_sum(dcsr.degrees, S))
    n_cap = nnz_cap
    if train and getattr(self, "_dp", None) is not None and not getattr(self._dp, "local_sets", False):
      # the union item set can exceed one rank's nnz bound; the SAME capacity on every rank (a
      # rank with lighter users would otherwise clamp n_b on its own and the gradient exchange
      # would disagree on its sizes): MAX over the ranks, once per (matrix, group size)
      cache = self.__dict__.setdefault("_dp_nnz_cap", {})
      key = (id(dcsr), int(S))
      if key not in cache:
        t = torch.tensor([nnz_cap], dtype=torch.int32, device=self.device)
        cache[key] = int(self._dp.union_marks(t).max().item())
      n_cap = min(dcsr.n_items, cache[key] * self._dp.world)
    if train and getattr(self, "_ip", None) is not None and negative_sampling:
      n_cap = min(nnz_cap, -(-dcsr.n_items // self._ip.world))   # at most the owned items
    return Block(S, nnz_cap, dcsr.n_items, self.device, negative_sampling=negative_sampling,
                 n_cap=n_cap)

  def _step_generator(self, dataloader):
    """Yields (blk, row_off, B, keep_noise, keep_drop, tgt_blk) for one pass over the
    dataset: the device-side equivalent of iterating the reference's
    RecommendationDataLoader (data.py:138-144).  tgt_blk: the same rows collated from the
    dataset's target matrix (its own item set, data.py:60-62), or None."""
    ds = dataloader.dataset
    dcsr = ds.device_csr()
    dcsr_t = ds.device_target_csr()
    tgt_blk = None
    if dcsr_t is not None:
      tgt_blk = getattr(self, "_train_tgt_blk", None)
      if tgt_blk is None or tgt_blk.S_cap < dataloader.num_sampling_users or \
          getattr(self, "_train_tgt_src", None) is not dcsr_t or \
          tgt_blk.negative_sampling != dataloader.negative_sampling:
        tgt_blk = self._make_block(dcsr_t, dataloader.num_sampling_users,
                                   dataloader.negative_sampling)
        self._train_tgt_blk, self._train_tgt_src = tgt_blk, dcsr_t
    B, S = dataloader.batch_size, dataloader.num_sampling_users
    pf = getattr(self, "_train_pf", None)
    dp = getattr(self, "_dp", None)
    if pf is None or pf.dcsr is not dcsr or pf.blocks[0][0].S_cap < S or \
        pf.blocks[0][0].negative_sampling != dataloader.negative_sampling or \
        getattr(pf, "owner_dp", None) is not dp:
      from .device import CollatePrefetcher
      ns = dataloader.negative_sampling
      pf = CollatePrefetcher(lambda: self._make_block(dcsr, S, ns, train=True), dcsr, self.device,
                             collate_fn=(dp.collate if dp is not None else None),
                             group=self.prefetch_group)
      pf.owner_dp = dp
      self._train_pf = pf
    pf.reset()
    n = len(ds)
    order, self._pending_order = getattr(self, "_pending_order", None), None
    if order is None and self.user_order_hook is not None:
      order = self.user_order_hook(self.current_epoch, n)
    if order is None:
      order = epoch_user_order(n)
    if getattr(self, "_ip", None) is not None:
      o = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int64)).to(self.device)
      order = self._ip.broadcast(o).cpu().numpy()   # one user order for all item shards
    if getattr(self, "_dp", None) is not None:
      order = order[:self._dp_users_per_epoch]      # equal step counts on every rank
      n = len(order)
    order_dev = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int64)).to(self.device)
    offs = [o for o in range(0, n, S) if order_dev[o:o + S].numel() > 0]
    G = pf.group
    # chunks of up to G sampling groups; a chunk never straddles a step mark
    marks = self.step_marks
    step0 = getattr(self, "_global_step", 0)
    first_step, k = {}, step0
    for o in offs:
      first_step[o] = k
      k += -(-min(S, n - o) // B)
    chunks = []
    for o in offs:
      if not chunks or len(chunks[-1]) == G or first_step[o] in marks:
        chunks.append([])
      chunks[-1].append(o)
    users_of = lambda chunk: [order_dev[o:o + S] for o in chunk]
    marked = lambda ci: first_step[chunks[ci][0]] in marks
    submitted = set()

    def submit(ci):
      if ci < len(chunks) and ci not in submitted:
        submitted.add(ci)
        pf.submit(ci % 2, users_of(chunks[ci]))
    # the chunk after the current one is collated on the prefetcher's side stream (unless it
    # starts at a mark: then nothing of it may be in flight before the mark's callback ran)
    if chunks and not marked(0):
      submit(0)
    for ci, chunk in enumerate(chunks):
      slot = ci % 2
      if marked(ci):
        if marks[first_step[chunk[0]]]():
          self._stop_training = True
          return
      submit(ci)
      if ci + 1 < len(chunks) and not marked(ci + 1):
        submit(ci + 1)
      for blk, off in zip(pf.acquire(slot), chunk):
        Sg = int(order_dev[off:off + S].numel())
        if tgt_blk is not None:
          tgt_blk.collate(dcsr_t, order_dev[off:off + S])
        keep_noise = keep_drop = None
        if self.mask_hook is not None:
          keep_noise, keep_drop = self.mask_hook(self._global_step, order[off:off + S])
        for r in range(0, Sg, B):
          rows = min(B, Sg - r)
          kd = None
          if keep_drop is not None:
            kd = keep_drop[r:r + rows].contiguous()
          eps = None
          if self.eps_hook is not None:
            # (the consumer has counted the steps before this one: _global_step is this step's index)
            eps = self.eps_hook(self._global_step, order[off + r:off + r + rows])
            if eps is not None:
              eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous()
          yield blk, r, rows, keep_noise, kd, tgt_blk, eps
      pf.release(slot)

  def _train(self, train_dataloader, val_dataloader, num_epochs, current_epoch, lr_scheduler,
             batch_size, model_checkpoint_prefix, checkpoint_freq, eval_freq, metrics,
             eval_num_recommendations, iters_per_epoch, eval_num_users, eval_batch_size):
    """model.py:349-437."""
    engine = self._engine()
    self._order_ahead = None             # (an order drawn ahead belongs to ONE train() call)
    num_batches = len(train_dataloader)
    iters_processed = 0
    if iters_per_epoch is None:
      iters_per_epoch = num_batches
    self._global_step = getattr(self, "_global_step", 0)
    loss_buf = torch.zeros(max(1, min(iters_per_epoch, num_batches)), dtype=torch.float32,
                           device=self.device)
    iterator = None
    self._stop_training = False
    for epoch in range(current_epoch, num_epochs + 1):
      if self._stop_training:
        break
      self.current_epoch = epoch
      self.model.train()
      self._sync_ranges()
      if lr_scheduler is not None:
        lr_scheduler.step()     # at epoch start, as model.py:364-366
      if iters_processed == 0 or iters_processed == num_batches:
        iters_processed = 0
        iterator = enumerate(self._step_generator(train_dataloader), 1)
      iters_to_process = min(iters_per_epoch, num_batches - iters_processed)
      iters_processed += iters_to_process

      if self._graph_ok(train_dataloader, iters_per_epoch, num_batches):
        # whole epochs of the one-call autoencoder step: replayed as HIP graphs (graph.py)
        iters_processed = num_batches
        # the NEXT epoch's user order is drawn while the GPU still works on this one (torch.randperm
        # of 10^5 users costs 2-11 ms of host time, a quarter of a C2 epoch) -- unless something
        # else would draw from the global RNG in between (validation), a hook supplies the order or
        # this is the last epoch: the SEQUENCE of draws stays the reference's
        ahead = (epoch < num_epochs and self.user_order_hook is None and
                 not (eval_freq > 0 and epoch % eval_freq == 0 and val_dataloader is not None))
        losses = self._train_epoch_graph(train_dataloader, draw_next_order=ahead)
        if losses is not None:
          self.last_epoch_losses = losses
          self._epoch_end(epoch, num_epochs, len(self.last_epoch_losses), val_dataloader, eval_freq,
                          metrics, eval_num_recommendations, eval_batch_size, eval_num_users,
                          model_checkpoint_prefix, checkpoint_freq)
          continue
        # (the hook's order is not one pass over the users: eagerly sequenced steps below)
        iterator = enumerate(self._step_generator(train_dataloader), 1)
        iters_to_process = num_batches

      n_done = 0
      for batch_itr, (blk, row_off, rows, keep_noise, keep_drop, tgt_blk, eps) in iterator:
        dp = getattr(self, "_dp", None)
        engine.train_step(blk, row_off, rows, keep_noise, keep_drop,
                          out=loss_buf[n_done:n_done + 1],
                          global_rows=(rows * dp.world if dp is not None else None), tgt=tgt_blk,
                          **({} if eps is None else dict(eps=eps)))
        n_done += 1
        self._global_step += 1
        if batch_itr % iters_per_epoch == 0:
          break
      if getattr(self, "_ip", None) is not None and n_done:
        self._ip.allreduce_sum(loss_buf[:n_done])   # every rank holds its items' share
      # one device->host read per epoch instead of loss.item() per step (model.py:404)
      self.last_epoch_losses = loss_buf[:n_done].cpu().numpy().copy()
      self._epoch_end(epoch, num_epochs, n_done, val_dataloader, eval_freq, metrics,
                      eval_num_recommendations, eval_batch_size, eval_num_users,
                      model_checkpoint_prefix, checkpoint_freq)

  def _epoch_end(self, epoch, num_epochs, n_done, val_dataloader, eval_freq, metrics,
                 eval_num_recommendations, eval_batch_size, eval_num_users, model_checkpoint_prefix,
                 checkpoint_freq):
    """model.py:406-437: the epoch's log line, validation / evaluation, checkpoint."""
    # (the stream is drained here: the one place where the blocks' overflow flags are read back)
    for holder in (getattr(self, "_train_pf", None), getattr(self, "_graph_stepper", None)):
      if holder is not None:
        for blk in (b for row in holder.blocks for b in row):
          blk.check()
    self.loss_history.append(self.last_epoch_losses)
    if n_done and not np.all(np.isfinite(self.last_epoch_losses)):
      # the reference keeps training on a NaN loss too (the split-fp16 decoder GEMMs take their
      # operand scales from device-side maxima, recoder_amd/csrc/gemm.hip, so they add no way to
      # get one that fp32 does not have)
      log.warning("non-finite training loss in epoch %d", epoch)
    postfix = {"loss": float(self.last_epoch_losses[-1]) if n_done else float("nan")}
    if eval_freq > 0 and epoch % eval_freq == 0 and val_dataloader is not None:
      self._sync_user_rows()
      postfix["val_loss"] = self._validate(val_dataloader)
      if metrics is not None and eval_num_recommendations is not None:
        results = self._evaluate(val_dataloader.dataset,
                                 num_recommendations=eval_num_recommendations,
                                 metrics=metrics, batch_size=eval_batch_size,
                                 num_users=eval_num_users)
        for metric in results:
          postfix[str(metric)] = np.mean(results[metric])
    log.info("Epoch {}/{} {}".format(epoch, num_epochs, postfix))
    self.last_epoch_summary = postfix
    if model_checkpoint_prefix and \
        ((checkpoint_freq > 0 and epoch % checkpoint_freq == 0) or epoch == num_epochs):
      self._sync_user_rows()
      # multi-GPU training (every rank is here): the replicas are identical -- one writer
      # (concurrent writers of one path can truncate each other on a shared filesystem), the
      # others wait for the file
      import torch.distributed as dist
      # (also the replicated fallback of _setup_data_parallel -- generic engine, target matrix --
      # where neither _dp nor _ip is set: every process of an initialised group is here)
      multi = getattr(self, "_dp_override", None) is None and getattr(self, "_ip_override", None) is None and \
          dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
      if not multi or dist.get_rank() == 0:
        self.save_state(model_checkpoint_prefix)
      if multi:
        dist.barrier()

  # ------------------------------------------------------------ graph replay
  def _graph_ok(self, dataloader, iters_per_epoch, num_batches):
    if os.environ.get("RK_GRAPH", "1") == "0":
      return False
    eng = self._engine()
    if getattr(eng, "generic", False):
      return False
    if getattr(self, "_ip", None) is not None:
      return False
    dp = getattr(self, "_dp", None)
    if dp is not None:
      # users-DP replays too when its collectives are our own in-order RCCL calls (capturable) and
      # the step is the one-call autoencoder step; injected collectives (virtual ranks in tests),
      # torch.distributed / gloo and the entry-by-entry engines keep the eager sequencing
      # (round 5: so do the entry-by-entry engines -- MatrixFactorization, hidden stacks -- with the
      # replicated update; owned-row SparseAdam exchanges row counts only the host knows: eager)
      if not (dp.direct and not dp.virtual and not getattr(eng, "owned_rows", False) and
              self.graph_group <= 8):
        return False
    ds = dataloader.dataset
    return (self.mask_hook is None and self.eps_hook is None and
            dataloader.num_sampling_users == dataloader.batch_size and
            ds.device_target_csr() is None and iters_per_epoch == num_batches and
            len(ds) >= dataloader.batch_size)

  def _train_epoch_graph(self, dataloader, draw_next_order=False):
    """One pass over the dataset with the whole-batch steps replayed as HIP graphs
    (recoder_amd/graph.py); returns the per-step losses."""
    from .graph import GraphStepper
    eng = self._engine()
    ds = dataloader.dataset
    dcsr = ds.device_csr()
    B, ns, n = dataloader.batch_size, dataloader.negative_sampling, len(ds)
    gs = getattr(self, "_graph_stepper", None)
    G = max(1, min(self.graph_group, n // B))
    if gs is None or gs.eng is not eng or gs.dcsr is not dcsr or gs.B != B or gs.ns != ns or gs.G != G or \
        gs.dp is not getattr(eng, "allreduce", None) or \
        (not gs.c_step and set(gs.slots) != set(eng.states)):
      if gs is not None:
        gs.close()
      gs = GraphStepper(eng, dcsr, lambda: self._make_block(dcsr, B, ns, train=True), B, ns, G, n,
                        self.device)
      self._graph_stepper = gs
    order = None
    ahead, self._order_ahead = getattr(self, "_order_ahead", None), None
    if self.user_order_hook is not None:
      order = self.user_order_hook(self.current_epoch, n)
    elif ahead is not None and ahead[0] == n:
      order = ahead[1]                     # drawn at the end of the previous epoch
    if order is None:
      order = epoch_user_order(n)
    order = np.ascontiguousarray(order, dtype=np.int64)
    n_draw = n
    if getattr(self, "_dp", None) is not None and order.shape == (n,):
      n = self._dp_users_per_epoch         # equal step counts on every rank (as _step_generator)
      order = np.ascontiguousarray(order[:n])
    if order.shape != (n,):
      # a hook may hand over any list of users (a subset, repeats): the replayed graphs are laid out
      # for one pass over the n users -- this epoch takes the eagerly sequenced path with the SAME
      # order (the hook is not asked twice)
      self._pending_order = order
      return None
    caller = torch.cuda.current_stream()
    gs.main.wait_stream(caller)
    with torch.cuda.stream(gs.main):
      losses = self._run_epoch_graph(gs, eng, dcsr, order, n, B, draw_next_order, n_draw)
    caller.wait_stream(gs.main)
    return losses

  def _run_epoch_graph(self, gs, eng, dcsr, order, n, B, draw_next_order=False, n_draw=None):
    n_full = gs.begin_epoch(order, eng.rng_step)
    n_total = n_full + (1 if n % B else 0)
    g0 = self._global_step
    # (a mark is called BEFORE step m is enqueued: one that coincides with the end of this epoch
    # belongs to the first step of the next one -- as in the eager path)
    marks = sorted(m - g0 for m in self.step_marks if g0 <= m < g0 + n_total)
    # (looked up per group: a step mark may install / change the engine's time plan)
    plan = lambda i: eng.time_plan is not None and eng.time_plan(i) is not None
    pos, stopped = 0, False
    for m in marks + [None]:
      target = n_full if m is None else min(m, n_full)
      if target > pos:
        gs.run(target - pos, plan)
        self._global_step += target - pos
        pos = target
      if m is None or m > n_full:
        break                            # (a mark behind the ragged step is handled below)
      gs.cut()                           # nothing of the steps after the mark may be in flight
      if self.step_marks[g0 + m]():
        self._stop_training = stopped = True
        break
    losses = gs.losses(pos)
    if not stopped and n % B:
      # the ragged last batch: eager, host-provided arguments (its own block)
      users = torch.from_numpy(order[n_full * B:]).to(self.device)
      dp = getattr(self, "_dp", None)
      out = torch.zeros(1, dtype=torch.float32, device=self.device)
      if dp is not None:
        dp.collate(gs.tail_blk, dcsr, users)
        eng.train_step(gs.tail_blk, 0, int(users.numel()), out=out,
                       global_rows=int(users.numel()) * dp.world)
      else:
        gs.tail_blk.collate(dcsr, users)
        eng.train_step(gs.tail_blk, 0, int(users.numel()), out=out)
      self._global_step += 1
      losses = torch.cat([losses, out])
    if draw_next_order and not self._stop_training:
      n_draw = n if n_draw is None else n_draw
      self._order_ahead = (n_draw, epoch_user_order(n_draw))      # (everything of this epoch is enqueued)
    return losses.cpu().numpy().copy()

  def _validate(self, val_dataloader):
    """model.py:439-452: mean over batches of the eval-mode loss; input and
    target are collated independently (different item sets)."""
    self.model.eval()
    engine = self._engine()
    ds = val_dataloader.dataset
    dcsr = ds.device_csr()
    dcsr_t = ds.device_target_csr()
    B, S = val_dataloader.batch_size, val_dataloader.num_sampling_users
    ns = val_dataloader.negative_sampling
    blk = self._make_block(dcsr, S, ns)
    blk_t = self._make_block(dcsr_t, S, ns) if dcsr_t is not None else None
    n = len(ds)
    order = None
    if self.user_order_hook is not None:
      order = self.user_order_hook(-1, n)
    if order is None:
      order = epoch_user_order(n)
    order_dev = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int64)).to(self.device)
    nb = int(np.ceil(n / B)) if n else 1
    buf = torch.zeros(max(1, nb), dtype=torch.float32, device=self.device)
    k = 0
    for off in range(0, n, S):
      users = order_dev[off:off + S]
      blk.collate(dcsr, users)
      if blk_t is not None:
        blk_t.collate(dcsr_t, users)
      Sg = int(users.numel())
      for r in range(0, Sg, B):
        rows = min(B, Sg - r)
        engine.compute_loss(blk, r, rows, tgt=blk_t, out=buf[k:k + 1])
        k += 1
    total = float(buf[:k].double().sum().item()) if k else 0.0
    return total / max(1, k)

  # -------------------------------------------------------------- inference
  def predict(self, users_interactions, return_input=False):
    """model.py:487-511.  Returns ``(output, input_dense)`` -- like the
    reference, always a tuple (its ``return output, input if .. else output``
    precedence quirk); when return_input is False the second element is the
    output again."""
    if self.model is None:
      raise Exception("Model not initialized.")
    self.model.eval()
    self._check_ranges()
    out, blk, B = self._predict_scores(users_interactions)
    if return_input:
      m = users_interactions.interactions_matrix
      dense = torch.from_numpy(np.asarray(m.todense(), dtype=np.float32)).to(self.device)
      return out, dense
    return out, out

  def _input_block(self, users_interactions, ws=None, lookup_users=True):
    """The users' interactions as an unsampled device block (bitmap over the whole catalogue),
    in buffers that are kept and reused across predict / recommend calls (``ws``: in that
    workspace instead, ``recoder_amd.validation`` keeps one per batch)."""
    m = users_interactions.interactions_matrix
    B = m.shape[0]
    n_items = self.num_items if self.num_items is not None else m.shape[1]
    dcsr = DeviceCSR(m, self.device)
    assert dcsr.n_items <= n_items
    if dcsr.n_items != n_items:
      dcsr.shape = (B, n_items)
    if ws is None:
      ws = getattr(self, "_eval_ws", None)
      if ws is None or ws["n_items"] != n_items:
        ws = self._eval_ws = self._new_eval_ws(n_items)
    ws["dcsr"] = dcsr
    blk = ws["blk"]
    if blk is None or blk.S_cap < B or blk.nnz_cap < max(1, dcsr.nnz):
      blk = ws["blk"] = Block(max(B, blk.S_cap if blk else 0),
                              max(1, dcsr.nnz, blk.nnz_cap if blk else 0), n_items, self.device,
                              negative_sampling=False, need_bits_cr=False)
    rows = torch.arange(B, dtype=torch.int64, device=self.device)
    blk.collate(dcsr, rows, negative_sampling=False)
    # MF looks user rows up by their global ids (not with ``recommend_folded``'s rows, whose users have none)
    if lookup_users:
      blk.users = torch.as_tensor(np.asarray(users_interactions.users), dtype=torch.int64) \
          .to(self.device)
    return blk, B, n_items

  @staticmethod
  def _new_eval_ws(n_items):
    return dict(n_items=n_items, blk=None, strips={}, scores=None, cand=None)

  def _predict_scores(self, users_interactions):
    engine = self._engine()
    blk, B, n_items = self._input_block(users_interactions)
    ld = blk.ld_cap
    out = torch.empty(B, ld, dtype=torch.float32, device=self.device)
    if self._scores_from_csr_rows():
      self.model.csr_scores(self._eval_ws["dcsr"], 0, n_items, out, ld, B)
      return out[:, :n_items], blk, B
    if self._scores_from_user_ids():
      self.model.user_scores(self._user_ids(users_interactions), 0, n_items, out, ld)
      return out[:, :n_items], blk, B
    engine.predict_scores(blk, 0, B, out, ld, blk)
    return out[:, :n_items], blk, B

  def _evaluate(self, eval_dataset, num_recommendations, metrics, batch_size=1, num_users=None, on_device=False):
    """model.py:513-523."""
    if self.model is None:
      raise Exception("Model not initialized")
    self.model.eval()
    recommender = InferenceRecommender(self, num_recommendations)
    evaluator = RecommenderEvaluator(recommender, metrics)
    if on_device:
      return evaluator.evaluate(eval_dataset, batch_size=batch_size, num_users=num_users, on_device=True)
    return evaluator.evaluate(eval_dataset, batch_size=batch_size, num_users=num_users)

  # items decoded at a time by recommend(): [B, strip] fp32 scores stay cache-resident
  # (B = 500: 128 MB) instead of a [B, n_items] matrix in HBM (2 GB at C5's 1 M items)
  eval_strip_items = 65536

  def recommend(self, users_interactions, num_recommendations):
    """model.py:525-544: scores with the seen (positive) items at -inf, top-k sorted; a list of
    lists like the reference's (``recommend_array``: the same as one [users, k] int64 array)."""
    return self.recommend_array(users_interactions, num_recommendations).tolist()

  def recommend_array(self, users_interactions, num_recommendations):
    """recommend() as a numpy array (what the evaluator consumes: 50 k Python ints per batch of
    500 users cost more than scoring them).

    The fused engines never materialise the [B, n_items] score matrix: the catalogue is decoded
    in strips of ``eval_strip_items`` items, each strip's masked top k is kept
    (``rk_topk_masked`` with a column offset) and the per-strip winners are merged with one more top-k pass --
    ties resolve to the lower item id at both levels, as torch.topk on the full row would."""
    ids, _ = self._recommend_device(users_interactions, num_recommendations, host_ok=True)
    if isinstance(ids, np.ndarray):                                 # (the fused form: already on the host)
      return ids
    return ids.cpu().numpy().copy()

  def _recommend_device(self, users_interactions, num_recommendations, host_ok=False, ws=None, inputs=None,
                        user_rows=None, seen=None, with_scores=False):
    """``recommend_array`` before its copy to the host: (ids, ld), an int64 device tensor [users, k] (possibly a
    strided view of the candidate buffer, valid until the next call on the same workspace) and its row stride.
    The fused form of ``engine.recommend_fused`` reads its ids back with its status word, so it is taken only
    with ``host_ok`` and then returns (the numpy array, k); without it the catalogue is decoded strip by strip.
    ``ws`` is the workspace of the scores and candidates (None: the Recoder's own ``_eval_ws``), ``inputs`` an
    earlier ``(blk, B, n_items, dcsr)`` of ``_input_block`` for these users (None: collated now).  ``user_rows``
    (``recommend_folded``): a [users, h] f32 device tensor scored in place of the encoder's output, strip by strip;
    ``users_interactions.users`` is then not read.  ``seen`` (``recommend_filtered``): a block whose ``bits_rc`` is
    a deny bitmap with ``implicit`` set, masked in place of the users' own input block, strip by strip; with
    ``with_scores`` the result is (ids, ld, scores), the f32 values the ranking ranked laid out like the ids."""
    self.model.eval()
    self._check_ranges()
    k = int(num_recommendations)
    from . import _lib
    from .device import current_stream
    lib = _lib.load()
    engine = self._engine()
    ids_model = self._scores_from_user_ids()
    csr_model = self._scores_from_csr_rows() or ids_model        # (either way: no encoder, a scores kernel of its own)
    if (getattr(engine, "generic", False) and not csr_model) or k > lib.rk_topk_max_k():
      assert seen is None and not with_scores                     # (serve.check_serving refused it)
      if user_rows is not None:
        raise ValueError("recommend_folded scores on the fused HIP engine (optimizer_type='adam', an embedding size "
                         "that is a multiple of 4) and takes at most %d recommendations (got %d)"
                         % (lib.rk_topk_max_k(), k))
      return self._recommend_dense_device(users_interactions, k), k
    if inputs is None:
      blk, B, n_items = self._input_block(users_interactions, ws, lookup_users=user_rows is None)
      if ws is None:
        ws = self._eval_ws
      dcsr = ws["dcsr"]
    else:
      blk, B, n_items, dcsr = inputs
      assert ws is not None and ws["n_items"] == n_items
    if user_rows is not None:
      assert not csr_model and tuple(user_rows.shape) == (B, engine.h[0]) and user_rows.dtype == torch.float32
      engine.ensure_capacity(B, blk.n_cap)
      z = user_rows.contiguous()
      host_ok = False                                             # (the fused form encodes the block's users itself)
    else:
      z = None if csr_model else engine.encode_eval(blk, 0, B)
    if seen is not None or with_scores:
      host_ok = False                                             # (the strips: their mask is an argument, they keep scores)
    seen_ref = blk.ref if seen is None else seen.ref
    strip = max(k, min(n_items, int(self.eval_strip_items)))
    bounds = [(lo, min(n_items, lo + strip)) for lo in range(0, n_items, strip)]
    if len(bounds) > 1 and bounds[-1][1] - bounds[-1][0] < k:      # a last strip shorter than k:
      lo0 = bounds[-2][0]                                         # merge it into the one before
      bounds = bounds[:-2] + [(lo0, n_items)]
    ns = len(bounds)
    if host_ok and ns > 1 and not csr_model and os.environ.get("RK_EVAL_FUSED", "1") != "0" and \
        hasattr(engine, "recommend_fused"):
      # catalogues of more than one strip: the top-k filter rides in the decode's epilogue (no score
      # matrix, no passes over it): a strided sample of the catalogue bounds every row's k-th best
      # score from below, the decode over all items keeps only what reaches the bound
      # (engine.recommend_fused / include/recoder_hip.h "The fused form") -- the same ids, ties included
      res = engine.recommend_fused(blk, B, k, n_items)
      if res is not None:
        out, status = res
        host = torch.cat([out.reshape(-1), status.to(torch.int64)]).cpu().numpy()
        if host[-1] == 0:
          self.eval_fused_batches = getattr(self, "eval_fused_batches", 0) + 1
          return host[:-1].reshape(B, k).copy(), k
        # (a candidate list overflowed, or a row has fewer than k unseen items: strip by strip)
    width = max(hi - lo for lo, hi in bounds)
    ld = -(-width // 32) * 32
    if ws["scores"] is None or ws["scores"].numel() < B * ld:
      ws["scores"] = torch.empty(B * ld, dtype=torch.float32, device=self.device)
    if ws["cand"] is None or ws["cand"][0].shape[0] < B or ws["cand"][0].shape[1] != ns * k:
      ws["cand"] = (torch.empty(B, ns * k, dtype=torch.int64, device=self.device),
                    torch.empty(B, ns * k, dtype=torch.float32, device=self.device))
    cand_idx, cand_val = ws["cand"][0][:B], ws["cand"][1][:B]
    scores = ws["scores"]
    user_ids = self._user_ids(users_interactions) if ids_model else None
    for s, (lo, hi) in enumerate(bounds):
      if csr_model:
        if ids_model:
          # scored from user ids: the strip of the model's own kernel (rk_als_ncf_scores)
          self.model.user_scores(user_ids, lo, hi, scores, ld)
        else:
          # an item-item model's strip of scores: the users' CSR rows times W[:, lo:hi]
          self.model.csr_scores(dcsr, lo, hi, scores, ld, B)
        _lib.check(lib.rk_topk_masked(scores.data_ptr(), B, hi - lo, ld, seen_ref, 0, k, lo, 1,
                                      cand_idx[:, s * k:].data_ptr(), cand_val[:, s * k:].data_ptr(),
                                      ns * k, current_stream()), "rk_topk_masked")
        continue
      key = (lo, hi, B)
      sblk = ws["strips"].get(key)
      if sblk is None:
        sblk = Block(B, 1, n_items, self.device, negative_sampling=True, need_bits_cr=False,
                     n_cap=hi - lo)
        sblk.set_items(torch.arange(lo, hi, dtype=torch.int32, device=self.device), hi - lo, B)
        if len(ws["strips"]) > 64:
          ws["strips"].clear()
        ws["strips"][key] = sblk
      engine.decode_scores(z, B, sblk, scores, ld)
      _lib.check(lib.rk_topk_masked(scores.data_ptr(), B, hi - lo, ld, seen_ref, 0, k, lo, 1,
                                          cand_idx[:, s * k:].data_ptr(), cand_val[:, s * k:].data_ptr(),
                                          ns * k, current_stream()), "rk_topk_masked")
    if ns == 1:
      return (cand_idx[:, :k], ns * k, cand_val[:, :k]) if with_scores else (cand_idx[:, :k], ns * k)
    # merge: top k of the ns * k candidates (positions), then their item ids.  Candidates are laid
    # out strip by strip, each sorted by (score desc, id asc): equal scores keep ascending ids
    pos = torch.empty(B, k, dtype=torch.int64, device=self.device)
    val = torch.empty(B, k, dtype=torch.float32, device=self.device) if with_scores else None
    _lib.check(lib.rk_topk_masked(cand_val.data_ptr(), B, ns * k, ns * k, None, 0, k, 0, 1, pos.data_ptr(),
                                  None if val is None else val.data_ptr(), k, current_stream()), "rk_topk_masked")
    ids = torch.gather(cand_idx, 1, pos)
    return (ids, k, val) if with_scores else (ids, k)

  def _recommend_dense(self, users_interactions, k):
    """Full score matrix + torch.topk: the generic (torch-autograd) engine and k above the
    top-k kernel's limit."""
    return self._recommend_dense_device(users_interactions, k).cpu().numpy()

  def _recommend_dense_device(self, users_interactions, k):
    out, dense = self.predict(users_interactions, return_input=True)
    out = out.clone()
    out[dense > 0] = -float("inf")
    return torch.topk(out, k, dim=1, sorted=True)[1]

  def evaluate(self, eval_dataset, num_recommendations, metrics, batch_size=1, num_users=None, on_device=False):
    """model.py:546-559.  ``on_device=True``: the top-k lists stay on the device and the three built-in metrics are
    computed there (``metrics.RecommenderEvaluator.evaluate``); the same values, user-defined metrics fall back."""
    results = self._evaluate(eval_dataset, num_recommendations, metrics, batch_size=batch_size,
                             num_users=num_users, on_device=on_device)
    for metric in results:
      log.info("{}: {}".format(metric, np.mean(results[metric])))
    return results
