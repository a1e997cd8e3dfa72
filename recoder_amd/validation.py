"""Validation during a fit, and early stopping, for the iterative trainers of ``MatrixFactorization``
(``Recoder.train_bpr``, ``train_warp``, ``train_lightgcn``, ``train_simgcl``, ``train_directau``, ``train_ssm``,
``train_ultragcn``).

``Validator`` scores a validation set with the Recoder's own recommend path and leaves the top-k lists on the device,
where rk_als_rank_metrics (include/recoder_als.h) turns them into one metric: a call of ``score()`` costs one small
read-back.  ``EarlyStopping`` is the stopping rule as host logic; ``Monitor`` is what a fit's epoch loop talks to: it
decides which epochs are due, scores, keeps a device copy of the best epoch and puts it back at the end.

The trainers' workspaces, their sampler (a counter hash of seed, step and slot) and torch's global RNG are not
touched: a fit with a validation set and ``patience=None, restore_best=False`` leaves the bits of one without.
"""
import collections

import numpy as np
import torch

from . import metrics as metrics_mod
from .data import UsersInteractions

Config = collections.namedtuple("Config", "dataset metric eval_freq batch_size num_users patience restore_best")

DEFAULTS = dict(eval_metric=None, eval_freq=1, eval_batch_size=500, eval_num_users=None, patience=None)


def _int(name, v, lo, optional=False):
  if v is None and optional:
    return None
  if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
    raise ValueError("%s must be an integer >= %d%s (got %r)" % (name, lo, " or None" if optional else "", v))
  return int(v)


def check_metric(metric, max_k=None):
  """ValueError unless ``metric`` is one Recall / NDCG / AveragePrecision whose k the top-k kernel can take
  (``max_k`` None: rk_topk_max_k(), read from the library; no GPU is touched)."""
  if not metrics_mod.device_metrics_ok([metric]):
    raise ValueError("eval_metric must be a Recall, NDCG or AveragePrecision with an integer k >= 1 (got %r)"
                     % (metric,))
  if max_k is None:
    from . import _lib
    max_k = _lib.load().rk_topk_max_k()
  if metric.k > max_k:
    raise ValueError("eval_metric's k = %d is above the top-k kernel's limit rk_topk_max_k() = %d" % (metric.k, max_k))
  return metric


def check_config(method, val_dataset, eval_metric=None, eval_freq=1, eval_batch_size=500, eval_num_users=None,
                 patience=None, restore_best=True, num_items=None, max_k=None):
  """The validation arguments of ``method`` (a trainer's name, for the messages), checked before any GPU work.
  Returns None without a ``val_dataset`` -- every other argument must then be at its default -- else a ``Config``
  with ``eval_metric`` None replaced by Recall(20).  ``num_items`` is the catalogue's size when it is known."""
  eval_freq = _int("eval_freq", eval_freq, 1)
  patience = _int("patience", patience, 1, optional=True)
  eval_batch_size = _int("eval_batch_size", eval_batch_size, 1)
  eval_num_users = _int("eval_num_users", eval_num_users, 1, optional=True)
  if val_dataset is None:
    given = dict(eval_metric=eval_metric, eval_freq=eval_freq, eval_batch_size=eval_batch_size,
                 eval_num_users=eval_num_users, patience=patience)
    extra = sorted(k for k, v in given.items() if v != DEFAULTS[k])
    if extra:
      raise ValueError("%s: %s need%s a val_dataset" % (method, ", ".join(extra), "s" if len(extra) == 1 else ""))
    return None
  metric = check_metric(metrics_mod.Recall(20) if eval_metric is None else eval_metric, max_k)
  if getattr(val_dataset, "interactions_matrix", None) is None or \
      getattr(val_dataset, "target_interactions_matrix", None) is None:
    raise ValueError("%s: val_dataset needs an interactions_matrix and a target_interactions_matrix" % method)
  widths = (val_dataset.interactions_matrix.shape[1], val_dataset.target_interactions_matrix.shape[1])
  if num_items is not None and max(widths) > num_items:
    raise ValueError("%s: the validation matrices have %d columns, the catalogue %d items"
                     % (method, max(widths), num_items))
  if val_dataset.interactions_matrix.shape[0] != val_dataset.target_interactions_matrix.shape[0]:
    raise ValueError("%s: val_dataset's input and target matrices differ in their rows" % method)
  return Config(val_dataset, metric, eval_freq, eval_batch_size, eval_num_users, patience, bool(restore_best))


SETTINGS = ("val_dataset", "eval_metric", "eval_freq", "eval_batch_size", "eval_num_users", "patience", "restore_best")


def check_settings(settings):
  """``Recoder.fit_validation`` as keywords of ``check_config``: a dict of SETTINGS' names with a ``val_dataset``."""
  if not isinstance(settings, dict) or set(settings) - set(SETTINGS) or settings.get("val_dataset") is None:
    raise ValueError("fit_validation must be None or a dict with a val_dataset and any of %s (got %r)"
                     % (", ".join(SETTINGS[1:]), settings))
  return dict(settings)


class EarlyStopping(object):
  """The stopping rule: ``update(epochs, value)`` after each evaluation, ``epochs`` the epochs fitted so far.  A
  new best is strictly greater than every value before it (a tie keeps the earlier epoch); nan is never one.
  ``patience = p`` stops after p evaluations in a row without a new best (None: never)."""

  def __init__(self, patience=None):
    self.patience = patience
    self.best_value, self.best_epoch, self.stopped_epoch, self.stale = None, None, None, 0
    self.values, self.epochs = [], []

  def update(self, epochs, value):
    """Returns (whether this evaluation is the new best, whether the fit stops here)."""
    value = float(value)
    self.values.append(value), self.epochs.append(int(epochs))
    best = value == value and (self.best_value is None or value > self.best_value)
    if best:
      self.best_value, self.best_epoch, self.stale = value, int(epochs), 0
    else:
      self.stale += 1
    stop = self.patience is not None and self.stale >= self.patience
    if stop:
      self.stopped_epoch = int(epochs)
    return best, stop


class Validator(object):
  """One metric of ``recoder`` on ``val_dataset`` (inputs ``interactions_matrix``, targets
  ``target_interactions_matrix``), everything on the device.  The users are taken in ascending order in batches of
  ``batch_size``, the first ``num_users`` of them (None: all); their input blocks and target CSRs are uploaded here,
  once.  ``num_recommendations`` None takes the metric's k.  The scores, candidates and metric buffers are this
  object's own."""

  def __init__(self, recoder, val_dataset, metric, num_recommendations=None, batch_size=500, num_users=None):
    check_metric(metric)
    self.recoder, self.metric = recoder, metric
    self.k = int(metric.k if num_recommendations is None else num_recommendations)
    n_items = recoder.num_items
    inp_m, tgt_m = val_dataset.interactions_matrix.tocsr(), val_dataset.target_interactions_matrix.tocsr()
    if n_items is None or recoder.model is None:
      raise ValueError("Validator needs an initialised Recoder (its catalogue's size is not known yet)")
    if max(inp_m.shape[1], tgt_m.shape[1]) > n_items:
      raise ValueError("the validation matrices have %d columns, the catalogue %d items"
                       % (max(inp_m.shape[1], tgt_m.shape[1]), n_items))
    n = inp_m.shape[0] if num_users is None else min(int(num_users), inp_m.shape[0])
    users = np.asarray(val_dataset.users)
    dev = recoder.device
    self.ws = recoder._new_eval_ws(n_items)
    self.tables = metrics_mod.DeviceMetricTables([metric], dev)
    self.batches = []
    for lo in range(0, n, int(batch_size)):
      rows = np.arange(lo, min(n, lo + int(batch_size)))
      inp = UsersInteractions(users=users[rows], interactions_matrix=inp_m[rows])
      ws_b = recoder._new_eval_ws(n_items)
      blk, B, _ = recoder._input_block(inp, ws_b)
      self.batches.append((inp, (blk, B, n_items, ws_b["dcsr"]), metrics_mod.DeviceTarget(tgt_m[rows], dev)))
    nb = len(self.batches)
    cap = max([b[1][1] for b in self.batches] + [1])
    self.values = torch.empty((cap, 1), dtype=torch.float64, device=dev)
    self.sums = torch.zeros(max(nb, 1), dtype=torch.float64, device=dev)
    self.counts = torch.zeros(max(nb, 1), dtype=torch.int64, device=dev)

  def score(self):
    """The mean of the metric over the users that have a target (nan when none has): per batch the kernel's fixed-order
    sum and count, added here in batch order.  One host synchronisation."""
    rec = self.recoder
    rec._weights_written()            # (the trainers write the tables through .data)
    for b, (inp, inputs, target) in enumerate(self.batches):
      ids, ld = rec._recommend_device(inp, self.k, ws=self.ws, inputs=inputs)
      metrics_mod.device_batch_metrics(ids, ld, target, [self.metric], self.tables,
                                       out=(self.values, self.sums[b:b + 1], self.counts[b:b + 1]))
    host = torch.cat([self.sums, self.counts.double()]).cpu().numpy()        # (the synchronisation)
    nb = len(self.sums)
    total, count = 0.0, 0
    for b in range(len(self.batches)):
      total, count = total + float(host[b]), count + int(host[nb + b])
    return total / count if count else float("nan")


class Monitor(object):
  """What an epoch loop calls: ``due(e)`` after epoch e (from 0), then -- once the model's tables are what a fit
  ending there would leave -- ``epoch_end(e, tensors, step)``, which scores, keeps the best epoch's ``tensors`` and
  says whether to stop; ``finish(tensors, epochs_run)`` after the loop puts the best copy back."""

  def __init__(self, validator, config):
    self.validator, self.config = validator, config
    self.rule = EarlyStopping(config.patience)
    self.restore_best = config.restore_best
    self._best, self._best_step = None, None

  def due(self, e):
    return (e + 1) % self.config.eval_freq == 0

  def epoch_end(self, e, tensors, step=None, prepare=None):
    """``tensors``: what to copy when this epoch is the best so far; ``prepare`` = (tables, function): the tables are
    copied, changed in place by the function for the scoring alone, and put back bit for bit."""
    if prepare is not None:
      tables, change = prepare
      keep = [t.clone() for t in tables]
      for t in tables:
        change(t)
    value = self.validator.score()
    if prepare is not None:
      for t, k in zip(tables, keep):
        t.copy_(k)
    best, stop = self.rule.update(e + 1, value)
    if best and self.restore_best:
      if self._best is None:
        self._best = [t.clone() for t in tensors]
      else:
        for dst, src in zip(self._best, tensors):
          dst.copy_(src)
      self._best_step = step
    return stop

  def finish(self, tensors, epochs_run):
    """True when the best epoch's copy was put back into ``tensors`` (its step count is then ``best_step``): with
    ``restore_best``, a best epoch, and ``epochs_run`` epochs fitted past it."""
    if not self.restore_best or self._best is None or self.rule.best_epoch == epochs_run:
      return False
    for dst, src in zip(tensors, self._best):
      dst.copy_(src)
    return True

  @property
  def best_step(self):
    return self._best_step

  def result(self):
    m, r = self.config.metric, self.rule
    return {"metric": str(m), "k": int(m.k), "values": list(r.values), "epochs": list(r.epochs),
            "best_epoch": r.best_epoch, "stopped_epoch": r.stopped_epoch}
