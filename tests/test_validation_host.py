"""CPU: the validation settings of the seven iterative trainers (keywords; Recoder.fit_validation for the two whose
parameter lists are pinned) are refused with a ValueError before any GPU work, and
the early-stopping rule of recoder_amd/validation.py gives the documented best_epoch / stopped_epoch."""
import numpy as np
import pytest
import scipy.sparse as sp

TRAINERS = ("train_bpr", "train_warp", "train_lightgcn", "train_simgcl", "train_directau", "train_ssm",
            "train_ultragcn")
# (their parameter lists are pinned by tests/test_ssm_host.py and tests/test_ultragcn_host.py: the settings come from
# Recoder.fit_validation)
BY_ATTRIBUTE = ("train_ssm", "train_ultragcn")


def _rec():
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(16, activation_type="none"), loss="mse", loss_params={},
                 optimizer_type="adam")


def _dataset(n_items=5, target=False):
  from recoder_amd.data import RecommendationDataset
  m = sp.csr_matrix(np.eye(5, n_items, dtype=np.float32))
  return RecommendationDataset(m, m.copy() if target else None)


def _cases():
  from recoder_amd.metrics import Metric, Recall
  from recoder_amd import _lib
  kmax = _lib.load().rk_topk_max_k()
  val = _dataset(target=True)
  return {
      "eval_freq_zero": dict(val_dataset=val, eval_freq=0),
      "eval_freq_float": dict(val_dataset=val, eval_freq=1.5),
      "patience_zero": dict(val_dataset=val, patience=0),
      "patience_without_val": dict(patience=2),
      "eval_freq_without_val": dict(eval_freq=2),
      "eval_metric_without_val": dict(eval_metric=Recall(5)),
      "eval_batch_size_without_val": dict(eval_batch_size=100),
      "eval_num_users_without_val": dict(eval_num_users=10),
      "user_metric": dict(val_dataset=val, eval_metric=Metric("mine")),
      "k_above_topk": dict(val_dataset=val, eval_metric=Recall(kmax + 1)),
      "wider_than_catalogue": dict(val_dataset=_dataset(n_items=9, target=True)),
      "no_target": dict(val_dataset=_dataset()),
  }


@pytest.mark.parametrize("trainer", TRAINERS)
@pytest.mark.parametrize("case", [
    "eval_freq_zero", "eval_freq_float", "patience_zero", "patience_without_val", "eval_freq_without_val",
    "eval_metric_without_val", "eval_batch_size_without_val", "eval_num_users_without_val", "user_metric",
    "k_above_topk", "wider_than_catalogue", "no_target"])
def test_validation_arguments_rejected_before_gpu_work(trainer, case, monkeypatch):
  # (every module imported before patching: one imported inside the patch would keep the stand-in)
  import recoder_amd.model as model_mod
  import recoder_amd.validation  # noqa: F401
  from recoder_amd import device

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  rec = _rec()
  with pytest.raises(ValueError):
    if trainer in BY_ATTRIBUTE:
      rec.fit_validation = _cases()[case]
      getattr(rec, trainer)(_dataset(), num_epochs=1)
    else:
      getattr(rec, trainer)(_dataset(), num_epochs=1, **_cases()[case])


@pytest.mark.parametrize("settings", [{"val_dataset": None}, {"patience": 2}, {"val_dataset": 1, "epochs": 3}, [1]])
def test_fit_validation_must_be_a_dict_of_the_keywords_with_a_val_dataset(settings, monkeypatch):
  import recoder_amd.model as model_mod
  monkeypatch.setattr(model_mod, "require_gpu", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU work")))
  for trainer in TRAINERS:
    rec = _rec()
    rec.fit_validation = settings
    with pytest.raises(ValueError, match="fit_validation"):
      getattr(rec, trainer)(_dataset(), num_epochs=1)


def test_check_config_defaults():
  from recoder_amd import validation
  from recoder_amd.metrics import NDCG
  assert validation.check_config("train_bpr", None) is None
  cfg = validation.check_config("train_bpr", _dataset(target=True), max_k=100)
  assert str(cfg.metric) == "Recall@20" and cfg.eval_freq == 1 and cfg.batch_size == 500 and cfg.num_users is None
  assert cfg.patience is None and cfg.restore_best is True
  cfg = validation.check_config("train_bpr", _dataset(target=True), NDCG(10), 2, 64, 3, 4, False, num_items=5,
                                max_k=100)
  assert (str(cfg.metric), cfg.eval_freq, cfg.batch_size, cfg.num_users, cfg.patience, cfg.restore_best) == \
      ("NDCG@10", 2, 64, 3, 4, False)


def _run(patience, values):
  from recoder_amd.validation import EarlyStopping
  rule = EarlyStopping(patience)
  flags = []
  for e, v in enumerate(values):
    best, stop = rule.update(e + 1, v)
    flags.append(best)
    if stop:
      break
  return rule, flags


def test_early_stopping_rule():
  nan = float("nan")
  # a tie is no new best: the earlier epoch stays, and the tie counts against the patience
  rule, flags = _run(2, [0.1, 0.2, 0.2, 0.15, 0.9])
  assert (rule.best_epoch, rule.stopped_epoch, flags) == (2, 4, [True, True, False, False])
  assert rule.values == [0.1, 0.2, 0.2, 0.15] and rule.epochs == [1, 2, 3, 4]
  # nan is never a best, not even the first value; it counts against the patience
  rule, flags = _run(2, [nan, 0.3, nan, 0.31, 0.1, 0.2])
  assert (rule.best_epoch, rule.stopped_epoch, flags) == (4, 6, [False, True, False, True, False, False])
  rule, _ = _run(2, [nan, nan, 0.5])
  assert (rule.best_epoch, rule.best_value, rule.stopped_epoch) == (None, None, 2)
  # a late improvement inside the patience resets the count
  rule, flags = _run(3, [0.5, 0.4, 0.4, 0.6, 0.1, 0.1, 0.1, 0.7])
  assert (rule.best_epoch, rule.stopped_epoch) == (4, 7)
  # ... and one after it comes too late with patience 1
  rule, _ = _run(1, [0.5, 0.4, 0.9])
  assert (rule.best_epoch, rule.stopped_epoch) == (1, 2)
  # no patience: never stops, the best is still tracked
  rule, _ = _run(None, [0.5, 0.4, 0.9, 0.9])
  assert (rule.best_epoch, rule.stopped_epoch, len(rule.values)) == (3, None, 4)


def test_monitor_due_epochs():
  from recoder_amd import validation
  cfg = validation.check_config("train_bpr", _dataset(target=True), eval_freq=3, max_k=100)
  mon = validation.Monitor(None, cfg)
  assert [e for e in range(7) if mon.due(e)] == [2, 5]


def test_snapshot_bytes_enter_the_memory_checks():
  from recoder_amd import bpr, lightgcn, warp
  u, n, h, nnz, T = 1000, 300, 32, 5000, 256
  tables = (u + n) * h * 4
  assert bpr.required_bytes(u, n, h, nnz, T, snapshot=True) - bpr.required_bytes(u, n, h, nnz, T) == tables + n * 4
  assert warp.required_bytes(u, n, h, nnz, T, snapshot=True) - warp.required_bytes(u, n, h, nnz, T) == tables + n * 4
  assert lightgcn.method_required_bytes(lightgcn.METHOD, u, n, h, nnz, T, snapshot=True) - \
      lightgcn.method_required_bytes(lightgcn.METHOD, u, n, h, nnz, T) == 3 * tables
  with pytest.raises(ValueError, match="are free"):
    need = bpr.required_bytes(u, n, h, nnz, T, False)
    bpr.check_memory(u, n, h, nnz, T, free_bytes=need, allocate_model=False, snapshot=True)
