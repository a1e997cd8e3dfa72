"""GPU: Recoder.evaluate(on_device=True) beside the host path, and validation / early stopping inside the seven
iterative trainers (recoder_amd/validation.py).

Everything here is exact unless said otherwise: the trainers are bit-reproducible for a fixed seed, the metric
kernel has fixed summation orders, and a validation score is the kernel's fixed-order sum over the users in ascending
order divided by their count -- restated from the per-user values by ``_mean`` below."""
import numpy as np
import pytest
import torch

from recoder_amd.data import RecommendationDataset, epoch_user_order
from recoder_amd.metrics import NDCG, AveragePrecision, Recall

from . import bpr_util
from . import rank_metrics_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
METRIC = Recall(20)


def _recoder(h=16):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


@pytest.fixture(scope="module")
def data():
  tr, ho = bpr_util.planted()                            # 200 users x 120 items, a fifth of every row held out
  return tr, ho, RecommendationDataset(tr), RecommendationDataset(tr, ho), bpr_util.init_tables(200, 120, 16, 0)


def _start(rec, trainer, train_ds, start, **kw):
  """The model built by an empty fit, its tables set to ``start``."""
  getattr(rec, trainer)(train_ds, num_epochs=0, **kw)
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias), start):
    p.data.copy_(torch.as_tensor(a, device=DEV))
  return rec


def _tables(rec):
  m = rec.model
  return tuple(p.detach().cpu().numpy().copy() for p in
               (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


def _same(a, b):
  return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _state(rec, prefix):
  st = getattr(rec, prefix + "_state")
  return tuple(t.cpu().numpy().copy() for k in ("E0", "M", "V") for t in st[k]) + (np.array([st["step"]]),)


def _per_user(rec, val_ds, metrics, seed=5, **kw):
  """evaluate()'s per-user values put back into user order (the evaluator walks a random order drawn from torch's
  global generator)."""
  torch.manual_seed(seed)
  res = rec.evaluate(val_ds, 20, metrics, batch_size=500, **kw)
  torch.manual_seed(seed)
  order = epoch_user_order(len(val_ds))
  out = np.empty((len(val_ds), len(metrics)))
  for j, m in enumerate(metrics):
    out[order, j] = res[m]
  return out


def _mean(values):
  sums, count = U.fixed_order_sums(values.reshape(len(values), -1)[:, :1])
  return sums[0] / count


def _score(rec, val_ds):
  return _mean(_per_user(rec, val_ds, [METRIC], on_device=True))


# ------------------------------------------------------------------ evaluate
def test_evaluate_on_device_equals_the_host_path(data):
  _, _, train_ds, val_ds, start = data
  rec = _start(_recoder(), "train_bpr", train_ds, start)
  rec.train_bpr(train_ds, num_epochs=2, batch_size=256, seed=0)
  metrics = [Recall(20), Recall(5, normalize=False), NDCG(20), AveragePrecision(20), AveragePrecision(7, normalize=False)]
  host, dev = _per_user(rec, val_ds, metrics), _per_user(rec, val_ds, metrics, on_device=True)
  assert np.array_equal(np.isnan(host), np.isnan(dev)) and not np.isnan(host).all()
  ok = ~np.isnan(host[:, 0])
  assert np.array_equal(host[ok, :2], dev[ok, :2])                                # Recall: one integer division
  assert (np.abs(host[ok] - dev[ok]) <= 2 * 20 * 2.0 ** -53 * np.maximum(host[ok], dev[ok])).all()

  class Mine(Recall):                                    # a user-defined metric: the host path, the same values
    pass
  mine = Mine(20)
  assert np.array_equal(_per_user(rec, val_ds, [mine], on_device=True)[ok], host[ok, :1])


def test_evaluate_on_device_over_several_strips():
  import scipy.sparse as sp
  n_users, n_items = 40, 200000
  rng = np.random.RandomState(3)

  def rand(per_row):
    rows = np.repeat(np.arange(n_users), per_row)
    m = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, rng.randint(0, n_items, size=len(rows)))),
                      shape=(n_users, n_items))
    m.data[:] = 1.0
    return m
  tr, ho = rand(30), rand(10)
  ho = (ho - ho.multiply(tr)).tocsr()
  ho = sp.vstack([sp.csr_matrix((1, n_items), dtype=np.float32), ho[1:]]).tocsr()   # user 0 without targets: nan
  ho.eliminate_zeros()
  rec = _recoder()
  rec.train_bpr(RecommendationDataset(tr), num_epochs=2, batch_size=256, seed=0)
  val_ds = RecommendationDataset(tr, ho)
  assert n_items > 3 * rec.eval_strip_items
  metrics = [Recall(20), NDCG(20)]
  host, dev = _per_user(rec, val_ds, metrics), _per_user(rec, val_ds, metrics, on_device=True)
  assert np.array_equal(np.isnan(host), np.isnan(dev)) and np.isnan(dev[0]).all() and not np.isnan(dev[1:]).any()
  ok = ~np.isnan(host[:, 0])
  assert np.array_equal(host[ok, 0], dev[ok, 0])
  assert (np.abs(host[ok] - dev[ok]) <= 2 * 20 * 2.0 ** -53 * np.maximum(host[ok], dev[ok])).all()
  # the lists themselves: the device path's strip merge against recommend_array
  from recoder_amd.data import UsersInteractions
  ui = UsersInteractions(np.arange(n_users), tr)
  ids, ld = rec._recommend_device(ui, 20)
  assert np.array_equal(ids.cpu().numpy(), rec.recommend_array(ui, 20))


# ---------------------------------------------------- training is undisturbed
def _call(rec, trainer, train_ds, settings, **kw):
  """A fit with the validation ``settings`` (None: without): as keywords, or through ``Recoder.fit_validation`` for
  train_ssm and train_ultragcn, whose parameter lists are pinned by their contract tests."""
  if settings is None:
    return getattr(rec, trainer)(train_ds, **kw)
  if trainer not in ("train_ssm", "train_ultragcn"):
    return getattr(rec, trainer)(train_ds, **kw, **settings)
  rec.fit_validation = settings
  try:
    return getattr(rec, trainer)(train_ds, **kw)
  finally:
    rec.fit_validation = None


FITS = {
    "train_bpr": ("bpr", dict(batch_size=256, seed=0)),
    "train_lightgcn": ("lightgcn", dict(num_layers=2, batch_size=256, seed=0)),
    "train_ssm": ("ssm", dict(num_layers=1, batch_size=256, num_negatives=64, normalize=True, seed=0)),
}


def _fit(data, trainer, epochs, validate, **extra):
  _, _, train_ds, val_ds, start = data
  prefix, kw = FITS[trainer]
  kw = dict(kw, **extra)
  vkw = {k: kw.pop(k) for k in list(kw) if k in ("patience", "restore_best", "eval_freq")}
  rec = _start(_recoder(), trainer, train_ds, start, **kw)
  hist = _call(rec, trainer, train_ds, dict(val_dataset=val_ds, eval_metric=METRIC, **vkw) if validate else None,
               num_epochs=epochs, **kw)
  return rec, hist, prefix


@pytest.mark.parametrize("trainer", ["train_bpr", "train_lightgcn"])
def test_validation_does_not_disturb_training(data, trainer):
  plain, hist0, prefix = _fit(data, trainer, 3, False)
  watched, hist1, _ = _fit(data, trainer, 3, True, restore_best=False)
  assert hist0 == hist1 and _same(_tables(plain), _tables(watched))
  if prefix != "bpr":
    assert _same(_state(plain, prefix), _state(watched, prefix))
  v = getattr(watched, prefix + "_validation")
  assert getattr(plain, prefix + "_validation") is None
  assert (v["metric"], v["k"], v["epochs"], v["stopped_epoch"]) == ("Recall@20", 20, [1, 2, 3], None)
  assert len(v["values"]) == 3 and all(0 < x <= 1 for x in v["values"])


@pytest.mark.parametrize("trainer", ["train_bpr", "train_lightgcn", "train_ssm"])
def test_the_curve_is_the_truth(data, trainer):
  """values[e] is evaluate(on_device=True) after a separate fit of e + 1 epochs from the same start; train_ssm with
  normalize=True scores the row-normalised tables an epoch's end would leave, and leaves the fit itself alone."""
  val_ds = data[3]
  watched, hist, prefix = _fit(data, trainer, 3, True, restore_best=False)
  values = getattr(watched, prefix + "_validation")["values"]
  for e in range(3):
    short, hist_e, _ = _fit(data, trainer, e + 1, False)
    assert values[e] == _score(short, val_ds), (trainer, e)
    assert hist_e == hist[:e + 1]
  assert _same(_tables(short), _tables(watched))


# ------------------------------------------------------------------- restore
# The learning rates below are far above the trainers' defaults (Adam at 0.5 against 0.01, SGD at 1.0 against 0.1): on
# the planted 200 x 120 matrix the validation Recall@20 falls within the first epochs, so that patience=1 stops the
# fit early.  Where it stops is read off the unwatched curve with the host rule, not assumed.
RESTORE = {"train_lightgcn": dict(lr=0.5), "train_bpr": dict(lr=1.0)}


@pytest.mark.parametrize("trainer", ["train_lightgcn", "train_bpr"])
def test_patience_stops_and_restores_the_best_epoch(data, trainer):
  from recoder_amd.validation import EarlyStopping
  train_ds, val_ds = data[2], data[3]
  epochs = 6
  free, _, prefix = _fit(data, trainer, epochs, True, restore_best=False, **RESTORE[trainer])
  curve = getattr(free, prefix + "_validation")["values"]
  rule = EarlyStopping(1)
  for e, v in enumerate(curve):
    if rule.update(e + 1, v)[1]:
      break
  print(trainer, "validation curve", curve)
  assert rule.stopped_epoch is not None and rule.stopped_epoch < epochs, curve       # (the setting must make it fall)
  rec, hist, _ = _fit(data, trainer, epochs, True, patience=1, **RESTORE[trainer])
  v = getattr(rec, prefix + "_validation")
  assert (v["best_epoch"], v["stopped_epoch"]) == (rule.best_epoch, rule.stopped_epoch)
  assert v["values"] == curve[:rule.stopped_epoch] and len(hist) == rule.stopped_epoch
  best, hist_b, _ = _fit(data, trainer, rule.best_epoch, False, **RESTORE[trainer])
  assert _same(_tables(rec), _tables(best)) and hist[:rule.best_epoch] == hist_b
  if prefix == "bpr":
    return
  assert _same(_state(rec, prefix), _state(best, prefix))
  kw = dict(FITS[trainer][1], **RESTORE[trainer])
  assert rec.train_lightgcn(train_ds, num_epochs=1, resume=True, **kw) == \
      best.train_lightgcn(train_ds, num_epochs=1, resume=True, **kw)
  assert _same(_tables(rec), _tables(best)) and _same(_state(rec, prefix), _state(best, prefix))


# ---------------------------------------------------------- the other trainers
@pytest.mark.parametrize("trainer,prefix,kw", [
    ("train_warp", "warp", dict(batch_size=256)),
    ("train_simgcl", "simgcl", dict(num_layers=1, batch_size=256)),
    ("train_directau", "directau", dict(num_layers=1, batch_size=256)),
    ("train_ultragcn", "ultragcn", dict(batch_size=256, num_negatives=8, neighbours=4)),
])
def test_the_other_trainers_validate(data, trainer, prefix, kw):
  _, _, train_ds, val_ds, start = data
  rec = _start(_recoder(), trainer, train_ds, start, **kw)
  hist = _call(rec, trainer, train_ds, dict(val_dataset=val_ds, eval_metric=METRIC, restore_best=False),
               num_epochs=2, **kw)
  v = getattr(rec, prefix + "_validation")
  assert len(hist) == 2 and len(v["values"]) == 2 and v["epochs"] == [1, 2] and v["best_epoch"] in (1, 2)
  assert v["values"][-1] == _score(rec, val_ds)
