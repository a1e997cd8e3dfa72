"""Ranking metrics + evaluator with the reference's API (recoder/metrics.py).

The metric arithmetic (metrics.py:9-45) is host-side numpy on the top-k lists
the GPU produces (``Recoder.recommend`` -> ``rk_topk_masked``); it is pinned by
the reference's own known-answer tests (tests/test_metrics.py:12-54, restated
in tests/test_host_logic.py here).
"""
import numpy as np

from .data import RecommendationDataLoader


def _hits(x, y, k):
  x = np.asarray(x)[:k]
  return x, np.isin(x, y, assume_unique=True).astype(int)


def average_precision(x, y, k, normalize=True):
  x, hit = _hits(x, y, k)
  precision = hit.cumsum() / (1 + np.arange(len(x)))
  normalization = min(k, len(y)) if normalize else len(y)
  return np.multiply(precision, hit).sum() / normalization


def recall(x, y, k, normalize=True):
  x, hit = _hits(x, y, k)
  normalization = min(k, len(y)) if normalize else len(y)
  return hit.sum() / normalization


def dcg(x, y, k):
  x, hit = _hits(x, y, k)
  return (hit / np.log2(2 + np.arange(len(x)))).sum()


def ndcg(x, y, k):
  return dcg(x, y, k) / dcg(y, y, k)


class Metric(object):
  """Base class for metrics (metrics.py:48-75)."""

  def __init__(self, metric_name):
    self.metric_name = metric_name

  def __str__(self):
    return self.metric_name

  def __hash__(self):
    return self.metric_name.__hash__()

  def evaluate(self, x, y):
    raise NotImplementedError


class AveragePrecision(Metric):
  def __init__(self, k, normalize=True):
    super().__init__(metric_name="AveragePrecision@{}".format(k))
    self.k = k
    self.normalize = normalize

  def evaluate(self, x, y):
    return average_precision(x, y, k=self.k, normalize=self.normalize)


class Recall(Metric):
  def __init__(self, k, normalize=True):
    super().__init__(metric_name="Recall@{}".format(k))
    self.k = k
    self.normalize = normalize

  def evaluate(self, x, y):
    return recall(x, y, k=self.k, normalize=self.normalize)


class NDCG(Metric):
  def __init__(self, k):
    super().__init__(metric_name="NDCG@{}".format(k))
    self.k = k

  def evaluate(self, x, y):
    return ndcg(x, y, k=self.k)


def batch_metrics(recommendations, target_csr, metrics):
  """The three built-in metrics for a whole batch of users at once: {metric: [value per user]},
  or None when it does not apply (a user-defined Metric, ragged recommendation lists) and the
  caller has to loop over the users.  Same arithmetic as average_precision / recall / ndcg above
  (metrics.py:9-45) on a [users, k] hit matrix -- the per-user Python loop made evaluation 100x
  slower than the scoring + top-k it evaluates."""
  if any(type(m) not in (AveragePrecision, Recall, NDCG) for m in metrics):
    return None
  try:
    recs = np.asarray(recommendations)
  except ValueError:
    return None
  if recs.dtype == object or recs.ndim != 2:
    return None
  recs = recs.astype(np.int64, copy=False)
  B, K = recs.shape
  tm = target_csr.tocsr()
  if tm.shape[0] < B:
    return None
  n_items = int(tm.shape[1])
  rows = np.repeat(np.arange(tm.shape[0], dtype=np.int64), np.diff(tm.indptr))
  nz = tm.data != 0
  ykeys = np.sort(rows[nz] * n_items + tm.indices[nz].astype(np.int64))
  ny = np.bincount(rows[nz], minlength=tm.shape[0])[:B].astype(np.int64)
  tkeys = (np.arange(B, dtype=np.int64)[:, None] * n_items + recs).ravel()
  if len(ykeys):
    pos = np.minimum(np.searchsorted(ykeys, tkeys), len(ykeys) - 1)
    # (an id outside the catalogue is a miss: recommend_filtered's padding id -1 would alias the row before's last item)
    hit = ((ykeys[pos] == tkeys).reshape(B, K) & (recs >= 0) & (recs < n_items)).astype(int)
  else:
    hit = np.zeros((B, K), dtype=int)
  out = {}
  with np.errstate(divide="ignore", invalid="ignore"):      # (users without targets: nan, as per user)
    for m in metrics:
      k = min(int(m.k), K)
      h = hit[:, :k]
      if isinstance(m, Recall):
        norm = np.minimum(m.k, ny) if m.normalize else ny
        out[m] = (h.sum(axis=1) / norm).tolist()
      elif isinstance(m, AveragePrecision):
        precision = h.cumsum(axis=1) / (1 + np.arange(k))
        norm = np.minimum(m.k, ny) if m.normalize else ny
        out[m] = (np.multiply(precision, h).sum(axis=1) / norm).tolist()
      else:
        w = np.log2(2 + np.arange(max(int(m.k), 1)))
        got = (h / w[:k]).sum(axis=1)
        ideal = np.concatenate([[0.0], np.cumsum(1.0 / w)])[np.minimum(m.k, ny)]
        out[m] = (got / ideal).tolist()
  return out


def sampled_candidates(target_matrix, seen_matrix, num_negatives, seed):
  """The candidate sets of the sampled-negatives protocol (one held-out positive among N sampled negatives, He et
  al. 2017) as a CSR [num_users, n_items] of ones: each user's target items (the stored non-zeros of
  ``target_matrix``) plus ``num_negatives`` items drawn uniformly without replacement from the items that are
  neither stored non-zeros of ``seen_matrix`` nor targets; a user with fewer such items takes all of them.  It is
  the ``user_allow`` of ``Recoder.recommend_filtered`` / ``recommender.FilteredRecommender``.  Host numpy, one
  generator per user seeded with (seed, user): the same arguments give the same matrix, whatever the other rows
  hold."""
  import scipy.sparse as sp
  if isinstance(num_negatives, bool) or not isinstance(num_negatives, (int, np.integer)) or num_negatives < 0:
    raise ValueError("num_negatives must be an integer >= 0 (got %r)" % (num_negatives,))
  tm, sm = sp.csr_matrix(target_matrix), sp.csr_matrix(seen_matrix)
  if tm.shape != sm.shape:
    raise ValueError("target_matrix %r and seen_matrix %r must have one shape" % (tm.shape, sm.shape))
  n_users, n_items = tm.shape
  indptr, indices = np.zeros(n_users + 1, dtype=np.int64), []
  for u in range(n_users):
    t = tm.indices[tm.indptr[u]:tm.indptr[u + 1]][tm.data[tm.indptr[u]:tm.indptr[u + 1]] != 0]
    s = sm.indices[sm.indptr[u]:sm.indptr[u + 1]][sm.data[sm.indptr[u]:sm.indptr[u + 1]] != 0]
    free = np.ones(n_items, dtype=bool)
    free[t] = False
    free[s] = False
    pool = np.nonzero(free)[0]
    rng = np.random.RandomState([int(seed) & 0x7fffffff, u])
    neg = pool if len(pool) <= num_negatives else rng.choice(pool, size=int(num_negatives), replace=False)
    row = np.union1d(t, neg)
    indices.append(row)
    indptr[u + 1] = indptr[u] + len(row)
  indices = np.concatenate(indices) if indices else np.zeros(0, dtype=np.int64)
  return sp.csr_matrix((np.ones(len(indices), dtype=np.float32), indices.astype(np.int32), indptr),
                       shape=(n_users, n_items))


# ---------------------------------------------------------------- on the device
MAX_DEVICE_METRICS = 8        # RK_ALS_RANK_METRICS_MAX: the records of one rk_als_rank_metrics call
_KINDS = {Recall: 0, NDCG: 1, AveragePrecision: 2}      # RK_ALS_METRIC_RECALL, _NDCG, _AP


def device_metrics_ok(metrics):
  """True when ``metrics`` are what rk_als_rank_metrics computes: built-in ones only, 1..8 of them, every k an
  integer >= 1 that fits 32 bits."""
  metrics = list(metrics)
  return 1 <= len(metrics) <= MAX_DEVICE_METRICS and all(
      type(m) in _KINDS and isinstance(m.k, (int, np.integer)) and not isinstance(m.k, bool) and 1 <= m.k < 2 ** 31
      for m in metrics)


class DeviceTarget(object):
  """A batch's target CSR on the device, uploaded once: int64 indptr [B + 1] and int32 indices, ascending within a
  row, stored zeros dropped (as ``batch_metrics`` does with ``tm.data != 0``)."""

  def __init__(self, target_csr, device):
    import torch
    tm = target_csr.tocsr().copy()
    tm.eliminate_zeros()
    tm.sort_indices()
    self.rows, self.nnz = int(tm.shape[0]), int(tm.nnz)
    self.indptr = torch.from_numpy(tm.indptr.astype(np.int64)).to(device)
    self.indices = torch.from_numpy(tm.indices.astype(np.int32)).to(device)


class DeviceMetricTables(object):
  """The metric records of a call and the two float64 tables the kernel divides by, built on the host with numpy --
  1 / log2(2 + r) and its cumulative sum from 0, the doubles ``batch_metrics`` uses -- and uploaded once."""

  def __init__(self, metrics, device):
    import torch
    from ctypes import c_int32
    metrics = list(metrics)
    if not device_metrics_ok(metrics):
      raise ValueError("the device path computes 1..%d of Recall, NDCG and AveragePrecision with integer k >= 1 "
                       "(got %s)" % (MAX_DEVICE_METRICS, ", ".join(str(m) for m in metrics) or "none"))
    n = len(metrics)
    self.n, self.max_k = n, max(int(m.k) for m in metrics)
    self.kinds = (c_int32 * n)(*[_KINDS[type(m)] for m in metrics])
    self.ks = (c_int32 * n)(*[int(m.k) for m in metrics])
    self.normalize = (c_int32 * n)(*[int(bool(getattr(m, "normalize", True))) for m in metrics])
    inv_w = 1.0 / np.log2(2 + np.arange(self.max_k))
    self.inv_w = torch.from_numpy(inv_w).to(device)
    self.ideal = torch.from_numpy(np.concatenate([[0.0], np.cumsum(inv_w)])).to(device)


def device_batch_metrics(recs_dev, ld, target, metrics, tables=None, out=None):
  """``batch_metrics`` without the host: ``recs_dev`` an int64 device tensor whose first B rows of K ids lie ``ld``
  elements apart (a contiguous [B, K] tensor, or a strided view such as ``cand_idx[:, :k]``), ``target`` a
  ``DeviceTarget`` of at least B rows, ``metrics`` 1..8 of Recall / NDCG / AveragePrecision.  Returns (values
  [B, len(metrics)] float64, (sums [len(metrics)] float64, count [1] int64)), all device tensors and nothing
  synchronised: nan for a user without targets, ``sums`` over the other rows, ``count`` of them
  (rk_als_rank_metrics; fixed summation orders, the same inputs give the same bits).  ``tables`` (a
  ``DeviceMetricTables`` of ``metrics``) and ``out`` (an earlier call's three tensors) are reused when given."""
  import torch
  from . import _als_lib
  from ._lib import ptr
  from .device import current_stream
  B, K = int(recs_dev.shape[0]), int(recs_dev.shape[1])
  assert recs_dev.dtype == torch.int64 and recs_dev.dim() == 2 and recs_dev.stride(1) == 1 and int(ld) >= K and \
      (B == 1 or recs_dev.stride(0) == int(ld)), (recs_dev.dtype, recs_dev.shape, recs_dev.stride(), ld)
  if target.rows < B:
    raise ValueError("the target holds %d users, the recommendations %d" % (target.rows, B))
  if tables is None:
    tables = DeviceMetricTables(metrics, recs_dev.device)
  if out is None:
    out = (torch.empty((B, tables.n), dtype=torch.float64, device=recs_dev.device),
           torch.empty(tables.n, dtype=torch.float64, device=recs_dev.device),
           torch.empty(1, dtype=torch.int64, device=recs_dev.device))
  values, sums, count = out
  values = values[:B]
  assert values.is_contiguous() and values.shape[1] == tables.n
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_rank_metrics(ptr(recs_dev), B, K, int(ld), ptr(target.indptr), ptr(target.indices),
                                         target.nnz, tables.n, tables.kinds, tables.ks, tables.normalize,
                                         ptr(tables.inv_w), ptr(tables.ideal), ptr(values), ptr(sums), ptr(count),
                                         current_stream()), "rk_als_rank_metrics")
  return values, (sums, count)


class RecommenderEvaluator(object):
  """Evaluates a recommender on a dataset with input/target interactions
  (metrics.py:135-232).  ``num_workers`` is accepted for compatibility; scoring
  and top-k run on the GPU, the per-user metric arithmetic on the host -- or, with
  ``evaluate(on_device=True)``, on the GPU as well."""

  def __init__(self, recommender, metrics):
    self.recommender = recommender
    self.metrics = metrics

  def _device_lists(self):
    """``recommender``'s device top-k (``recommend_device(inp) -> (ids, ld)``) when it has one and the metrics are
    the kernel's, else None."""
    fn = getattr(self.recommender, "recommend_device", None)
    return fn if fn is not None and device_metrics_ok(self.metrics) else None

  def evaluate(self, eval_dataset, batch_size=1, num_users=None, num_workers=0, on_device=False):
    """``on_device=True``: with a ``Recoder``-backed recommender and only built-in metrics the top-k lists stay on
    the device and rk_als_rank_metrics computes the per-user values, read back as one array per batch; anything
    else takes the host path below."""
    dataloader = RecommendationDataLoader(eval_dataset, batch_size=batch_size,
                                          collate_fn=lambda _: _)
    results = {metric: [] for metric in self.metrics}
    processed = 0
    device_lists = self._device_lists() if on_device else None
    tables = None
    for inp, target in dataloader:
      if device_lists is not None:
        recs_dev, ld = device_lists(inp)
        if tables is None:
          tables = DeviceMetricTables(self.metrics, recs_dev.device)
        values, _ = device_batch_metrics(recs_dev, ld, DeviceTarget(target.interactions_matrix, recs_dev.device),
                                         self.metrics, tables)
        host = values.cpu().numpy()
        for j, metric in enumerate(self.metrics):
          results[metric].extend(host[:, j].tolist())
        processed += len(target.users)
        if num_users is not None and processed >= num_users:
          break
        continue
      as_array = getattr(self.recommender, "recommend_array", None)
      recommendations = as_array(inp) if as_array is not None else self.recommender.recommend(inp)
      tm = target.interactions_matrix.tocsr()
      fast = batch_metrics(recommendations, tm, self.metrics)
      if fast is not None:
        for metric in self.metrics:
          results[metric].extend(fast[metric])
        recommendations = ()
      for i, x in enumerate(recommendations):
        lo, hi = tm.indptr[i], tm.indptr[i + 1]
        y = tm.indices[lo:hi][tm.data[lo:hi] != 0]
        for metric in self.metrics:
          results[metric].append(metric.evaluate(x, y))
      processed += len(target.users)
      if num_users is not None and processed >= num_users:
        break
    return results
