"""rk_als_rank_metrics restated in numpy: the kernel's arithmetic, every floating-point sum a sequential float64
chain in ascending rank order, the sum over the users in the kernel's fixed order (256 strided partials, then a
halving tree).  Shared by tests/test_rank_metrics_host.py (against recoder_amd.metrics' per-user functions) and
tests/test_rank_metrics.py (against the kernel)."""
import numpy as np

from recoder_amd import metrics as M

SUM_THREADS = 256


def specs_of(metrics):
  """(kind, k, normalize) per metric, kind in 'recall' / 'ndcg' / 'ap'."""
  out = []
  for m in metrics:
    kind = {M.Recall: "recall", M.NDCG: "ndcg", M.AveragePrecision: "ap"}[type(m)]
    out.append((kind, int(m.k), bool(getattr(m, "normalize", True))))
  return out


def tables(max_k):
  """(inv_w, ideal) as metrics.batch_metrics builds them: 1 / log2(2 + r) and its cumulative sum from 0."""
  inv_w = 1.0 / np.log2(2 + np.arange(max(int(max_k), 1)))
  return inv_w, np.concatenate([[0.0], np.cumsum(inv_w)])


def user_values(rec, y, specs, inv_w, ideal):
  """One user's values: ``rec`` the K ids, ``y`` the ascending target ids."""
  K, ny = len(rec), len(y)
  hit = np.zeros(K, dtype=bool)
  if ny:
    pos = np.minimum(np.searchsorted(y, rec), ny - 1)
    hit = np.asarray(y)[pos] == rec
  out = []
  with np.errstate(divide="ignore", invalid="ignore"):
    for kind, k, normalize in specs:
      kk = min(k, K)
      capped = min(k, ny)
      norm = np.float64(capped if normalize else ny)
      acc, cum = np.float64(0.0), 0
      for r in range(kk):
        if hit[r]:
          cum += 1
          if kind == "ndcg":
            acc = acc + inv_w[r]
          elif kind == "ap":
            acc = acc + np.float64(cum) / np.float64(r + 1)
      if kind == "recall":
        out.append(np.float64(int(hit[:kk].sum())) / norm)
      elif kind == "ap":
        out.append(acc / norm)
      else:
        out.append(acc / np.float64(ideal[capped]))
  return out


def fixed_order_sums(values):
  """(sums [n], count) of the non-nan rows in the kernel's order."""
  B, n = values.shape
  sums = np.zeros(n)
  count = 0
  for m in range(n):
    part = np.zeros(SUM_THREADS)
    cnt = np.zeros(SUM_THREADS, dtype=np.int64)
    for t in range(min(SUM_THREADS, B)):
      for v in values[t::SUM_THREADS, m]:
        if v == v:
          part[t] = part[t] + v
          cnt[t] += 1
    off = SUM_THREADS // 2
    while off:
      part[:off] = part[:off] + part[off:2 * off]
      cnt[:off] = cnt[:off] + cnt[off:2 * off]
      off //= 2
    sums[m] = part[0]
    if m == 0:
      count = int(cnt[0])
  return sums, count


def rank_metrics(recs, target_csr, metrics):
  """(values [B, n] float64, sums [n], count) for recs [B, K] int64 and the first B rows of ``target_csr``."""
  recs = np.asarray(recs, dtype=np.int64)
  specs = specs_of(metrics)
  inv_w, ideal = tables(max(k for _, k, _ in specs))
  tm = target_csr.tocsr().copy()
  tm.eliminate_zeros()
  tm.sort_indices()
  values = np.array([user_values(recs[u], tm.indices[tm.indptr[u]:tm.indptr[u + 1]].astype(np.int64), specs, inv_w,
                                 ideal) for u in range(recs.shape[0])], dtype=np.float64).reshape(recs.shape[0], -1)
  return (values,) + fixed_order_sums(values)


# ------------------------------------------------------------------ the cases
K_CASES = (1, 20, 64, 65, 100)
N_ITEMS = 5000
ROW_KINDS = ("empty", "one", "three", "long", "first", "last", "all", "none")


def make_case(K, B, seed):
  """B random lists of K distinct ids over N_ITEMS items and a target matrix whose rows cycle through ROW_KINDS:
  no target, 1, 3 and 2 000 targets, the first / the last target id recommended, every recommendation a hit, none."""
  import scipy.sparse as sp
  rng = np.random.default_rng(seed)
  recs = np.stack([rng.permutation(N_ITEMS)[:K] for _ in range(B)]).astype(np.int64)
  rows, cols = [], []
  for u in range(B):
    kind = ROW_KINDS[u % len(ROW_KINDS)]
    rest = np.setdiff1d(np.arange(N_ITEMS), recs[u])
    if kind == "empty":
      y = np.zeros(0, dtype=np.int64)
    elif kind in ("one", "three", "long"):
      y = rng.choice(N_ITEMS, {"one": 1, "three": 3, "long": 2000}[kind], replace=False)
    elif kind == "first":          # the smallest target id is recommended, nothing else of the row
      y = np.concatenate([[recs[u, K // 2]], rest[rest > recs[u, K // 2]][:7]])
    elif kind == "last":           # the largest
      y = np.concatenate([rest[rest < recs[u, 0]][:7], [recs[u, 0]]])
    elif kind == "all":
      y = np.concatenate([recs[u], rest[:5]])
    else:
      y = rest[:40]
    rows += [u] * len(y)
    cols += list(y)
  tm = sp.csr_matrix((np.ones(len(rows), dtype=np.float32), (rows, cols)), shape=(B, N_ITEMS))
  if B > 2:                        # a stored zero is no target
    tm.data[tm.indptr[2]] = 0.0
  return recs, tm


def metric_set(K):
  """Every kind at the cutoffs 1, K and K + 5, normalize on and off, in calls of at most 8 metrics."""
  ks = sorted({1, K, K + 5})
  a = [M.Recall(k, normalize=n) for k in ks for n in (True, False)]
  b = [M.AveragePrecision(k, normalize=n) for k in ks for n in (True, False)]
  c = [M.NDCG(k) for k in ks]
  return [a, b, c + [M.Recall(ks[-1]), M.AveragePrecision(ks[0], normalize=False)]]


def bound(K, a, b):
  """|a - b| allowed between two float64 sums of at most K non-negative terms added in different orders."""
  return 2.0 * K * 2.0 ** -53 * max(abs(a), abs(b))
