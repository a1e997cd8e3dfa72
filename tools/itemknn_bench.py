#!/usr/bin/env python
"""ItemKNN fit and serving times (recoder_amd/itemknn.py, rk_rp3_item_fit), one JSON line per run:

    python tools/itemknn_bench.py [--data c2|slice] [--quality] [--no-torch] [--no-rp3] [--out FILE]
    python tools/itemknn_bench.py --cpu-grid [--jobs N] [--out FILE]        (no GPU)

  hip     ms of rk_rp3_item_fit (HIP events, mean of 5 calls after a warm one) at the model's defaults, without
          values (the slice and c2 are binary: the kernel's all-1.0 form) and with tfidf values (the fmaf form),
          multiply-adds per second with adds = sum over the users of r_v^2 (what the accumulation performs);
          ms of rk_rp3_fit on the same matrix, same K (what the value loads and the division cost); users/s of
          ``recommend_array`` (rk_slim_scores + rk_topk_masked) at B = 500, k = 100, beside RP3beta's
  torch   the fit restated in torch ops on the same GPU, in a guarded step (an op this torch build does not
          have is reported as null, not as a failure): row-blocked torch.sparse.mm of the item-major matrix
          with the dense matrix, the denominator, the diagonal at 0 and torch.topk
  quality (--quality, on the ML-20M slice) Recall@20 and NDCG@100 over a small grid through
          ``Recoder.evaluate``
  --cpu-grid  the float64 comparator (tests/itemknn_util.py) over neighbours x shrink x similarity / feature
          weighting on the slice, one line per point, to profiles/itemknn_quality.jsonl: the grid the model's
          defaults come from

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz: above rk_rp3_lds_items(), so the workspace form).
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, event_ms, guarded, load  # noqa: E402

B, K = 500, 100
GRID = [(200, 300.0, "cosine", "none"), (200, 0.0, "cosine", "none"), (100, 100.0, "cosine", "none"),
        (200, 300.0, "cosine", "tfidf"), (200, 300.0, "cosine", "bm25"), (200, 300.0, "jaccard", "none"),
        (200, 300.0, "dice", "none"), (200, 300.0, "asymmetric", "none")]
CPU_NEIGHBOURS = (50, 100, 200, 400)
CPU_SHRINKS = (0.0, 5.0, 20.0, 100.0, 300.0, 1000.0)
CPU_KINDS = [("cosine", "none", 0.5), ("cosine", "tfidf", 0.5), ("cosine", "bm25", 0.5), ("jaccard", "none", 0.5),
             ("dice", "none", 0.5), ("asymmetric", "none", 0.3), ("asymmetric", "none", 0.5),
             ("asymmetric", "none", 0.7)]


# ------------------------------------------------------------------ CPU grid
def cpu_point(cfg):
  from tests import itemknn_util as iu
  similarity, weighting, alpha, shrink = cfg
  x, y = load("slice")
  A = iu.weighted_f64(x, weighting)
  form, own, oth, g, binary = iu.vectors_f64(A, similarity, alpha)
  W = iu.sims_f64(A, form, own, oth, g, shrink, binary)
  rows = []
  for nb in CPU_NEIGHBOURS:
    r, n = iu.quality(x, y, iu.cut_columns(W, nb))
    rows.append(dict(similarity=similarity, feature_weighting=weighting,
                     asymmetric_alpha=alpha if similarity == "asymmetric" else None, shrink=shrink, neighbours=nb,
                     recall20=r, ndcg100=n))
  return rows


def cpu_grid(out, jobs):
  from multiprocessing import Pool
  from tests import itemknn_util as iu
  from tests import rp3_util
  x, y = load("slice")
  pop, = rp3_util.metric_means(iu.popularity_lists(x, 20), y, ks=((20, "recall"),))
  emit(dict(bench="itemknn_quality", data="slice", comparator="float64 (tests/itemknn_util.py)", popularity_recall20=pop),
       out)
  cfgs = [(s, f, a, sh) for s, f, a in CPU_KINDS for sh in CPU_SHRINKS]
  with Pool(jobs) as pool:
    rows = [row for rows in pool.map(cpu_point, cfgs) for row in rows]
  for row in rows:
    emit(row, out)
  best = max((r for r in rows if r["neighbours"] <= 200), key=lambda r: r["recall20"])
  print("best Recall@20 at neighbours <= 200: %s" % best)


# ----------------------------------------------------------------------- GPU
def serve_time(rec, inp, reps=10):
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  return (time.perf_counter() - t0) / reps


def hip_side(x, out, with_rp3):
  import torch
  from recoder_amd import als, itemknn, rp3
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel, RandomWalkItemModel
  rec = Recoder(model=ItemNeighbourhoodModel())
  ds = RecommendationDataset(x)
  info = rec.train_itemknn(ds)
  m = rec.model
  p = m.model_params()
  dev = "cuda"
  pair = als.csr_pair(x, x.shape[0], x.shape[1], dev)
  ids, w, count = torch.empty_like(m.item_neighbours), torch.empty_like(m.item_weights.data), \
      torch.empty_like(m.neighbour_counts)
  adds = float((np.diff(x.indptr).astype(np.float64) ** 2).sum())
  out.update(n=info["n"], nnz=info["nnz"], neighbours=p["neighbours"], shrink=p["shrink"], similarity=p["similarity"],
             kept=info["kept"], adds=adds)
  state = {}
  for tag, weighting in (("", p["feature_weighting"]), ("tfidf_", "tfidf")):
    ud, td, form, own, oth, g = itemknn.host_inputs(pair, p["similarity"], weighting)
    if ud is not None:
      ud, td = torch.from_numpy(ud).to(dev), torch.from_numpy(td).to(dev)
    own, oth = torch.from_numpy(own).to(dev), torch.from_numpy(oth).to(dev)

    def fit():
      state["ws"] = itemknn.fit_columns(*pair, ud, td, own, oth, form, g, p["shrink"], ids, w, count,
                                        ws=state.get("ws"))
    ms = event_ms(fit, 5)
    out.update({tag + "fit_ms": ms, tag + "adds_per_s": adds / (ms * 1e-3), tag + "values": ud is not None})
  uw, rs, cs = (torch.from_numpy(a).to(dev) for a in rp3.host_weights(pair, 0.6, 0.3))
  rp3_ms = event_ms(lambda: rp3.fit_rows(*pair, uw, rs, cs, ids, w, count, ws=state["ws"]), 5)
  out.update(rp3_fit_ms=rp3_ms, fit_vs_rp3_fit=out["fit_ms"] / rp3_ms, tfidf_fit_vs_rp3_fit=out["tfidf_fit_ms"] / rp3_ms)
  users = np.arange(min(B, x.shape[0]))
  inp = UsersInteractions(users, x[users])
  dt = serve_time(rec, inp)
  out.update(serve_batch=len(users), serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt)
  if with_rp3:
    other = Recoder(model=RandomWalkItemModel())
    other.train_rp3beta(ds)
    dr = serve_time(other, inp)
    out.update(rp3_serve_ms=dr * 1e3, rp3_serve_users_per_s=len(users) / dr)
    del other
    torch.cuda.empty_cache()
  return rec


def torch_fit(x, nb, shrink, block=2048):
  """The default fit (cosine on the matrix as stored) in torch ops; returns its ms."""
  import torch
  dev = "cuda"
  n = x.shape[1]
  a = sp.csr_matrix(x).astype(np.float32)
  xd = torch.as_tensor(np.asarray(a.todense()), device=dev)
  norm = torch.as_tensor(np.sqrt(np.asarray(a.multiply(a).sum(axis=0)).ravel()).astype(np.float32), device=dev)
  xt = a.T.tocsr()
  ids = torch.empty(n, nb, dtype=torch.int64, device=dev)
  w = torch.empty(n, nb, dtype=torch.float32, device=dev)
  blocks = []
  for lo in range(0, n, block):
    c = xt[lo:lo + block].tocoo()
    blocks.append((lo, torch.sparse_coo_tensor(np.vstack([c.row, c.col]), c.data, c.shape).to(dev).coalesce()))
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  for lo, blk in blocks:
    hi = lo + blk.shape[0]
    W = torch.sparse.mm(blk, xd)                        # [own j in the block, i]
    W /= norm[lo:hi, None] * norm[None, :] + shrink
    W[torch.arange(hi - lo, device=dev), torch.arange(lo, hi, device=dev)] = 0
    w[lo:hi], ids[lo:hi] = torch.topk(W, min(nb, n), dim=1)
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1)


def torch_side(x, out):
  ok = x.shape[0] * x.shape[1] * 4 <= 2 ** 34
  res = guarded(lambda: (torch_fit(x, out["neighbours"], out["shrink"]),
                         torch_fit(x, out["neighbours"], out["shrink"]))[1]) if ok else None
  out["torch_fit_ms"] = res
  if res is not None:
    out["fit_speedup_vs_torch"] = res / out["fit_ms"]


def quality(x, y, out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel
  ds, ev = RecommendationDataset(x), RecommendationDataset(x, y)
  metrics = [Recall(k=20, normalize=True), NDCG(k=100)]
  grid = []
  for nb, shrink, similarity, weighting in GRID:
    rec = Recoder(model=ItemNeighbourhoodModel(nb, shrink, similarity, weighting))
    rec.train_itemknn(ds)
    res = rec.evaluate(ev, num_recommendations=100, metrics=metrics, batch_size=B)
    row = dict(neighbours=nb, shrink=shrink, similarity=similarity, feature_weighting=weighting)
    row.update({str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()})
    print("ItemKNN %s" % row)
    grid.append(row)
  out["grid"] = grid


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--data", choices=["c2", "slice"], action="append")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--no-rp3", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--jobs", type=int, default=4)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    cpu_grid(args.out or os.path.join(ROOT, "profiles", "itemknn_quality.jsonl"), args.jobs)
    return
  import torch
  dest = args.out or os.path.join(ROOT, "profiles", "itemknn_bench.jsonl")
  for name in (args.data or ["slice", "c2"]):
    x, y = load(name)
    out = dict(bench="itemknn", data=name, users=int(x.shape[0]), device=torch.cuda.get_device_name(0))
    rec = hip_side(x, out, not args.no_rp3)
    if not args.no_torch:
      torch_side(x, out)
    if args.quality and y is not None:
      quality(x, y, out)
    emit(out, dest)
    del rec
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
