#!/usr/bin/env python
"""UserKNN serving times (recoder_amd/userknn.py, the rk_rp3_user_* kernels), one JSON line per run:

    python tools/userknn_bench.py [--data c2|slice] [--quality] [--no-torch] [--no-rp3] [--out FILE]

  hip     ms of rk_rp3_user_neighbours and of rk_rp3_user_scores over the whole catalogue (HIP events, mean
          of 10 after a warm call) for B = 500 training users as queries, and users/s of
          ``recommend_array`` (neighbours + scores + rk_topk_masked, k = 100) beside RP3beta's serving rate
          on the same matrix and the same users
  torch   the same batch in torch ops on the same GPU, in a guarded step (an op this torch build does not
          have is reported as null, not as a failure): torch.sparse.mm of the query rows with the dense
          binary X^T, the scaling, torch.topk, and a sparse product with X for the scores
  quality (--quality, on the ML-20M slice) Recall@20 and NDCG@100 over a small (neighbours, shrink) grid
          through ``Recoder.evaluate``

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz: more users than rk_rp3_lds_items(), so the workspace path).
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, event_ms, guarded, load  # noqa: E402

B, K = 500, 100
GRID = [(n, s) for n in (100, 200, 400, 800) for s in (0.0, 10.0)]


def serve_time(rec, inp, reps=10):
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  return (time.perf_counter() - t0) / reps


def hip_side(x, out, with_rp3):
  from recoder_amd import userknn
  from recoder_amd.als import AlsCSR
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel, UserNeighbourhoodModel
  rec = Recoder(model=UserNeighbourhoodModel())
  ds = RecommendationDataset(x)
  info = rec.train_userknn(ds)
  m = rec.model
  users = np.arange(min(B, x.shape[0]))
  q = AlsCSR(x[users], "cuda")
  ucsr, icsr = m._csrs()
  qn = userknn.query_norms(q)
  state = {}

  def nb():
    *state["nbr"], state["ws"] = userknn.neighbours(q, icsr, m.user_norms, m.neighbours, m.shrink, qn=qn,
                                                    ws=state.get("ws"))
  nb_ms = event_ms(nb, 10)
  buf = torch.empty(len(users), x.shape[1], dtype=torch.float32, device="cuda")
  sc_ms = event_ms(lambda: userknn.scores(state["nbr"], ucsr, out=buf), 10)
  r = np.diff(x.indptr)[users].astype(np.float64)
  d = np.diff(x.T.tocsr().indptr).astype(np.float64)
  adds = float(sum(d[x.indices[x.indptr[u]:x.indptr[u + 1]]].sum() for u in users))
  out.update(n_users=info["n_users"], n=info["n"], nnz=info["nnz"], neighbours=info["neighbours"],
             shrink=info["shrink"], batch=len(users), neighbours_ms=nb_ms, scores_ms=sc_ms, count_adds=adds,
             count_adds_per_s=adds / (nb_ms * 1e-3))
  inp = UsersInteractions(users, x[users])
  dt = serve_time(rec, inp)
  out.update(serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt)
  if with_rp3:
    rp3 = Recoder(model=RandomWalkItemModel())
    rp3.train_rp3beta(ds)
    dr = serve_time(rp3, inp)
    out.update(rp3_serve_ms=dr * 1e3, rp3_serve_users_per_s=len(users) / dr)
    del rp3
    torch.cuda.empty_cache()
  return rec


def torch_batch(x, N, shrink):
  """The same batch in torch ops; returns the ms of (similarities, top-N, scores)."""
  dev = "cuda"
  users = np.arange(min(B, x.shape[0]))
  bx = sp.csr_matrix(x).astype(bool).astype(np.float32)
  bt = torch.as_tensor(np.asarray(bx.T.todense()), device=dev)                 # [n, U] dense
  c = bx[users].tocoo()
  q = torch.sparse_coo_tensor(np.vstack([c.row, c.col]), c.data, c.shape).to(dev).coalesce()
  xc = sp.csr_matrix(x).astype(np.float32).T.tocoo()                             # X^T: scores^T = X^T kept^T
  xt = torch.sparse_coo_tensor(np.vstack([xc.row, xc.col]), xc.data, xc.shape).to(dev).coalesce()
  un = torch.as_tensor(np.sqrt(np.diff(x.indptr).astype(np.float64)).astype(np.float32), device=dev)
  qn = un[torch.as_tensor(users, device=dev)]

  def run():
    sim = torch.sparse.mm(q, bt)
    sim /= qn[:, None] * un[None, :] + shrink
    w, ids = torch.topk(sim, min(N, sim.shape[1]), dim=1)
    kept = torch.zeros_like(sim).scatter_(1, ids, w)
    return torch.sparse.mm(xt, kept.t().contiguous()).t()
  return event_ms(run, 5)


def torch_side(x, out):
  ok = x.shape[0] * x.shape[1] * 4 <= 2 ** 34
  res = guarded(lambda: torch_batch(x, out["neighbours"], out["shrink"])) if ok else None
  out["torch_batch_ms"] = res
  if res is not None:
    out["speedup_vs_torch"] = res / (out["neighbours_ms"] + out["scores_ms"])


def quality(x, y, out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import UserNeighbourhoodModel
  ds, ev = RecommendationDataset(x), RecommendationDataset(x, y)
  metrics = [Recall(k=20, normalize=True), NDCG(k=100)]
  grid = []
  for nb, shrink in GRID:
    rec = Recoder(model=UserNeighbourhoodModel(nb, shrink))
    rec.train_userknn(ds)
    res = rec.evaluate(ev, num_recommendations=100, metrics=metrics, batch_size=B)
    row = dict(neighbours=nb, shrink=shrink)
    row.update({str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()})
    print("UserKNN %s" % row)
    grid.append(row)
  out["grid"] = grid


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--data", choices=["c2", "slice"], action="append")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--no-rp3", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "userknn_bench.jsonl"))
  args = ap.parse_args()
  for name in (args.data or ["slice", "c2"]):
    x, y = load(name)
    out = dict(bench="userknn", data=name, device=torch.cuda.get_device_name(0))
    rec = hip_side(x, out, not args.no_rp3)
    if not args.no_torch:
      torch_side(x, out)
    if args.quality and y is not None:
      quality(x, y, out)
    emit(out, args.out)
    del rec
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
