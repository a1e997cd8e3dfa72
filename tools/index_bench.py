#!/usr/bin/env python
"""Exact item-similarity throughput (recoder_amd.embedding / include/recoder_index.h), one JSON line per
measurement:

    python tools/index_bench.py [--quick] [--no-torch]

  normalize  rk_ix_normalize over the table: bytes/s (one read + one write of [N, h] floats)
  scores     rk_ix_scores over the whole catalogue for Q queries, in the strips and query chunks knn uses:
             TFLOP/s (2 Q N h) and its fraction of the 157.3 TF f32-MFMA peak
  knn        ExactEmbeddingsIndex.knn end to end: queries/s, and the share of its time that is not scoring
             (the per-strip top-n + the merge)
  torch      the same search as torch.mm + a stable descending torch.sort, in query chunks of <= 128 MB of scores
  table      neighbor_table(10) at C2's shape
  recommend  SimilarityRecommender.recommend for 500 users (UsersInteractions, n = 10, 100 recommendations)

Shapes: (N, h) = (20 108, 200) (C2's catalogue) and (1 000 000, 200) (C5's); Q in {1, 500, 4096}, n in {10, 100}.
Times are host clocks around work that ends in a device synchronise, median of the repeats after a warm-up.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA_TF = 157.3
SHAPES = [("c2", 20108, 200), ("c5", 1000000, 200)]


def timed(fn, reps, warmup=1):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
  return float(np.median(ts))


def emit(rec):
  print(json.dumps(rec), flush=True)


def scores_only(index, Qn, n):
  """rk_ix_scores over the strips and query chunks knn(Qn, n) uses, without the selection."""
  from recoder_amd import embedding
  En = index.normalized()
  N = En.shape[0]
  bounds = index._strips(N, n)
  ld = -(-max(hi - lo for lo, hi in bounds) // 32) * 32
  Q = Qn.shape[0]
  qc = max(1, min(Q, embedding._SCORE_BYTES // (4 * ld)))
  buf = torch.empty(qc * ld, dtype=torch.float32, device=En.device)
  for q0 in range(0, Q, qc):
    q1 = min(Q, q0 + qc)
    S = buf[:(q1 - q0) * ld].view(q1 - q0, ld)
    for lo, hi in bounds:
      index.scores(Qn[q0:q1], lo, hi, S)


def torch_search(En, Qn, n):
  N = En.shape[0]
  qc = max(1, min(Qn.shape[0], (128 << 20) // (4 * N)))
  out = []
  for q0 in range(0, Qn.shape[0], qc):
    s = torch.mm(Qn[q0:q0 + qc], En.t())
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    out.append(i[:, :n])
  return torch.cat(out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="C2's shape only, fewer repeats (for the profiler run)")
  ap.add_argument("--no-torch", action="store_true", help="skip the torch.mm + torch.sort comparison")
  args = ap.parse_args()
  from recoder_amd.data import UsersInteractions
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.recommender import SimilarityRecommender
  import scipy.sparse as sp
  dev = torch.device("cuda")
  shapes = SHAPES[:1] if args.quick else SHAPES
  reps = 3 if args.quick else 5
  for tag, N, h in shapes:
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    emb = torch.randn(N, h, device=dev, generator=g)
    index = ExactEmbeddingsIndex(embeddings=emb)
    index.build()
    En = index.normalized()

    def normalize():
      index._En = None
      index.normalized()
    t = timed(normalize, reps)
    emit({"what": "normalize", "shape": tag, "N": N, "h": h, "ms": t * 1e3, "GB_per_s": 2 * N * h * 4 / t / 1e9})
    for Q in (1, 500, 4096):
      rows = torch.randint(0, N, (Q,), device=dev, generator=g)
      Qn = En.index_select(0, rows)
      for n in (10, 100):
        ts = timed(lambda: scores_only(index, Qn, n), reps)
        tk = timed(lambda: index.knn(rows, n), reps)
        flop = 2.0 * Q * N * h
        rec = {"what": "knn", "shape": tag, "N": N, "h": h, "Q": Q, "n": n,
               "scores_ms": ts * 1e3, "scores_TFLOPs": flop / ts / 1e12,
               "scores_frac_f32_mfma_peak": flop / ts / 1e12 / PEAK_F32_MFMA_TF,
               "knn_ms": tk * 1e3, "queries_per_s": Q / tk, "topk_share": max(0.0, (tk - ts) / tk)}
        if not args.no_torch:
          i_ref = torch_search(En, Qn, n)
          tt = timed(lambda: torch_search(En, Qn, n), 1 if N > 100000 else reps)
          rec.update({"torch_mm_sort_ms": tt * 1e3, "speedup_vs_torch": tt / tk,
                      "top1_equal_torch": float((index.knn(rows, n)[0][:, 0] == i_ref[:, 0]).float().mean())})
        emit(rec)
    if tag == "c2":
      def table():
        index._tables.clear()
        index.neighbor_table(10)
      t = timed(table, reps)
      emit({"what": "neighbor_table", "shape": tag, "N": N, "h": h, "n": 10, "ms": t * 1e3, "items_per_s": N / t})
      rng = np.random.RandomState(0)
      U = 500
      lens = rng.randint(5, 200, size=U)
      indptr = np.concatenate([[0], np.cumsum(lens)])
      cols = np.concatenate([np.sort(rng.choice(N, L, replace=False)) for L in lens])
      m = sp.csr_matrix((np.ones(len(cols), np.float32), cols, indptr), shape=(U, N))
      inp = UsersInteractions(np.arange(U), m)
      rec = SimilarityRecommender(index, 100, n=10)
      t = timed(lambda: rec.recommend(inp), reps)
      emit({"what": "recommend", "shape": tag, "N": N, "h": h, "users": U, "mean_history": float(lens.mean()),
            "n": 10, "num_recommendations": 100, "ms": t * 1e3, "users_per_s": U / t})


if __name__ == "__main__":
  main()
