#!/usr/bin/env python
"""ADMM-SLIM quality grid, iteration and serving times (recoder_amd/admm.py, rk_ease_gemm, rk_ease_admm_update), one
JSON line per record:

    python tools/admm_bench.py --cpu-grid [--out FILE]       (no GPU)
    python tools/admm_bench.py --quality [--out FILE]

  --quality   on the GPU, into profiles/admm_bench.jsonl:
          admm_gemm     rk_ease_gemm (the iteration's product, E = A) at n = 7 915 and n = 20 108 (C2's): ms (mean of
                        3 after a warm call), TF/s on 2 n^3 flop, the share of the 157 TF f32-matrix peak, and
                        torch.mm on the same operands
          admm_small    the n = 257 fit of tests/test_admm.py: its error to the float64 loop beside the f32 numpy loop's
          admm_quality  the grid on the ML-20M slice through the kernels: l1 x l2 x rho x nonneg, each run read after
                        10, 25 and 50 iterations (Recall@20, NDCG@100, density, residuals)
          admm          at the model's defaults: gram / inverse / admm ms (second of two fits), ms per iteration
                        split into the product and the update, users/s of rk_ease_scores + rk_topk_masked at
                        B = 500, k = 100, Recall@20 / Recall@50 / NDCG@100
  --cpu-grid  the float64 restatement (tests/admm_util.py) on the slice, into profiles/admm_quality.jsonl: the model's
          default cell and the same cell with l1 = 0, nonneg False (its distance to EASE at reg = l2: what the
          truncation at that (rho, iterations) leaves); each iteration is a 7 915^3 float64 product.  The default
          cell's Recall@20, NDCG@100 and density, the truncation distance and the f32 budget of tests/test_ease.py's
          weights at reg = l2 go to tests/golden/admm_slice.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, event_ms, guarded, load  # noqa: E402

B, K = 500, 100
F32_MATRIX_PEAK_TF = 157.0
# (l1 is kept off the integers: on binary data an integer l1 puts every pair of items that exactly l1 users share, and
# that no other weight reaches, exactly on the threshold, and rounding decides whether it counts as a non-zero)
L1S, L2S, RHOS, READ_AT = (0.25, 0.5, 0.75, 1.5), (500.0, 1000.0, 2000.0), (500.0, 2000.0), (10, 25, 50)
GOLDEN = os.path.join(ROOT, "tests", "golden", "admm_slice.json")


# ------------------------------------------------------------------ the CPU cells
def cpu_grid(out):
  from recoder_amd.nn import AdmmSlimModel
  from tests import admm_util as au, ease_util, gfcf_util as gu
  from tests.test_ease import _weights_budget
  x, y = load("slice")
  p = AdmmSlimModel().model_params()
  src = "float64 restatement (tests/admm_util.py), CPU"
  cells = {}
  for name, l1, nonneg in (("default", p["l1_reg"], p["nonneg"]), ("ease_limit", 0.0, False)):
    t0 = time.perf_counter()
    C, info = au.fit(x, l1, p["l2_reg"], p["rho"], p["num_iterations"], nonneg)
    r20, n100 = gu.quality(x, y, S=ease_util.scores(x, C))
    cells[name] = (C, info)
    emit(dict(bench="admm_quality", cell=name, l1_reg=l1, l2_reg=p["l2_reg"], rho=p["rho"],
              iterations=p["num_iterations"], nonneg=nonneg, recall20=round(r20, 6), ndcg100=round(n100, 6),
              density=info["density"], primal_residual=info["primal_residual"][-1],
              dual_residual=info["dual_residual"][-1], seconds=round(time.perf_counter() - t0, 1), source=src), out)
    if name == "default":
      golden = dict(default=dict(params=p, recall20=r20, ndcg100=n100, density=info["density"]))
  A64 = ease_util.gram(x, p["l2_reg"])
  P64 = np.linalg.inv(A64)
  B64 = ease_util.weights(P64)
  dist = float(np.abs(cells["ease_limit"][0] - B64).max())
  budget = float(_weights_budget(A64, P64, B64))
  r20, n100 = gu.quality(x, y, S=ease_util.scores(x, B64))
  emit(dict(bench="admm_ease_limit", l2_reg=p["l2_reg"], rho=p["rho"], iterations=p["num_iterations"],
            truncation_distance=dist, max_abs_ease=float(np.abs(B64).max()), ease_weights_budget=budget,
            ease_recall20=round(r20, 6), ease_ndcg100=round(n100, 6), source=src), out)
  golden["ease_limit"] = dict(l2_reg=p["l2_reg"], rho=p["rho"], num_iterations=p["num_iterations"],
                              truncation_distance=dist, ease_weights_budget=budget)
  with open(GOLDEN, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")


# ------------------------------------------------------------------ the GPU runs
def gemm_rates(out):
  import torch
  from recoder_amd import admm
  for n in (7915, 20108):
    g = torch.Generator(device="cuda").manual_seed(n)
    P, M = (torch.rand(n, n, device="cuda", generator=g) - 0.5 for _ in range(2))
    T = torch.empty(n, n, device="cuda")
    ms = event_ms(lambda: admm.gemm(P, M, T, 2.0, -3.0, E=P), 3)
    tf = 2.0 * n ** 3 / (ms * 1e-3) / 1e12
    rec = dict(bench="admm_gemm", n=n, kernel_ms=ms, kernel_tf=tf, kernel_share_of_f32_peak=tf / F32_MATRIX_PEAK_TF,
               device=torch.cuda.get_device_name(0))
    tms = guarded(lambda: event_ms(lambda: torch.mm(P, M, out=T), 3))
    if tms is not None:
      rec.update(torch_mm_ms=tms, torch_mm_tf=2.0 * n ** 3 / (tms * 1e-3) / 1e12, kernel_speedup_vs_torch=tms / ms)
    emit(rec, out)
    del P, M, T
    torch.cuda.empty_cache()


def small_fit(out):
  from recoder_amd import admm, als
  from tests import admm_util as au
  X = au.zipf_matrix(600, 257, seed=0)
  for nonneg in (False, True):
    C64, i64 = au.fit(X, 2.0, 50.0, 100.0, 30, nonneg)
    C32, _ = au.fit(X, 2.0, 50.0, 100.0, 30, nonneg, dtype=np.float32)
    C, _ = admm.fit(als.csr_pair(X, 600, 257, "cuda"), 2.0, 50.0, 100.0, 30, nonneg)
    e32 = float(np.abs(C32 - C64).max())
    V = i64["V"] if nonneg else np.abs(i64["V"])
    keep = np.abs(V - 0.02) > e32
    scale = float(np.abs(C64).max())
    emit(dict(bench="admm_small", n=257, nonneg=nonneg, iterations=30, kernels_error=float(
        np.abs(C.cpu().numpy() - C64)[keep].max()) / scale, f32_numpy_error=e32 / scale,
        left_out=float(1.0 - keep.mean())), out)


def _metrics(rec, x, y, ks=(20, 100)):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  metrics = [Recall(k=20, normalize=True), Recall(k=50, normalize=True), NDCG(k=100)]
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100, metrics=metrics, batch_size=B)
  return {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}


def grid(x, y, out):
  """Every cell through the kernels; one State per (l2, rho) (the Gram and the inverse do not depend on l1 or the
  sign), its C the model's own parameter, read by ``Recoder.evaluate`` at the iterations of READ_AT."""
  import torch
  from recoder_amd import admm, als
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import AdmmSlimModel
  rec = Recoder(model=AdmmSlimModel())
  rec.train_admm_slim(RecommendationDataset(x), num_iterations=1)          # (allocates the model and its plumbing)
  W = rec.model.item_weights.data
  pair = als.csr_pair(x, x.shape[0], x.shape[1], W.device)
  n = x.shape[1]
  for l2 in L2S:
    for rho in RHOS:
      st = admm.State(pair, l2, rho, out=W)
      for l1 in L1S:
        for nonneg in (True, False):
          st.restart()
          sums = []
          for it in range(1, max(READ_AT) + 1):
            sums.append(st.iterate(l1 / rho, nonneg))
            if it in READ_AT:
              rec._weights_written()
              got = _metrics(rec, x, y)
              s = torch.stack(sums).cpu().numpy()
              primal, dual = admm.residuals(s, rho)
              emit(dict(bench="admm_quality", l1_reg=l1, l2_reg=l2, rho=rho, iterations=it, nonneg=nonneg,
                        recall20=round(got["Recall@20"], 6), recall50=round(got["Recall@50"], 6),
                        ndcg100=round(got["NDCG@100"], 6), density=float(s[-1, 2]) / (n * n),
                        primal_residual=primal[-1], dual_residual=dual[-1], source="kernels, MI355X"), out)
      admm.ease.raise_on_status(st.status)
      del st
      torch.cuda.empty_cache()
  return rec


def defaults(rec, x, y, out):
  import torch
  from recoder_amd import admm, als
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  ds = RecommendationDataset(x)
  rec.model.load_model_params(type(rec.model)().model_params())
  rec.train_admm_slim(ds)
  info = rec.train_admm_slim(ds)
  o = dict(bench="admm", data="slice", users=int(x.shape[0]), device=torch.cuda.get_device_name(0))
  o.update({k: info[k] for k in ("n", "nnz", "l1_reg", "l2_reg", "rho", "nonneg", "iterations", "density", "gram_ms",
                                 "inverse_ms", "admm_ms")})
  o.update(primal_residual=info["primal_residual"][-1], dual_residual=info["dual_residual"][-1],
           ms_per_iteration=info["admm_ms"] / info["iterations"])
  # the two halves of an iteration on a state of their own (the values do not change their time)
  st = admm.State(als.csr_pair(x, x.shape[0], x.shape[1], "cuda"), info["l2_reg"], info["rho"])
  theta = info["l1_reg"] / info["rho"]
  for _ in range(3):
    st.iterate(theta, info["nonneg"])
  o["gemm_ms"] = event_ms(lambda: admm.gemm(st.P, st.M, st.T, alpha=st.rho, beta=-st.kappa, E=st.P), 5)
  o["update_ms"] = event_ms(lambda: admm.admm_update(st.T, st.P, st.C, st.U, st.M, theta, info["nonneg"], st.gamma,
                                                     st.row_primal, st.row_dual, st.row_nnz), 5)
  o["update_gb_per_s"] = 7 * 4.0 * st.n * st.n / (o["update_ms"] * 1e-3) / 1e9      # (reads T, P, C, U; writes C, U, M)
  del st
  users = np.arange(min(B, x.shape[0]))
  inp = UsersInteractions(users, x[users])
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  reps = 10
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  dt = (time.perf_counter() - t0) / reps
  o.update(serve_batch=len(users), serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt)
  o.update(_metrics(rec, x, y))
  emit(o, out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return cpu_grid(args.out or os.path.join(ROOT, "profiles", "admm_quality.jsonl"))
  if not args.quality:
    ap.error("one of --quality (on the GPU) or --cpu-grid")
  out = args.out or os.path.join(ROOT, "profiles", "admm_bench.jsonl")
  x, y = load("slice")
  gemm_rates(out)
  small_fit(out)
  rec = grid(x, y, out)
  defaults(rec, x, y, out)


if __name__ == "__main__":
  main()
