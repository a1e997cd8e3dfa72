#!/usr/bin/env python
"""Recoder.recommend / evaluate throughput at C5's catalogue (1 M items, AE[512]) on one GPU:
the fused form (top-k filter in the decode epilogue, include/recoder_hip.h) against the strip-by-strip
path (RK_EVAL_FUSED=0: decode a 65 536-item strip -> scores -> radix-select top-k -> merge).

    python tools/eval_bench.py [n_items] [h] [k]

Synthetic: 20 000 users x n_items uniform, 100 interactions per user; random-init weights (scores of
an untrained model: a harder case for the sample bound than a trained one, whose scores are peaked).

    python tools/eval_bench.py --metrics [--data slice|c2] [--out profiles/eval_bench.jsonl]

The metric arithmetic on the host (recommend_array + metrics.batch_metrics) against the device path
(_recommend_device + rk_als_rank_metrics, recoder_amd/validation.py) for a MatrixFactorization (h = 64) after one
train_bpr epoch, on the ML-20M slice and the C2-shaped synthetic matrix (a fifth of every row held out as targets):
the metric step alone at B = 500 and over the whole user set for K in {20, 100}, the whole evaluation both ways, and
a train_bpr epoch with and without validation.  Every figure is the minimum of 5 timed loops after a warm-up, the
largest beside it; one JSON line per measurement."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from recoder_amd import synthetic  # noqa: E402
from recoder_amd.data import RecommendationDataset, UsersInteractions  # noqa: E402
from recoder_amd.metrics import Recall  # noqa: E402
from recoder_amd.model import Recoder  # noqa: E402
from recoder_amd.nn import DynamicAutoencoder  # noqa: E402


def main():
  n_items = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
  h = int(sys.argv[2]) if len(sys.argv) > 2 else 512
  k = int(sys.argv[3]) if len(sys.argv) > 3 else 20
  n_users = 20000
  csr = synthetic.uniform(n_users, n_items, 100, seed=5)
  torch.manual_seed(1)
  model = DynamicAutoencoder([h], activation_type="tanh", sparse=True)
  rec = Recoder(model=model, use_cuda=True, optimizer_type="adam", loss="mse")
  # one short epoch on 2 000 users: initialises the engine and moves the weights off their init
  rec.train(RecommendationDataset(csr[:2000]), batch_size=500, lr=1e-3, num_epochs=1, negative_sampling=True)
  print("catalogue %d items, h = %d, k = %d" % (n_items, h, k))
  for B in (500, 2000):
    users = np.arange(2000, 2000 + B)
    ui = UsersInteractions(users=users, interactions_matrix=csr[users])
    res = {}
    for mode in ("fused", "strips"):
      os.environ["RK_EVAL_FUSED"] = "1" if mode == "fused" else "0"
      rec.eval_fused_batches = 0
      out = rec.recommend_array(ui, k)          # warm-up (images, workspaces)
      torch.cuda.synchronize()
      reps = 5
      t0 = time.perf_counter()
      for _ in range(reps):
        out = rec.recommend_array(ui, k)
      torch.cuda.synchronize()
      dt = (time.perf_counter() - t0) / reps
      res[mode] = out
      flops = 2.0 * B * n_items * h
      print("  B = %4d  %-6s  %8.2f ms / batch  %9.0f users/s  %6.1f algorithmic TFLOP/s%s" %
            (B, mode, dt * 1e3, B / dt, flops / dt * 1e-12,
             "  (fused batches: %d of %d)" % (rec.eval_fused_batches, reps + 1) if mode == "fused" else ""))
    print("  B = %4d  identical recommendations: %s" % (B, bool(np.array_equal(res["fused"], res["strips"]))))
  # Recoder.evaluate end to end (host side included: collation of the users' rows, metrics)
  held = csr[2000:6000]
  for mode in ("fused", "strips"):
    os.environ["RK_EVAL_FUSED"] = "1" if mode == "fused" else "0"
    t0 = time.perf_counter()
    r = rec.evaluate(RecommendationDataset(held, held), num_recommendations=k, metrics=[Recall(k)], batch_size=500)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("  Recoder.evaluate 4000 users, batch 500, %-6s: %6.2f s  %7.0f users/s  (%s)" %
          (mode, dt, 4000 / dt, {str(m): float(np.mean(v)) for m, v in r.items()}))


def _min_max_ms(fn, reps=5):
  """(min, max) wall-clock ms of ``reps`` calls of ``fn`` after a warm one, the device drained before each stop."""
  fn()
  torch.cuda.synchronize()
  got = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    got.append((time.perf_counter() - t0) * 1e3)
  return round(min(got), 3), round(max(got), 3)


def _split(x, seed=0, hold=0.2):
  """(input, target): a share ``hold`` of the stored entries held out, drawn per entry."""
  import scipy.sparse as sp
  x = sp.csr_matrix(x)
  keep = np.random.RandomState(seed).rand(x.nnz) >= hold
  coo = x.tocoo()
  mk = lambda m: sp.csr_matrix((np.ones(int(m.sum()), np.float32), (coo.row[m], coo.col[m])), shape=x.shape)
  return mk(keep), mk(~keep)


def metrics_main(argv):
  import argparse
  from recoder_amd import metrics as M, validation
  from recoder_amd.nn import MatrixFactorization
  import bench_util
  ap = argparse.ArgumentParser()
  ap.add_argument("--metrics", action="store_true")
  ap.add_argument("--data", default="slice,c2")
  ap.add_argument("--out", default=None)
  args = ap.parse_args(argv)
  for name in args.data.split(","):
    x, y = bench_util.load(name)
    if y is None:
      x, y = _split(x)
    n_users, n_items = x.shape
    train_ds, val_ds = RecommendationDataset(x), RecommendationDataset(x, y)
    rec = Recoder(model=MatrixFactorization(64), use_cuda=True, optimizer_type="adam", loss="mse")
    rec.train_bpr(train_ds, num_epochs=1, batch_size=4096, seed=0)
    base = dict(tool="eval_bench", data=name, users=n_users, items=n_items, nnz=int(x.nnz), targets=int(y.nnz), h=64)
    for K in (20, 100):
      ms = [M.Recall(K), M.NDCG(K), M.AveragePrecision(K)]
      for B in (500, n_users):
        # the metric step alone: lists of B users already where each path wants them
        ids = np.concatenate([rec.recommend_array(UsersInteractions(np.arange(lo, min(B, lo + 500)),
                                                                      x[lo:min(B, lo + 500)]), K)
                              for lo in range(0, B, 500)])
        tm = y[:B]
        dev, tgt, tab = torch.as_tensor(ids, device="cuda"), M.DeviceTarget(tm, "cuda"), M.DeviceMetricTables(ms, "cuda")
        out = M.device_batch_metrics(dev, K, tgt, ms, tab)
        out = (out[0],) + out[1]
        kernel = bench_util.loop_ms(lambda s: M.device_batch_metrics(dev, K, tgt, ms, tab, out), 20, reps=5)
        host = _min_max_ms(lambda: M.batch_metrics(ids, tm, ms))
        bench_util.emit(dict(base, what="metrics_only", B=B, K=K, metrics=3, kernel_ms_min_max=kernel,
                             host_numpy_ms_min_max=host), args.out)
      # the whole evaluation of one metric over every user, batches of 500: scoring + top-k + metric
      metric = M.Recall(K)

      def host_path():
        total, count = 0.0, 0
        for lo in range(0, n_users, 500):
          rows = np.arange(lo, min(n_users, lo + 500))
          r = M.batch_metrics(rec.recommend_array(UsersInteractions(rows, x[rows]), K), y[rows], [metric])[metric]
          total, count = total + np.nansum(r), count + int(np.sum(~np.isnan(r)))
        return total / count
      val = validation.Validator(rec, val_ds, metric, batch_size=500)
      agree = abs(host_path() - val.score())
      bench_util.emit(dict(base, what="evaluation", K=K, batch=500, host_path_ms_min_max=_min_max_ms(host_path),
                           device_path_ms_min_max=_min_max_ms(val.score), mean_abs_difference=agree), args.out)
      del val
    # a train_bpr epoch with and without validation (Recall@20 after the epoch; the validator's uploads included)
    plain = _min_max_ms(lambda: rec.train_bpr(train_ds, num_epochs=1, batch_size=4096, seed=0))
    watched = _min_max_ms(lambda: rec.train_bpr(train_ds, num_epochs=1, batch_size=4096, seed=0, val_dataset=val_ds,
                                                restore_best=False))
    bench_util.emit(dict(base, what="train_bpr_epoch", batch=4096, plain_ms_min_max=plain,
                         with_validation_ms_min_max=watched), args.out)


if __name__ == "__main__":
  if "--metrics" in sys.argv:
    metrics_main(sys.argv[1:])
  else:
    main()
