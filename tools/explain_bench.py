"""Explanations (recoder_amd/explain.py: rk_ease_explain, rk_slim_explain, rk_als_explain): (user, target) pairs per
second on the GPU, each route beside the same result in torch ops, and the f32 restatement's error against float64.

  python tools/explain_bench.py            GPU -> profiles/explain_bench.jsonl
      J = 20 targets a user (drawn uniformly), m = 5, batches of 500 users, the minimum of 5 timed loops with the largest
      beside it, on the last 2 000 users of tests/golden/real_ml20m_slice.npz and on the C2-shaped matrix
      (synthetic.ml20m_like):
        dense   rk_ease_explain on a random dense W; torch: W[cols, j] gathers over the padded histories plus topk
        lists   rk_slim_explain on random ascending lists of K = 100, both layouts (no torch comparator: the dense one
                on the lists' matrix is the same work as above)
        mf      rk_als_explain at h = 64 and 128; torch: A by einsum over the padded histories, torch.linalg.cholesky,
                cholesky_solve against the J targets' rows, an einsum for the contributions, topk
      The first record holds the error of tests/explain_util.py's f32 restatement against float64 on the cases of
      tests/test_explain.py (CPU): the kernels equal that restatement bit for bit, so it is the feature's error.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

J, M, BATCH, K = 20, 5, 500, 100


def timed(fn, loops=5):
  import torch
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(loops):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
  return min(times), max(times)


def errors():
  from tests import explain_util as U
  rec = {"bench": "explain_error", "item_total_rel": U.item_error()}
  for h in U.HS:
    rec["mf_h%d_rel" % h] = max(U.mf_error(h, vi) for vi in range(len(U.VARIANTS)))
  return rec


def padded(c, width, dev):
  """(cols int64 [B, width], live f32 [B, width]) of an AlsCSR batch."""
  import torch
  B = c.shape[0]
  lens = (c.indptr[1:] - c.indptr[:-1])
  pos = torch.arange(width, device=dev)[None, :]
  live = pos < lens[:, None]
  idx = (c.indptr[:-1, None] + pos).clamp(max=max(c.nnz - 1, 0))
  return c.indices[idx].to(torch.int64) * live, live.to(torch.float32)


def torch_dense(c, W, items, width, dev):
  import torch
  cols, live = padded(c, width, dev)
  w = W[cols[:, :, None], items[:, None, :]]                 # [B, width, J]
  contrib = torch.where(live[:, :, None] > 0, w, torch.full_like(w, float("-inf")))
  top = torch.topk(contrib, min(M, width), dim=1)
  return top, (w * live[:, :, None]).sum(1)


def torch_mf(c, Y, G, v, b, alpha, items, width, dev):
  import torch
  cols, live = padded(c, width, dev)
  y = Y[cols] * live[:, :, None]
  A = G[None] + alpha * torch.einsum("bek,bel->bkl", y, y)
  coef = ((1 + alpha) - alpha * b[cols]) * live
  L = torch.linalg.cholesky(A)
  z = torch.cholesky_solve(Y[items].transpose(1, 2), L)      # [B, h, J]
  contrib = coef[:, :, None] * torch.einsum("bek,bkj->bej", y, z)
  base = b[items] - torch.einsum("bkj,k->bj", z, v)
  masked = torch.where(live[:, :, None] > 0, contrib, torch.full_like(contrib, float("-inf")))
  return torch.topk(masked, min(M, width), dim=1), base + contrib.sum(1)


def bench(out):
  import torch
  from recoder_amd import als, explain, synthetic
  from tests import svd_util
  dev = torch.device("cuda")
  rows = [errors()]
  print(json.dumps(rows[0]), flush=True)
  x, _ = svd_util.load_slice()
  for name, m in (("slice", x[-2000:]), ("c2", synthetic.ml20m_like()[:2000])):
    m = sp.csr_matrix(m)
    m.data[:] = 1.0
    n = m.shape[1]
    g = torch.Generator(device="cpu").manual_seed(n)
    los = list(range(0, m.shape[0], BATCH))
    batches = [als.AlsCSR(m[lo:lo + BATCH], dev) for lo in los]
    widths = [max(int(np.diff(m[lo:lo + BATCH].indptr).max()), 1) for lo in los]
    items = [torch.randint(0, n, (c.shape[0], J), generator=g).to(dev) for c in batches]
    pairs = sum(c.shape[0] for c in batches) * J
    base = {"data": name, "users": m.shape[0], "items": n, "nnz": int(m.nnz), "J": J, "m": M, "batch": BATCH}

    def record(route, fns, **extra):
      rec = dict(base, bench="explain", route=route, **extra)
      for key, fn in fns:
        lo, hi = timed(fn)
        rec[key + "_ms"] = round(lo, 4)
        rec[key + "_ms_max"] = round(hi, 4)
        rec[key + "_pairs_per_s"] = round(pairs / (lo * 1e-3))
      rows.append(rec)
      print(json.dumps(rec), flush=True)

    W = torch.randn(n, n, generator=g).to(dev)
    record("dense", (("kernel", lambda: [explain.dense(c, W, it, M) for c, it in zip(batches, items)]),
                     ("torch", lambda: [torch_dense(c, W, it, w, dev) for c, it, w in zip(batches, items, widths)])))
    del W
    ids = torch.sort(torch.rand(n, n, device=dev).topk(K, dim=1).indices.to(torch.int32), dim=1).values.contiguous()
    lw = torch.randn(n, K, device=dev)
    count = torch.full((n,), K, dtype=torch.int32, device=dev)
    for columns in (True, False):
      record("lists", (("kernel", lambda: [explain.lists(c, ids, lw, count, columns, it, M)
                                           for c, it in zip(batches, items)]),), K=K, columns=columns)
    del ids
    for h in (64, 128):
      Y = (0.1 * torch.randn(n, h, generator=g)).to(dev)
      b = torch.zeros(n, device=dev)
      G, v = als.gram(Y, 10.0, b)
      record("mf", (("kernel", lambda: [explain.folded(c, Y, G, v, b, 10.0, it, M) for c, it in zip(batches, items)]),
                    ("torch", lambda: [torch_mf(c, Y, G, v, b, 10.0, it, w, dev)
                                       for c, it, w in zip(batches, items, widths)])), h=h)
  with open(out, "w") as f:
    for r in rows:
      f.write(json.dumps(r) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_bench.jsonl"))
  bench(ap.parse_args().out)


if __name__ == "__main__":
  main()
