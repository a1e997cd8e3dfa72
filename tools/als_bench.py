#!/usr/bin/env python
"""Implicit-feedback ALS throughput (recoder_amd/als.py, include/recoder_als.h), one JSON line per
(dataset, h):

    python tools/als_bench.py [--quick] [--no-torch] [--iters N] [--out FILE]

  hip     ms per iteration of als.fit (end to end, HIP events), and the per-kernel split of one
          instrumented iteration: gram (X and Y), solve (users, items), objective
  gather  the bytes one gather pass of a half-step moves (nnz x h x 4) over that half-step's solve
          time, and the share of entries in rows too long for the LDS stash (those re-read every CG step)
  L       the objective after 1 and 5 iterations
  torch   the same algorithm restated in torch ops on the GPU (torch.mm Gram; gathered factor rows,
          batched row-wise CG with index_add for the sparse terms): ms per iteration, the speed-up of
          the HIP path, and the relative difference of the objectives after the same iterations

Data: C2 = synthetic.ml20m_like (116 677 x 20 108, 6.32 M nnz) and msd_like (471 355 x 41 140,
21.7 M nnz); h in {64, 128, 200}; alpha = 10, reg = 100, 3 CG steps, xavier init from seed 0.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_util import emit  # noqa: E402

ALPHA, REG, CG = 10.0, 100.0, 3


def init_tables(n_users, n_items, h, dev):
  torch.manual_seed(0)
  X = torch.empty(n_users, h)
  Y = torch.empty(n_items, h)
  torch.nn.init.xavier_uniform_(X)
  torch.nn.init.xavier_uniform_(Y)
  return X.to(dev), Y.to(dev), torch.zeros(n_items, device=dev)


def stash_rows(h):
  """rows of h floats rk_als_solve stashes per wave (csrc/als/solve.h: 64 KB per workgroup of 4 waves)."""
  g = h * h if h * h * 4 <= 32 * 1024 else 0
  return (64 * 1024 // 4 - g) // 4 // h


class Ev:
  def __init__(self):
    self.t = {}

  def time(self, name, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    self.t.setdefault(name, []).append((a, b))
    return r

  def ms(self):
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.t.items()}


def instrumented_iteration(als, X, Y, b, uc, ic):
  ev = Ev()
  gws = torch.empty(max(als._als_lib.load().rk_als_gram_workspace_bytes(X.shape[0], X.shape[1]),
                        als._als_lib.load().rk_als_gram_workspace_bytes(Y.shape[0], Y.shape[1])),
                    dtype=torch.uint8, device=X.device)
  out = torch.zeros(1, dtype=torch.float64, device=X.device)
  Gy, cy = ev.time("gram", lambda: als.gram(Y, REG, b, gws))
  ev.time("solve_users", lambda: als.solve(uc, Y, Gy, cy, X, ALPHA, CG, col_bias=b))
  Gx, sx = ev.time("gram", lambda: als.gram(X, REG, None, gws))
  ev.time("solve_items", lambda: als.solve(ic, X, Gx, sx, Y, ALPHA, CG, row_bias=b))
  Gy, cy = ev.time("gram", lambda: als.gram(Y, REG, b, gws))
  ev.time("objective", lambda: als.objective(uc, X, Y, b, ALPHA, REG, Gx, sx, Gy, cy, out))
  return ev.ms()


# ------------------------------------------------------------- torch restatement
class TorchSide:
  """One side's CSR as COO tensors for the torch-ops restatement."""

  def __init__(self, c):
    n = c.shape[0]
    deg = c.indptr[1:] - c.indptr[:-1]
    self.n = n
    self.row = torch.repeat_interleave(torch.arange(n, device=c.indptr.device), deg)
    self.col = c.indices[:c.nnz].long()
    self.val = c.data[:c.nnz] if c.data is not None else torch.ones(c.nnz, device=c.indptr.device)
    self.a = torch.where(self.val > 0, torch.full_like(self.val, ALPHA), torch.zeros_like(self.val))


def torch_half_step(side, F, X, b, user_side):
  h = F.shape[1]
  G = torch.mm(F.t(), F) + REG * torch.eye(h, device=F.device)
  if user_side:
    v = torch.mv(F.t(), b)
    const = -v.expand(side.n, h)
    bsel = b[side.col]
  else:
    v = F.sum(0)
    const = -b[:, None] * v[None, :]
    bsel = b[side.row]
  Fc = F[side.col]                                        # gathered once per half-step
  coef = (1 + side.a) * side.val - side.a * bsel
  rhs = const.clone().index_add_(0, side.row, coef[:, None] * Fc)

  def matvec(P):
    d = (Fc * P[side.row]).sum(1) * side.a
    return torch.mm(P, G).index_add_(0, side.row, d[:, None] * Fc)

  x = X.clone()
  r = rhs - matvec(x)
  p = r.clone()
  rs = (r * r).sum(1)
  active = rs > 0
  for _ in range(CG):
    q = matvec(p)
    pq = (p * q).sum(1)
    active = active & (pq > 0)
    al = torch.where(active, rs / torch.where(active, pq, torch.ones_like(pq)), torch.zeros_like(pq))
    x += al[:, None] * p
    r -= al[:, None] * q
    rsn = (r * r).sum(1)
    beta = torch.where(active, rsn / torch.where(active, rs, torch.ones_like(rs)), torch.zeros_like(rs))
    p = torch.where(active[:, None], r + beta[:, None] * p, p)
    rs = torch.where(active, rsn, rs)
    active = active & (rs > 0)
  X.copy_(x)


def torch_objective(us, X, Y, b):
  s = (X[us.row] * Y[us.col]).sum(1) + b[us.col]
  s64, v64 = s.double(), us.val.double()
  w = 1 + us.a.double()
  sparse = (w * (v64 - s64) ** 2 - s64 ** 2).sum()
  X64, Y64, b64 = X.double(), Y.double(), b.double()
  dense = (torch.mm(X64.t(), X64) * torch.mm(Y64.t(), Y64)).sum() + 2 * X64.sum(0) @ (Y64.t() @ b64) \
      + X.shape[0] * (b64 ** 2).sum()
  return float(sparse + dense + REG * ((X64 ** 2).sum() + (Y64 ** 2).sum()))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="C2 at h = 64 only")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--iters", type=int, default=5)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from recoder_amd import als, synthetic
  dev = torch.device("cuda")
  sets = [("c2", synthetic.ml20m_like)] + ([] if args.quick else [("msd", synthetic.msd_like)])
  hs = [64] if args.quick else [64, 128, 200]
  for name, gen in sets:
    t0 = time.perf_counter()
    m = gen()
    uc, ic = als.csr_pair(m, m.shape[0], m.shape[1], dev)
    prep_s = time.perf_counter() - t0
    deg_u = np.diff(m.indptr)
    deg_i = np.bincount(m.indices, minlength=m.shape[1])
    for h in hs:
      rec = {"bench": "als", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
             "alpha": ALPHA, "reg": REG, "cg_steps": CG, "host_prep_s": round(prep_s, 2)}
      # warm-up (code objects), then the timed fit from the same init
      X, Y, b = init_tables(m.shape[0], m.shape[1], h, dev)
      als.fit(X, Y, b, uc, ic, ALPHA, REG, CG, 1)
      X, Y, b = init_tables(m.shape[0], m.shape[1], h, dev)
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      hist = als.fit(X, Y, b, uc, ic, ALPHA, REG, CG, args.iters)
      e1.record()
      torch.cuda.synchronize()
      rec["hip_ms_per_iter"] = round(e0.elapsed_time(e1) / args.iters, 3)
      rec["L_iter1"], rec["L_iter5"] = hist[0], hist[min(4, len(hist) - 1)]
      split = instrumented_iteration(als, X, Y, b, uc, ic)
      rec["split_ms"] = {k: round(v, 3) for k, v in split.items()}
      st = stash_rows(h)
      for side, deg, t in (("users", deg_u, split["solve_users"]), ("items", deg_i, split["solve_items"])):
        gb = float(m.nnz) * h * 4
        rec["gather_TBps_" + side] = round(gb / (t * 1e-3) / 1e12, 3)
        rec["streamed_share_" + side] = round(float(deg[deg > st].sum()) / m.nnz, 4)
      rec["stash_rows_per_wave"] = st
      if not args.no_torch:
        us, its = TorchSide(uc), TorchSide(ic)
        X, Y, b = init_tables(m.shape[0], m.shape[1], h, dev)
        torch_half_step(us, Y, X, b, True)                 # warm-up
        X, Y, b = init_tables(m.shape[0], m.shape[1], h, dev)
        torch.cuda.synchronize()
        t_hist = []
        e0.record()
        for it in range(args.iters):
          torch_half_step(us, Y, X, b, True)
          torch_half_step(its, X, Y, b, False)
          if it in (0, 4):
            e1.record()
            torch.cuda.synchronize()
            t_hist.append((e0.elapsed_time(e1), torch_objective(us, X, Y, b)))
            e0.record()
        e1.record()
        torch.cuda.synchronize()
        ms = t_hist[0][0] + (t_hist[1][0] if len(t_hist) > 1 else 0) + e0.elapsed_time(e1)
        rec["torch_ms_per_iter"] = round(ms / args.iters, 3)
        rec["speedup_vs_torch"] = round(rec["torch_ms_per_iter"] / rec["hip_ms_per_iter"], 2)
        rec["torch_L_iter1"] = t_hist[0][1]
        rec["torch_L_iter5"] = t_hist[-1][1]
        rec["L_rel_diff_iter1"] = abs(rec["L_iter1"] - t_hist[0][1]) / abs(t_hist[0][1])
        rec["L_rel_diff_iter5"] = abs(rec["L_iter5"] - t_hist[-1][1]) / abs(t_hist[-1][1])
        del us, its
        torch.cuda.empty_cache()
      emit(rec, args.out)


if __name__ == "__main__":
  main()
