"""iALS++ (recoder_amd/ials.py, rk_als_ials_*): quality on the CPU, time on the GPU.

  python tools/ials_bench.py --cpu-grid [--jobs N]     float64, no GPU -> profiles/ials_quality.jsonl
      tests/golden/real_ml20m_slice.npz: the float64 fit of tests/ials_util.py on the training part, Recall@20 and
      NDCG@100 on the held-out part after 8 and after 16 sweeps, blocks of 32, init_std 0.1, seed 0, over h in
      {64, 256}, nu in {0, 0.5, 1}, alpha0 in ALPHAS and the reg values of REGS[nu] (reg scales with
      (count + alpha0 n)^nu, so each nu has its own decade range).  h = 256 runs the alpha0 = 0.1 column only.  Also
      writes tests/golden/ials_slice.json: the default cell's L history and figures.
  python tools/ials_bench.py --quality                 GPU -> profiles/ials_bench.jsonl
      ms per sweep and per kernel (predict, the panels, the user and item block steps, the objective with its Grams)
      at h in {64, 512, 2048} with blocks of 64, the minimum of 5 timed loops after a warm-up with the largest beside
      it, on the slice and on the C2-shaped matrix (synthetic.ml20m_like); the same sweep in torch ops (slice only: the
      padded [rows, width, k] gathers of the C2 item side, 20 108 rows x 106 584 entries x 64 floats, are 0.5 TB); a
      train_als iteration (rk_als_solve at cg_steps = 3 with its Grams) at h = 512; and, to place the dense term
      alpha0 P x, the dense [n, h] x [h, k] product of a side (torch.matmul) beside the block step that computes it
      in the kernel.
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHAS = (0.03, 0.1, 0.3)
REGS = {0.0: (1.0, 3.0, 10.0, 30.0), 0.5: (0.03, 0.1, 0.3, 1.0), 1.0: (0.001, 0.003, 0.01, 0.03)}
GRID_BLOCK, GRID_STD, GRID_SEED = 32, 0.1, 0
DEFAULT_CELL = {"h": 64, "nu": 1.0, "alpha0": 0.03, "reg": 0.03}


def cells():
  for h in (64, 256):
    for nu in (0.0, 0.5, 1.0):
      for alpha0 in (ALPHAS if h == 64 else (0.1,)):
        for reg in REGS[nu]:
          yield {"h": h, "nu": nu, "alpha0": alpha0, "reg": reg}


def run_cell(cell):
  from tests import ials_util as U
  x, y = U.load_slice()
  x = sp.csr_matrix(x)
  x.data[:] = 1.0
  X0, Y0 = U.init_tables(x.shape[0], x.shape[1], cell["h"], GRID_STD, GRID_SEED)
  figures = {}

  def after(s, X, Y):
    if s + 1 in (8, 16):
      lists = U.top_k(X @ Y.T, x, 100)
      figures[s + 1] = (U.recall_at(lists, y, 20), U.ndcg_at(lists, y, 100))
  t0 = time.time()
  _, _, hist = U.fit(x, X0, Y0, cell["alpha0"], cell["reg"], cell["nu"], GRID_BLOCK, 16, fast=True, after_sweep=after)
  rec = dict(cell, bench="ials_quality", block=GRID_BLOCK, init_std=GRID_STD, seed=GRID_SEED, users=x.shape[0],
             items=x.shape[1], nnz=int(x.nnz), L=hist, seconds=round(time.time() - t0, 1))
  for s, (r, n) in figures.items():
    rec["recall20_s%d" % s], rec["ndcg100_s%d" % s] = round(r, 5), round(n, 5)
  return rec


def cpu_grid(out, jobs):
  with multiprocessing.Pool(jobs) as pool:
    rows = []
    for rec in pool.imap(run_cell, list(cells())):
      rows.append(rec)
      print(json.dumps({k: v for k, v in rec.items() if k != "L"}), flush=True)
  with open(out, "w") as f:
    for r in rows:
      f.write(json.dumps(r) + "\n")
  d = next(r for r in rows if all(r[k] == v for k, v in DEFAULT_CELL.items()))
  from tests import ials_util as U
  with open(U.GOLDEN, "w") as f:
    json.dump({k: d[k] for k in ("h", "nu", "alpha0", "reg", "block", "init_std", "seed", "L", "recall20_s8",
                                 "ndcg100_s8", "recall20_s16", "ndcg100_s16")}, f, indent=1)
    f.write("\n")


# ---------------------------------------------------------------------------------------------------------- GPU
def timed(fn, loops=5, reps=1):
  """(min, max) ms per call over ``loops`` timed loops of ``reps`` calls, after a warm-up loop."""
  import torch
  fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ms = []
  for _ in range(loops):
    e0.record()
    for _ in range(reps):
      fn()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1) / reps)
  return min(ms), max(ms)


def torch_block(indptr, indices, perm, F, X, reg, alpha0, p0, k, cache, chunk=2048):
  """The block step in torch ops, rows padded to the chunk's longest row."""
  import torch
  n = indptr.shape[0] - 1
  Fp = F[:, p0:p0 + k]
  P = Fp.T @ F
  eye = torch.eye(k, device=F.device)
  for lo in range(0, n, chunk):
    hi = min(n, lo + chunk)
    lens = indptr[lo + 1:hi + 1] - indptr[lo:hi]
    width = int(lens.max().item())
    if width == 0:
      width = 1
    pos = torch.arange(width, device=F.device)[None, :]
    live = pos < lens[:, None]
    idx = (indptr[lo:hi, None] + pos).clamp(max=indices.shape[0] - 1)
    cpos = idx if perm is None else perm[idx]
    y = Fp[indices[idx].long()] * live[:, :, None]
    A = torch.einsum("bek,bel->bkl", y, y) + alpha0 * P[:, p0:p0 + k][None] + reg[lo:hi, None, None] * eye[None]
    g = torch.einsum("be,bek->bk", (cache[cpos] - 1.0) * live, y) + alpha0 * (X[lo:hi] @ P.T) + \
        reg[lo:hi, None] * X[lo:hi, p0:p0 + k]
    delta = torch.cholesky_solve(g[:, :, None], torch.linalg.cholesky(A))[:, :, 0]
    X[lo:hi, p0:p0 + k] -= delta
    cache[cpos[live]] -= torch.einsum("bk,bek->be", delta, y)[live]


def quality(out, hs, sets):
  import torch
  from recoder_amd import als, ials, synthetic
  from tests import ials_util as U
  dev = torch.device("cuda")
  data = {"slice": lambda: U.load_slice()[0], "c2": synthetic.ml20m_like}
  rows = []
  for name in sets:
    m = sp.csr_matrix(data[name]())
    m.data[:] = 1.0
    n_users, n_items = m.shape
    pair = ials.Pair(m, n_users, n_items, dev)
    alpha0, reg, nu, k = ials.DEFAULT_ALPHA0, ials.DEFAULT_REG, 1.0, 64
    lam64, mu64 = ials.regularisers(pair.row_counts, pair.col_counts, alpha0, reg, nu)
    lam, mu = (torch.from_numpy(v.astype(np.float32)).to(dev) for v in (lam64, mu64))
    for h in hs:
      g = torch.Generator(device="cpu").manual_seed(h)
      X = (0.1 / h ** 0.5 * torch.randn(n_users, h, generator=g)).to(dev)
      Y = (0.1 / h ** 0.5 * torch.randn(n_items, h, generator=g)).to(dev)
      kk = min(k, h)
      cache = torch.empty(max(pair.nnz, 1), device=dev)
      status = torch.zeros(1, dtype=torch.int32, device=dev)
      P = torch.empty(kk, h, device=dev)
      ws = ials.panel_workspace(max(n_users, n_items), h, kk, dev)
      outv = torch.zeros(1, dtype=torch.float64, device=dev)
      nblk = len(ials.blocks(h, kk))
      rec = {"bench": "ials", "data": name, "users": n_users, "items": n_items, "nnz": pair.nnz, "h": h, "block": kk,
             "blocks": nblk, "longest_user_row": int(pair.row_counts.max()), "longest_item_row": int(pair.col_counts.max())}

      def put(key, fn, scale=1.0):
        lo, hi = timed(fn)
        rec[key + "_ms"], rec[key + "_ms_max"] = round(lo * scale, 4), round(hi * scale, 4)
      ials.predict(pair.ucsr, X, Y, cache)
      put("sweep", lambda: ials.sweep(X, Y, pair, lam, mu, alpha0, kk, cache, status, P, ws))
      put("predict", lambda: ials.predict(pair.ucsr, X, Y, cache))
      put("panel_users", lambda: ials.gram_panel(X, 0, kk, P, ws))
      put("panel_items", lambda: ials.gram_panel(Y, 0, kk, P, ws))
      ials.gram_panel(Y, 0, kk, P, ws)
      put("block_users", lambda: ials.block(pair.ucsr, None, Y, X, P, lam, alpha0, 0, kk, cache, status))
      ials.gram_panel(X, 0, kk, P, ws)
      put("block_items", lambda: ials.block(pair.icsr, pair.perm, X, Y, P, mu, alpha0, 0, kk, cache, status))
      # the alternative placement of the dense term alpha0 P x: one dense [n, h] x [h, k] product a side and block step
      put("dense_product_users", lambda: torch.matmul(X, P.T))
      put("dense_product_items", lambda: torch.matmul(Y, P.T))
      put("objective", lambda: ials.objective(cache, pair.nnz, ials.full_gram(X, kk, None, ws), ials.full_gram(Y, kk, None, ws),
                                              X, lam, Y, mu, alpha0, outv))
      rec["status"] = int(status.item())
      if name == "slice" and h <= 512:
        def torch_sweep():
          c = torch.einsum("eh,eh->e", X[rows_of], Y[pair.ucsr.indices.long()])
          for p0, kb in ials.blocks(h, kk):
            torch_block(pair.ucsr.indptr, pair.ucsr.indices, None, Y, X, lam, alpha0, p0, kb, c)
            torch_block(pair.icsr.indptr, pair.icsr.indices, pair.perm, X, Y, mu, alpha0, p0, kb, c)
        rows_of = torch.repeat_interleave(torch.arange(n_users, device=dev), torch.from_numpy(pair.row_counts).to(dev))
        put("torch_sweep", torch_sweep)
      if h == 512:
        def als_iteration():
          Gy, cy = als.gram(Y, 1.0, bias)
          als.solve(pair.ucsr, Y, Gy, cy, X, 10.0, 3, col_bias=bias)
          Gx, sx = als.gram(X, 1.0, None)
          als.solve(pair.icsr, X, Gx, sx, Y, 10.0, 3, row_bias=bias)
        bias = torch.zeros(n_items, device=dev)
        put("train_als_iteration_cg3", als_iteration)
      rows.append(rec)
      print(json.dumps(rec), flush=True)
      with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--jobs", type=int, default=8)
  ap.add_argument("--hs", default="64,512,2048")
  ap.add_argument("--sets", default="slice,c2")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    cpu_grid(args.out or os.path.join(ROOT, "profiles", "ials_quality.jsonl"), args.jobs)
  if args.quality:
    out = args.out or os.path.join(ROOT, "profiles", "ials_bench.jsonl")
    if os.path.exists(out):
      os.remove(out)
    quality(out, [int(v) for v in args.hs.split(",")], args.sets.split(","))


if __name__ == "__main__":
  main()
