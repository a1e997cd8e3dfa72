"""Constrained serving on an MI355X: what Recoder.recommend_filtered costs ("Constrained serving").

    python tools/serve_bench.py [--out profiles/serve_bench.jsonl] [--batch 500] [--h 64] [--k 20]

On the ML-20M slice (tests/golden/real_ml20m_slice.npz) and on the C2-shaped matrix (synthetic.ml20m_like), a
MatrixFactorization with random tables at h = 64 and batches of 500 users; one JSON line per measurement, each the
minimum of five timed loops after a warm-up with the largest beside it (ms per call, wall clock around a device
synchronise: the calls end in a copy to the host):

    recommend_array            against recommend_filtered with default filters: the mask build and the padding
    deny10                     recommend_filtered with 10 % of the catalogue in deny_items
    pairs / mask / torch @ C   rerank of C = 100, 1000, 8192 candidates a user on either route, and the same reranking in
                               torch ops (gather of the candidate rows, bmm, masked topk)
    kernel_*                   rk_als_serve_mask, rk_als_pair_scores and rk_als_pairs_topk alone (HIP events)
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

CANDIDATES = (100, 1000, 8192)


def wall(fn, loops=5, reps=5):
  """(min, max) ms per call over ``loops`` timed loops of ``reps`` calls, after a warm-up loop."""
  import torch
  for _ in range(2):
    fn()
  ms = []
  for _ in range(loops):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
      fn()
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3 / reps)
  return min(ms), max(ms)


def events(fn, loops=5, reps=20):
  import torch
  for _ in range(2):
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


def candidates(B, n_items, c, rng):
  idx = np.concatenate([np.sort(rng.choice(n_items, size=c, replace=False)) for _ in range(B)])
  return sp.csr_matrix((np.ones(B * c, np.float32), idx.astype(np.int32), np.arange(B + 1, dtype=np.int64) * c),
                       shape=(B, n_items))


def torch_rerank(z, Y, b, cand_idx, k):
  """The same reranking in torch ops: gather [B, C, h], bmm, topk; ids by gather."""
  import torch
  rows = Y[cand_idx]                                              # [B, C, h]
  s = torch.bmm(rows, z[:, :, None])[:, :, 0] + b[cand_idx]
  top = torch.topk(s, k, dim=1, sorted=True)[1]
  return torch.gather(cand_idx, 1, top).cpu()


def bench(name, matrix, args, out):
  import torch
  from recoder_amd import serve
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  n_users, n_items = matrix.shape
  B, h, k = args.batch, args.h, args.k
  rec = Recoder(model=MatrixFactorization(h), use_cuda=True, optimizer_type="adam", loss="mse",
                loss_params={"confidence": 10.0}, num_items=n_items, num_users=n_users)
  rec._Recoder__init_model()
  rec._sync_ranges()
  rng = np.random.RandomState(0)
  users = np.sort(rng.choice(n_users, size=B, replace=False))
  ui = UsersInteractions(users, matrix[users])

  def emit(what, mn, mx, **kw):
    line = dict(data=name, n_items=n_items, B=B, h=h, k=k, what=what, ms_min=round(mn, 4), ms_max=round(mx, 4), **kw)
    print(json.dumps(line), flush=True)
    out.write(json.dumps(line) + "\n")

  emit("recommend_array", *wall(lambda: rec.recommend_array(ui, k)))
  emit("recommend_filtered_default", *wall(lambda: rec.recommend_filtered(ui, k)))
  deny = rng.choice(n_items, size=n_items // 10, replace=False)
  emit("recommend_filtered_deny10", *wall(lambda: rec.recommend_filtered(ui, k, deny_items=deny)))
  Y, b = rec.model.item_embedding_layer.weight.data, rec.model.bias.data
  z = rec.model.user_embedding_layer.weight.data[torch.as_tensor(users, device=Y.device)].contiguous()
  for c in CANDIDATES:
    if c > n_items:
      continue
    cand = candidates(B, n_items, c, rng)
    for route in ("pairs", "mask"):
      emit("rerank_" + route, *wall(lambda: rec.rerank(ui, cand, k, route=route)), candidates=c)
    cand_idx = torch.as_tensor(cand.indices.reshape(B, c).astype(np.int64), device=Y.device)
    emit("rerank_torch", *wall(lambda: torch_rerank(z, Y, b, cand_idx, k)), candidates=c)
    indptr = torch.as_tensor(cand.indptr.astype(np.int64), device=Y.device)
    ids = torch.as_tensor(cand.indices.astype(np.int32), device=Y.device)
    scores = serve.pair_scores(indptr, ids, c, z, Y, b)
    emit("kernel_pair_scores", *events(lambda: serve.pair_scores(indptr, ids, c, z, Y, b, out=scores)), candidates=c)
    emit("kernel_pairs_topk", *events(lambda: serve.pairs_topk(indptr, ids, scores, c, n_items, k)), candidates=c)
  filters = serve.Filters(B, n_items, True, deny_items=deny)
  rec._input_block(ui)
  dcsr = rec._eval_ws["dcsr"]
  emit("kernel_serve_mask", *events(lambda: serve.build_mask(filters, dcsr, Y.device)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serve_bench.jsonl"))
  ap.add_argument("--batch", type=int, default=500)
  ap.add_argument("--h", type=int, default=64)
  ap.add_argument("--k", type=int, default=20)
  args = ap.parse_args()
  from recoder_amd import synthetic
  from tests import svd_util
  with open(args.out, "w") as out:
    bench("ml20m_slice", svd_util.load_slice()[0], args, out)
    bench("c2", synthetic.ml20m_like(), args, out)


if __name__ == "__main__":
  main()
