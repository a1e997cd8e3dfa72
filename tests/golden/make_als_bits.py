#!/usr/bin/env python
"""The bits of librecoder_als.so: every rk_als_* entry point that launches a kernel, driven directly through
recoder_amd._als_lib on seeded numpy inputs, and the SHA-256 of each output buffer (padding columns included).

    python tests/golden/make_als_bits.py        # writes tests/golden/als_bits.json (needs the GPU)

tests/test_als_bits.py recomputes digests() and compares.  als_bits.json was written at commit e25e53c ("Add UltraGCN:
constraint-loss training for MatrixFactorization"), the last one with csrc/als.hip in one file: this script uses only
names that exist there, so checking that commit out beside this file and running it reproduces the fixture.  It pins the kernels' order of operations: a
digest that moves means a chain was reordered, and the fix belongs in the kernels.  The cases, at every h of HS
(NT = 1, 2, 4, 8; scalar and 16-byte propagate; UltraGCN's 16-, 32- and 64-lane groups), all with padded leading
dimensions:
  one CSR (an empty row, a row of every item but one, an empty row in front of a drawn one, rows of 1024, 1023, 512
    and 511 entries: the long-row thresholds of rk_als_lgcn_propagate and rk_als_solve on either side) for gram,
    solve, objective, both samplers and both propagates
  sorted keys in runs of 1, 4, 5, 63, 64, 65 and 130 and a run of sentinels for apply, both scatters and the
    contrast; rk_als_ugcn_scatter also gets runs of 1023 and 1024 (RK_ALS_UGCN_LONG_KEY)
  rk_als_rank_sample with max_draws 1, 64 and 65 in both modes
The sorts are stable numpy argsorts on the host."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "als_bits.json")

HS = (6, 8, 24, 64, 96, 160, 300)
N_USERS, N_ITEMS, N_ROWS = 24, 1100, 50
T = 300                                                        # slots of the sampled steps
RUNS = (1, 4, 5, 63, 64, 65, 130, 3, 2, 1)                     # 338 entries, then 6 sentinels: n = 344 = 2 * 172
UG_T, UG_E = 96, 26                                            # rk_als_ugcn_scatter: n = 2496
UG_RUNS = RUNS[:7] + (1023, 1024, 40, 30, 20)                  # 2469 entries, then 27 sentinels
SEED, STEP = 11, 4
FILL = 7.0


def csr():
  """indptr (int64), indices (int32, ascending within a row), data (f32 counts, some stored zeros)."""
  rng = np.random.RandomState(1)
  lens = [0, N_ITEMS - 1, 0, 1024, 1023, 512, 511] + list(rng.randint(1, 41, N_USERS - 7))
  rows = [np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in lens]
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  indices = np.concatenate(rows).astype(np.int32)
  return indptr, indices, rng.randint(0, 4, len(indices)).astype(np.float32)


def run_keys(runs, n_rows, sentinels, seed):
  """(keys sorted, order) of entries laid out at random before a stable sort: run r holds the r-th smallest id."""
  rng = np.random.RandomState(seed)
  ids = np.sort(rng.choice(n_rows, len(runs), replace=False))
  unsorted = np.concatenate([np.repeat(ids, runs), np.full(sentinels, n_rows)]).astype(np.int32)
  rng.shuffle(unsorted)
  order = np.argsort(unsorted, kind="stable").astype(np.int64)
  return unsorted[order], order


def digests():
  import torch
  from recoder_amd import _als_lib
  from recoder_amd._lib import ptr
  from recoder_amd.device import current_stream

  lib, dev = _als_lib.load(), "cuda"
  out = {}

  def t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)

  def padded(a, ld):
    """the table inside a [rows, ld] buffer filled with FILL: (buffer, ld)"""
    full = torch.full((a.shape[0], ld), FILL, dtype=torch.float32, device=dev)
    full[:, :a.shape[1]] = t(a, np.float32)
    return full

  def filled(shape, dtype=torch.float32, fill=FILL):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device=dev)

  def call(name, *args):
    _als_lib.check(getattr(lib, name)(*args, current_stream()), name)

  def put(name, **bufs):
    torch.cuda.synchronize()
    for k, v in bufs.items():
      out["%s.%s" % (name, k)] = hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest()

  indptr_h, indices_h, data_h = csr()
  indptr, indices, data = t(indptr_h), t(indices_h), t(data_h)
  nnz = int(indptr_h[-1])
  keys_h, order_h = run_keys(RUNS, N_ROWS, 6, 2)
  order_h[17] = len(keys_h) + 5                                # (an order outside the batch adds nothing)
  keys, order = t(keys_h), t(order_h)
  n = len(keys_h)
  ug_keys_h, ug_order_h = run_keys(UG_RUNS, N_ROWS, 27, 3)
  ug_keys, ug_order = t(ug_keys_h), t(ug_order_h)
  ug_n = len(ug_keys_h)
  assert n == 344 and ug_n == UG_T * UG_E

  for h in HS:
    rng = np.random.RandomState(100 + h)
    sc = 1.0 / np.sqrt(h)
    Xh, Yh = (rng.randn(N_USERS, h) * sc).astype(np.float32), (rng.randn(N_ITEMS, h) * sc).astype(np.float32)
    bias_h = (rng.randn(N_ITEMS) * 0.1).astype(np.float32)
    ldx, ldy = h + 3, h + 5
    X, Y, bias = padded(Xh, ldx), padded(Yh, ldy), t(bias_h)
    ubias = t((rng.randn(N_USERS) * 0.1).astype(np.float32))
    tag = "h%d" % h

    # ---- gram, solve, objective
    def gram(F, rows, ld, w, reg):
      G, v = filled((h, h)), filled(h)
      nb = lib.rk_als_gram_workspace_bytes(rows, h)
      ws = filled(nb // 4)
      call("rk_als_gram", ptr(F), rows, h, ld, ptr(w), reg, ptr(G), ptr(v), ptr(ws), nb)
      return G, v
    Gx, sx = gram(X, N_USERS, ldx, None, 0.5)
    Gy, cy = gram(Y, N_ITEMS, ldy, bias, 0.5)
    put(tag + ".gram", Gx=Gx, sx=sx, Gy=Gy, cy=cy)
    Gy1, vy1 = gram(Y, N_ITEMS, ldy, None, 0.5)
    for flags in (0, 1, 2):
      if flags and h not in (24, 96):
        continue
      Xs = X.clone()
      call("rk_als_solve", ptr(indptr), ptr(indices), ptr(data), 0, N_USERS, ptr(Y), ldy, h, ptr(Gy), ptr(cy),
           ptr(bias), None, 2.0, 3, ptr(Xs), ldx, flags)
      Xr = X.clone()                                           # (the item side's form: row_bias, v the column sums)
      call("rk_als_solve", ptr(indptr), ptr(indices), None, 0, N_USERS, ptr(Y), ldy, h, ptr(Gy1), ptr(vy1), None,
           ptr(ubias), 2.0, 3, ptr(Xr), ldx, flags)
      put("%s.solve%d" % (tag, flags), col_bias=Xs, row_bias=Xr)
    nb = lib.rk_als_objective_workspace_bytes(N_USERS)
    ws, obj = filled(nb // 4), torch.zeros(1, dtype=torch.float64, device=dev)
    call("rk_als_objective", ptr(indptr), ptr(indices), ptr(data), N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy, h,
         ptr(bias), 2.0, 0.5, ptr(Gx), ptr(Gy), ptr(sx), ptr(cy), ptr(ws), nb, ptr(obj))
    put(tag + ".objective", out=obj)

    # ---- BPR: sample, grad; apply on the runs
    users, pos, neg = (filled(T, torch.int32, 7) for _ in range(3))
    call("rk_als_bpr_sample", ptr(indptr), ptr(indices), N_USERS, N_ITEMS, nnz, SEED, STEP, T, ptr(users), ptr(pos),
         ptr(neg))
    g, loss, x, D, P = filled(T), filled(T), filled(T), filled((T, h)), filled((T, h))
    call("rk_als_bpr_grad", ptr(users), ptr(pos), ptr(neg), T, N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy, ptr(bias),
         h, ptr(g), ptr(loss), ptr(x), ptr(D), ptr(P))
    if h == HS[0]:
      put("bpr_sample", users=users, pos=pos, neg=neg)
    put(tag + ".bpr_grad", g=g, loss=loss, x=x, D=D, P=P)
    gw, V = t((rng.rand(n) + 0.1).astype(np.float32)), t((rng.randn(n, h) * sc).astype(np.float32))
    tab_h, tb_h = (rng.randn(N_ROWS, h) * sc).astype(np.float32), (rng.randn(N_ROWS) * 0.1).astype(np.float32)
    for roles in (1, 2):
      table, tb = padded(tab_h, h + 2), t(tb_h)
      call("rk_als_bpr_apply", ptr(keys), ptr(order), n, roles, ptr(gw), ptr(V), h, 0.1, 0.01, N_ROWS, ptr(table),
           h + 2, ptr(tb) if roles == 2 else None)
      Gs, cnt = torch.zeros((N_ROWS, h + 2), device=dev), torch.zeros(N_ROWS, dtype=torch.int32, device=dev)
      call("rk_als_lgcn_scatter", ptr(keys), ptr(order), n, roles, ptr(gw), ptr(V), h, 0.25, N_ROWS, ptr(Gs), h + 2,
           ptr(cnt))
      put("%s.runs%d" % (tag, roles), table=table, bias=tb, G=Gs, count=cnt)

    # ---- WARP / DNS
    weight = t(np.log(np.maximum(1.0, (N_ITEMS - 1) // np.maximum(np.arange(257), 1))).astype(np.float32))
    for mode in (1, 0):                                        # (WARP last: its slots feed rk_als_warp_grad)
      for max_draws in (1, 64, 65):
        ru, rp, rn, rt = (filled(T, torch.int32, 7) for _ in range(4))
        s_pos, s_neg, scores = filled(T), filled(T), filled((T, max_draws))
        call("rk_als_rank_sample", ptr(indptr), ptr(indices), N_USERS, N_ITEMS, nnz, SEED, STEP, T, ptr(X), ldx,
             ptr(Y), ldy, ptr(bias), h, mode, max_draws, min(3, max_draws), 0.05, ptr(ru), ptr(rp), ptr(rn), ptr(rt),
             ptr(s_pos), ptr(s_neg), ptr(scores))
        put("%s.rank%d_%d" % (tag, mode, max_draws), users=ru, pos=rp, neg=rn, trials=rt, s_pos=s_pos, s_neg=s_neg,
            scores=scores)
    g, loss, D, P = filled(T), filled(T), filled((T, h)), filled((T, h))
    call("rk_als_warp_grad", ptr(ru), ptr(rp), ptr(rn), ptr(rt), T, N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy,
         ptr(bias), h, 0.05, ptr(weight), ptr(g), ptr(loss), ptr(D), ptr(P))
    put(tag + ".warp_grad", g=g, loss=loss, D=D, P=P)

    # ---- LightGCN / SimGCL propagate (16-byte accesses where h allows, and the scalar form), adam
    rs, cs = t((rng.rand(N_USERS) + 0.5).astype(np.float32)), t((rng.rand(N_ITEMS) + 0.5).astype(np.float32))
    for ld in (h + 4 - h % 4 if h % 4 else h + 4, h + 1):
      F = padded(Yh, ld)
      for noise in (False, True):
        Out, Acc = filled((N_USERS, ld)), padded(Xh, ld)
        if noise:
          call("rk_als_gcl_propagate", ptr(indptr), ptr(indices), ptr(rs), ptr(cs), 0, N_USERS, ptr(F), ld, h,
               ptr(Out), ld, ptr(Acc), ld, 0.5, 0.1, SEED, STEP, 1, 2, 0)
        else:
          call("rk_als_lgcn_propagate", ptr(indptr), ptr(indices), ptr(rs), ptr(cs), 0, N_USERS, ptr(F), ld, h,
               ptr(Out), ld, ptr(Acc), ld, 0.5)
        put("%s.propagate_ld%d_%s" % (tag, ld - h, "gcl" if noise else "lgcn"), Out=Out, Acc=Acc)
    E0, H = padded(tab_h, h + 2), padded((rng.randn(N_ROWS, h) * sc).astype(np.float32), h + 1)
    M, Vv = t((rng.randn(N_ROWS, h) * 0.1).astype(np.float32)), t((rng.rand(N_ROWS, h) * 0.1).astype(np.float32))
    cnt = t(rng.randint(0, 5, N_ROWS).astype(np.int32))
    call("rk_als_lgcn_adam", ptr(E0), h + 2, ptr(H), h + 1, ptr(cnt), 0.01, ptr(M), ptr(Vv), N_ROWS, h, 0.01, 0.9,
         0.999, 1e-8, 3)
    put(tag + ".adam", E0=E0, M=M, V=Vv)

    # ---- SimGCL's contrast, DirectAU, the sampled softmax
    ck_h = np.sort(np.concatenate([rng.randint(0, 260, 290), np.full(10, 260)])).astype(np.int32)
    V1, V2 = padded((rng.randn(260, h) * sc).astype(np.float32), h + 1), padded((rng.randn(260, h) * sc).astype(np.float32), h + 2)
    V1[int(ck_h[5]), :h] = 0                                   # (a zero row: z = 0)
    ck = t(ck_h)
    G1, G2 = padded((rng.randn(260, h) * sc).astype(np.float32), h + 3), padded((rng.randn(260, h) * sc).astype(np.float32), h + 4)
    nb = lib.rk_als_gcl_contrast_workspace_bytes(T, h)
    ws, loss, count = filled(nb // 4), filled(1), filled(1, torch.int32, 7)
    call("rk_als_gcl_contrast", ptr(ck), T, 260, ptr(V1), h + 1, ptr(V2), h + 2, h, 0.2, 0.1, ptr(G1), h + 3,
         ptr(G2), h + 4, ptr(ws), nb, ptr(loss), ptr(count))
    put(tag + ".gcl_contrast", G1=G1, G2=G2, loss=loss, count=count)
    du_h, di_h = rng.randint(0, N_USERS, T).astype(np.int32), rng.randint(0, N_ITEMS, T).astype(np.int32)
    du_h[3], di_h[8] = -1, N_ITEMS
    du, di = t(du_h), t(di_h)
    nb = lib.rk_als_dau_workspace_bytes(T, h)
    ws, DU, DI, valid, loss, count = filled(nb // 4), filled((T, h)), filled((T, h)), filled(T), filled(3), \
        filled(1, torch.int32, 7)
    call("rk_als_dau_grad", ptr(du), ptr(di), T, N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy, h, 1.0, ptr(ws), nb,
         ptr(DU), ptr(DI), ptr(valid), ptr(loss), ptr(count))
    put(tag + ".dau_grad", DU=DU, DI=DI, valid=valid, loss=loss, count=count)
    Ts, S = 130, 70
    corr = t((rng.rand(N_ITEMS) * 0.1).astype(np.float32))
    nb = lib.rk_als_ssm_workspace_bytes(Ts, S, h)
    for cosine in (0, 1):
      ws, cand, DU, DC = filled(nb // 4), filled(Ts + S, torch.int32, 7), filled((Ts, h)), filled((Ts + S, h))
      valid, cvalid, loss, count = filled(Ts), filled(Ts + S), filled(2), filled(1, torch.int32, 7)
      call("rk_als_ssm_grad", ptr(du), ptr(di), Ts, S, SEED, STEP, N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy, h, 5.0,
           cosine, ptr(corr), ptr(ws), nb, ptr(cand), ptr(DU), ptr(DC), ptr(valid), ptr(cvalid), ptr(loss), ptr(count))
      put("%s.ssm_grad%d" % (tag, cosine), cand=cand, DU=DU, DC=DC, valid=valid, cvalid=cvalid, loss=loss, count=count)

    # ---- UltraGCN: the grad (E = 76: two rounds of 64 candidates), the scatter on its own runs
    Tu, R, K = 70, 70, 5
    E = 1 + R + K
    bu, bi = t((rng.rand(N_USERS) + 0.1).astype(np.float32)), t((rng.rand(N_ITEMS) + 0.1).astype(np.float32))
    ids_h = rng.randint(0, N_ITEMS, (N_ITEMS, K)).astype(np.int32)
    ids_h[::3, K // 2:] = -1
    ids, wts = t(ids_h), t(rng.rand(N_ITEMS, K).astype(np.float32))
    cand, coef, DU = filled((Tu, E), torch.int32, 7), filled((Tu, E)), filled((Tu, h))
    valid, loss = filled(Tu), filled((Tu, 3))
    call("rk_als_ugcn_grad", ptr(du), ptr(di), Tu, R, K, SEED, STEP, N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy, h,
         ptr(bu), ptr(bi), ptr(ids), ptr(wts), 0.3, 1.0, 0.2, 0.7, 3.0, 0.4, ptr(cand), ptr(coef), ptr(DU), ptr(valid),
         ptr(loss))
    put(tag + ".ugcn_grad", cand=cand, coef=coef, DU=DU, valid=valid, loss=loss)
    su_h = rng.randint(0, N_USERS, UG_T).astype(np.int32)
    su_h[4] = -1
    su = t(su_h)
    sc_coef = t((rng.randn(ug_n) * 0.1).astype(np.float32))
    Gs, cnt = torch.zeros((N_ROWS, h + 2), device=dev), torch.zeros(N_ROWS, dtype=torch.int32, device=dev)
    call("rk_als_ugcn_scatter", ptr(ug_keys), ptr(ug_order), ug_n, UG_E, ptr(su), ptr(sc_coef), ptr(X), ldx,
         N_USERS, h, 0.25, N_ROWS, ptr(Gs), h + 2, ptr(cnt))
    put(tag + ".ugcn_scatter", G=Gs, count=cnt)
  return out


def main():
  sys.path.insert(0, ROOT)
  d = digests()
  with open(OUT, "w") as f:
    json.dump(d, f, indent=0, sort_keys=True)
    f.write("\n")
  print("wrote %d digests to %s" % (len(d), OUT))


if __name__ == "__main__":
  main()
