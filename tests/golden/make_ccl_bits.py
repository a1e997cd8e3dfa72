#!/usr/bin/env python
"""The bits of the cosine contrastive loss' kernels: rk_als_ccl_grad and rk_als_ccl_scatter, driven directly through
recoder_amd._als_lib on seeded numpy inputs, and the SHA-256 of each output buffer (padding columns included).

    python tests/golden/make_ccl_bits.py [out]  # writes tests/golden/ccl_bits.json (needs the GPU)

tests/test_ccl_bits.py recomputes digests() and compares.  ccl_bits.json was written once, at commit b4b157a ("Add CCL:
SimpleX's cosine contrastive loss (train_ccl) on new HIP"), the last one in which the CCL kernels were a copy of
UltraGCN's beside them; it is not regenerated.  This script uses only names that exist there (make_als_bits' run_keys,
sizes, seeds and fill value), so checking that commit out beside this file and running it reproduces the fixture.  It
pins the kernels' order of operations as als_bits.json pins UltraGCN's: a digest that moves means a chain was
reordered, and the fix belongs in the kernels.  The cases, at every h of make_als_bits.HS (every NT; the 16-, 32- and
64-lane groups), with make_als_bits' padded leading dimensions:
  rk_als_ccl_grad at T = 96 and R = 25 (E = 26: one chunk of 64) and 70 (E = 71: a full chunk and a tail of 7), the
    margin the median cosine of the tables (rounded to three decimals: live and dead negatives mixed, which digests()
    asserts), a user row and an item row of norm 0 (the item is a slot's positive), a slot with a user index out of
    range and one with an item index out of range; all eight outputs, pre-filled
  rk_als_ccl_scatter at T = 96, E = 26 on make_als_bits.UG_RUNS (runs of 1, 4, 5, 63, 64, 65, 130, 1023 and 1024:
    RK_ALS_UGCN_LONG_KEY on either side, then 27 sentinels), some users out of range and one order outside the batch;
    G and count pre-filled and digested whole
The sort is make_als_bits' stable numpy argsort on the host."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:                                       # (run as a script: make_als_bits is tests.golden's)
  sys.path.insert(0, ROOT)
from tests.golden.make_als_bits import (FILL, HS, N_ITEMS, N_ROWS, N_USERS, SEED, STEP, UG_E, UG_RUNS, UG_T,  # noqa: E402
                                        run_keys)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ccl_bits.json")

T = UG_T                                                       # slots of the grad, as of the scatter
RS = (25, 70)
ZERO_USER, ZERO_ITEM = 5, 40


def median_cosine(X, Y):
  """The median cosine between the rows of X and of Y (rows of norm 0 left out) in float64, to three decimals: the
  rounding keeps the margin's bits apart from the last bits of the product."""
  def unit(A):
    A = A.astype(np.float64)
    norms = np.linalg.norm(A, axis=1)
    return A[norms > 0] / norms[norms > 0, None]
  return round(float(np.median(unit(X) @ unit(Y).T)), 3)


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

  keys_h, order_h = run_keys(UG_RUNS, N_ROWS, 27, 3)
  order_h[17] = len(keys_h) + 5                                # (an order outside the batch adds nothing)
  keys, order = t(keys_h), t(order_h)
  n = len(keys_h)
  assert n == UG_T * UG_E

  for h in HS:
    rng = np.random.RandomState(200 + h)
    sc = 1.0 / np.sqrt(h)
    Xh, Yh = (rng.randn(N_USERS, h) * sc).astype(np.float32), (rng.randn(N_ITEMS, h) * sc).astype(np.float32)
    Xh[ZERO_USER], Yh[ZERO_ITEM] = 0, 0
    ldx, ldy = h + 3, h + 5                                    # (make_als_bits' leading dimensions; G's is h + 2)
    X, Y = padded(Xh, ldx), padded(Yh, ldy)
    tag = "h%d" % h

    # ---- the grad
    users_h, items_h = rng.randint(0, N_USERS, T).astype(np.int32), rng.randint(0, N_ITEMS, T).astype(np.int32)
    users_h[2], items_h[7] = ZERO_USER, ZERO_ITEM
    users_h[3], items_h[8] = -1, N_ITEMS
    users, items = t(users_h), t(items_h)
    margin = median_cosine(Xh, Yh)
    for R in RS:
      E = 1 + R
      cand, key = filled((T, E), torch.int32, 7), filled((T, E), torch.int32, 7)
      coef, self_, DU = filled((T, E)), filled((T, E)), filled((T, h))
      valid, loss, live = filled(T), filled((T, 2)), filled(T, torch.int32, 7)
      call("rk_als_ccl_grad", ptr(users), ptr(items), T, R, SEED, STEP, N_USERS, N_ITEMS, ptr(X), ldx, ptr(Y), ldy, h,
           margin, 3.0, ptr(cand), ptr(key), ptr(coef), ptr(self_), ptr(DU), ptr(valid), ptr(loss), ptr(live))
      put("%s.ccl_grad%d" % (tag, R), cand=cand, key=key, coef=coef, self=self_, DU=DU, valid=valid, loss=loss,
          live=live)
      assert int(valid.sum()) == T - 2 and 0 < int(live.sum()) < (T - 2) * R, (h, R, margin, int(live.sum()))

    # ---- the scatter on UltraGCN's runs
    su_h = rng.randint(0, N_USERS, UG_T).astype(np.int32)
    su_h[4], su_h[50] = -1, N_USERS
    su = t(su_h)
    sc_coef, sc_self = t((rng.randn(n) * 0.1).astype(np.float32)), t((rng.randn(n) * 0.1).astype(np.float32))
    G, count = filled((N_ROWS, h + 2)), filled(N_ROWS, torch.int32, 7)
    call("rk_als_ccl_scatter", ptr(keys), ptr(order), n, UG_E, ptr(su), ptr(sc_coef), ptr(sc_self), ptr(X), ldx,
         N_USERS, ptr(Y), ldy, h, 0.25, N_ROWS, ptr(G), h + 2, ptr(count))
    put(tag + ".ccl_scatter", G=G, count=count)
  return out


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else OUT
  d = digests()
  with open(path, "w") as f:
    json.dump(d, f, indent=0, sort_keys=True)
    f.write("\n")
  print("wrote %d digests to %s" % (len(d), path))


if __name__ == "__main__":
  main()
