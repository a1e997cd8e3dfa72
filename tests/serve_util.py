"""The constrained-serving kernels (csrc/als/serve.h, include/recoder_als.h) restated in numpy, the dense definition of
eligibility, and the float64 brute force every serving test compares against.  Nothing here touches torch.cuda or
recoder_amd.serve: tests/test_serve_host.py holds these restatements to each other.

* eligible_dense: the definition -- a stored POSITIVE entry is seen, the catalogue lists, the per-row patterns.
* mask_words: rk_als_serve_mask's bitmap [B, ldw] and count, built from that dense matrix.
* pair_order / pair_scores: rk_als_pair_scores' summation order, in f32 with exact fused multiply-adds.
* ragged_topk: rk_als_pairs_topk, on tests/recommend_util's ordering key.
* brute_force: the eligible items of a dense float64 score matrix by (score descending, id ascending), padded.
"""
import numpy as np
import scipy.sparse as sp

from tests import recommend_util as RU
from tests.als_util import _fma

F32 = np.float32


def pattern(matrix, rows, n_items):
  """bool [rows, n_items]: the stored entries of a scipy matrix, explicit zeros included (None: all False)."""
  out = np.zeros((rows, n_items), dtype=bool)
  if matrix is not None:
    m = sp.coo_matrix(matrix)
    out[m.row, m.col] = True
  return out


def catalogue(items, n_items):
  """bool [n_items] of an id list (duplicates allowed) or a boolean array."""
  a = np.asarray(items)
  if a.dtype == np.bool_:
    return a.copy()
  out = np.zeros(n_items, dtype=bool)
  out[a.astype(np.int64)] = True
  return out


def eligible_dense(rows, n_items, seen=None, filter_seen=True, allow_items=None, deny_items=None, user_allow=None,
                   user_deny=None):
  ok = np.ones((rows, n_items), dtype=bool)
  if filter_seen and seen is not None:
    dense = np.zeros((rows, n_items))
    s = sp.coo_matrix(seen)
    np.add.at(dense, (s.row, s.col), s.data)              # (duplicates summed, as the device CSR holds them)
    ok &= ~(dense > 0)
  if allow_items is not None:
    ok &= catalogue(allow_items, n_items)[None, :]
  if deny_items is not None:
    ok &= ~catalogue(deny_items, n_items)[None, :]
  if user_allow is not None:
    ok &= pattern(user_allow, rows, n_items)
  if user_deny is not None:
    ok &= ~pattern(user_deny, rows, n_items)
  return ok


def mask_words(ok, ldw):
  """(bits uint32 [B, ldw], eligible int32 [B]) of a dense eligibility matrix: bit c & 31 of word c >> 5 is 1 when item
  c is NOT eligible; the bits past n_items and the words past ceil(n_items / 32) are ones."""
  B, n = ok.shape
  deny = np.ones((B, ldw * 32), dtype=np.uint8)
  deny[:, :n] = ~ok
  bits = np.packbits(deny, axis=1, bitorder="little").view(np.uint32).reshape(B, ldw)
  return bits, ok.sum(axis=1).astype(np.int32)


def pair_order(h):
  """(W, Q): the lanes of a group and the float4 rounds of a lane, from h alone."""
  for top, w in ((16, 4), (32, 8), (64, 16), (128, 32), (256, 64)):
    if h <= top:
      return w, 1
  return 64, 2 if h <= 512 else 4 if h <= 1024 else 8


def pair_scores(z, Yrows, bias=None):
  """scores [m] f32 of one user row z [h] against the gathered item rows Yrows [m, h] (bias [m] or None): lane j < W
  owns d = 4 (j + W q) + c, one fmaf chain from +0 over q then c ascending, the xor butterfly at W / 2 .. 1, the
  bias added last."""
  z, Yrows = np.asarray(z, F32), np.asarray(Yrows, F32)
  m, h = Yrows.shape
  W, Q = pair_order(h)
  part = np.zeros((m, W), dtype=F32)
  for j in range(W):
    s = np.zeros(m, dtype=F32)
    for q in range(Q):
      for c in range(4):
        d = 4 * (j + W * q) + c
        if d < h:
          s = _fma(np.full(m, z[d], F32), Yrows[:, d], s, F32)
    part[:, j] = s
  off = W // 2
  lanes = np.arange(W)
  while off:
    part = (part + part[:, lanes ^ off]).astype(F32)
    off //= 2
  s = part[:, 0]
  return s if bias is None else (s + np.asarray(bias, F32)).astype(F32)


def forward_bound(z, Yrows, bias=None):
  """The standard forward bound of an (h + 1)-term f32 sum, any order: gamma_{h+1} (sum |z_d y_d| + |b|)."""
  z, Yrows = np.asarray(z, np.float64), np.asarray(Yrows, np.float64)
  h = Yrows.shape[1]
  u = (h + 1) * 2.0 ** -24
  mag = np.abs(Yrows * z[None, :]).sum(axis=1) + (0.0 if bias is None else np.abs(np.asarray(bias, np.float64)))
  return u / (1 - u) * mag


def ragged_topk(indptr, ids, scores, k, ok=None):
  """(ids int64 [B, k], values f32 [B, k], count [B]) of rk_als_pairs_topk: the entries with ok[e] (None: all) by
  (RU.order_key descending, id ascending), -1 / -inf past the row's count; a selected -0.0 reads +0.0."""
  B = len(indptr) - 1
  out = np.full((B, k), -1, dtype=np.int64)
  val = np.full((B, k), -np.inf, dtype=F32)
  cnt = np.zeros(B, dtype=np.int32)
  for r in range(B):
    lo, hi = int(indptr[r]), int(indptr[r + 1])
    keep = np.ones(hi - lo, dtype=bool) if ok is None else np.asarray(ok[lo:hi], dtype=bool)
    i, key = np.asarray(ids[lo:hi])[keep], RU.order_key(np.asarray(scores[lo:hi], F32))[keep]
    order = np.lexsort((i, RU.KEY_TOP - key))[:k]
    cnt[r] = keep.sum()
    out[r, :len(order)] = i[order]
    val[r, :len(order)] = RU.key_value(key[order])
  return out, val, cnt


def brute_force(scores, ok, k):
  """(ids int64 [B, k], scores float64 [B, k]): the eligible columns of a dense float64 score matrix by (score
  descending, id ascending), -1 / -inf past a row's eligible count."""
  scores = np.asarray(scores, np.float64)
  B = scores.shape[0]
  ids = np.full((B, k), -1, dtype=np.int64)
  val = np.full((B, k), -np.inf)
  for r in range(B):
    cols = np.nonzero(ok[r])[0]
    order = cols[np.argsort(-scores[r, cols], kind="stable")][:k]
    ids[r, :len(order)] = order
    val[r, :len(order)] = scores[r, order]
  return ids, val


def masked_topk_padded(scores, ok, k):
  """The expected list of the mask route from a strip scorer's own f32 output: recommend_util.masked_topk over the
  scores with the ineligible columns at -inf, then -1 / -inf past the eligible count."""
  scores = np.where(ok, np.asarray(scores, F32), F32(-np.inf))
  ids, val = RU.masked_topk(scores, k)
  pad = np.arange(k)[None, :] >= ok.sum(axis=1)[:, None]
  return np.where(pad, -1, ids), np.where(pad, F32(-np.inf), val).astype(F32)


def csr_lists(rows, n_items, counts, rng, must=()):
  """scipy CSR [rows, n_items] of ones with counts[r] distinct random items in row r (those of `must` first)."""
  indptr, idx = [0], []
  for r in range(rows):
    c = int(counts[r])
    head = [m for m in must if m < n_items][:c]
    rest = np.setdiff1d(np.arange(n_items), head)
    row = np.sort(np.concatenate([head, rng.choice(rest, size=c - len(head), replace=False)]).astype(np.int64))
    idx.append(row)
    indptr.append(indptr[-1] + c)
  idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
  return sp.csr_matrix((np.ones(len(idx), F32), idx.astype(np.int32), np.asarray(indptr, np.int64)),
                       shape=(rows, n_items))
