"""Numpy restatement of CCL training (recoder_amd/ccl.py, rk_als_ccl_grad and rk_als_ccl_scatter of
include/recoder_als.h) on tests/lightgcn_util.py's propagation and Adam, the sampler of tests/bpr_util.py and the
per-slot draws of tests/ultragcn_util.py: in float64 (the model, pinned against torch autograd in
tests/test_ccl_host.py) and in float32 in the kernels' operation order -- the lane layout, fmaf chains and xor
butterflies of the header's numerics block, every fmaf(a, b, c) as the float64 a * b + c rounded to f32 -- for the
measurement of what f32 costs."""
import numpy as np
import scipy.sparse as sp

from tests import lightgcn_util as lg
from tests.directau_util import valid_slots
from tests.lightgcn_util import F32, F64, fma32
from tests.ultragcn_util import draws  # noqa: F401  (the negatives are UltraGCN's draws)

LONG_KEY, LONG_WAVES = 1024, 16
NEAR = 1e-5                                                    # |cosine - margin| below it: liveness is not compared


def candidates(users, items, negs, n_users, n_items):
  """(cand int64 [T, E], ok [T]): the positive and the R draws; n_items in every column of an invalid slot."""
  users, items = np.asarray(users).astype(np.int64), np.asarray(items).astype(np.int64)
  ok = valid_slots(users, items, n_users, n_items)
  cand = np.full((len(users), 1 + negs.shape[1]), n_items, np.int64)
  cand[ok, 0] = items[ok]
  cand[ok, 1:] = negs[ok]
  return cand, ok


def _unit(V):
  """(rows / norm, 1 / norm) in float64; a row of norm 0 gives the zero vector and 0."""
  n = np.sqrt((V * V).sum(1))
  inv = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)
  return V * inv[:, None], inv


def grad_rows(users, items, negs, X, Y, margin, negative_weight):
  """What rk_als_ccl_grad and rk_als_ccl_scatter (at scale 1) leave, in float64: a dict of cand, key (int32 [T, E]),
  coef, self, cos [T, E], DU [T, h], valid [T], loss [T, 2], live [T], DI [n_items, h] and count [n_items]."""
  X, Y = np.asarray(X, F64), np.asarray(Y, F64)
  users = np.asarray(users).astype(np.int64)
  (n_users, h), n_items = X.shape, Y.shape[0]
  T, R = negs.shape
  cand, ok = candidates(users, items, negs, n_users, n_items)
  E = 1 + R
  Xu = np.zeros((T, h))
  Xu[ok] = X[users[ok]]
  A, inv_nu = _unit(Xu)
  Ye = np.concatenate([Y, np.zeros((1, h))])
  B, inv_ny = _unit(Ye)
  if 8 * E < n_items:
    c = np.einsum("th,teh->te", A, B[cand])
  else:
    c = np.take_along_axis(A @ B.T, cand, 1)
  margin = float(F32(margin))                                  # (the kernel's margin is an f32)
  ns = float(negative_weight) / R
  lv = (c - margin > 0) & ok[:, None]
  lv[:, 0] = False
  w = np.where(lv, ns, 0.0)
  w[:, 0] = np.where(ok, -1.0, 0.0)
  carries = (w != 0) & (inv_ny[cand] > 0) & (inv_nu[:, None] > 0)
  w_eff = np.where(carries, w, 0.0)
  coef = w_eff * inv_nu[:, None] * inv_ny[cand]
  self_ = w_eff * c * inv_ny[cand] ** 2
  rows = np.repeat(np.arange(T), E)
  mat = lambda v: sp.csr_matrix((v.ravel(), (rows, cand.ravel())), shape=(T, n_items + 1))
  DU = inv_nu[:, None] * (np.asarray(mat(w_eff) @ B) - (w_eff * c).sum(1)[:, None] * A)
  DI = np.asarray(mat(coef).T @ Xu)[:n_items] - np.asarray(mat(self_).sum(0)).ravel()[:n_items, None] * Y
  loss = np.stack([np.where(ok, 1.0 - c[:, 0], 0.0), ns * np.where(lv, c - margin, 0.0).sum(1)], 1)
  key = np.where(carries, cand, n_items)
  count = np.bincount(key[:, 0], minlength=n_items + 1)[:n_items].astype(np.int32)
  return dict(cand=cand.astype(np.int32), key=key.astype(np.int32), coef=coef, self=self_, cos=c, DU=DU,
              valid=ok.astype(F64), loss=loss, live=lv.sum(1).astype(np.int32), DI=DI, count=count)


def near_margin(ref, margin):
  """[T, E] bool: the negatives of valid slots whose float64 cosine lies within NEAR of the margin."""
  near = np.abs(ref["cos"] - float(F32(margin))) < NEAR
  near[:, 0] = False
  return near & (ref["valid"] > 0)[:, None]


def slot_loss(users, items, negs, X, Y, margin, negative_weight):
  """sum_valid L_t in float64, written slot by slot (no matrices)."""
  X, Y = np.asarray(X, F64), np.asarray(Y, F64)
  cand, ok = candidates(users, items, negs, X.shape[0], Y.shape[0])
  R = negs.shape[1]
  unit = lambda v: v / np.sqrt(v @ v) if (v @ v) > 0 else np.zeros_like(v)
  total = 0.0
  for t in np.nonzero(ok)[0]:
    a = unit(X[int(users[t])])
    total += 1.0 - a @ unit(Y[cand[t, 0]])
    for j in cand[t, 1:]:
      total += (negative_weight / R) * max(0.0, a @ unit(Y[j]) - float(F32(margin)))
  return total


# ------------------------------------------------------- the kernels' chains
def group_width(h):
  """The lanes of a group of rk_als_ccl_grad: 16 for h <= 16, 32 for h <= 32, else the wave."""
  return 16 if h <= 16 else 32 if h <= 32 else 64


def _lanes(V, W):
  """[..., h] -> [..., NT, W]: dimension k = l + W q on lane l, register q; +0 past h."""
  h = V.shape[-1]
  nt = -(-h // W)
  out = np.zeros(V.shape[:-1] + (nt * W,), F32)
  out[..., :h] = V
  return out.reshape(V.shape[:-1] + (nt, W))


def _butterfly(s):
  """The xor butterfly over the last axis (offsets W / 2 .. 1); every lane ends with the same f32."""
  W = s.shape[-1]
  idx = np.arange(W)
  off = W // 2
  while off:
    s = (s + s[..., idx ^ off]).astype(F32)
    off //= 2
  return s[..., 0]


def _chain(Aq, Bq):
  """The fmaf chain over the registers from +0, then the butterfly: [..., NT, W] x [..., NT, W] -> [...]."""
  s = np.zeros(np.broadcast_shapes(Aq.shape, Bq.shape)[:-2] + (Aq.shape[-1],), F32)
  for q in range(Aq.shape[-2]):
    s = fma32(Aq[..., q, :], Bq[..., q, :], s)
  return _butterfly(s)


def _inv_norm(n2):
  with np.errstate(divide="ignore"):
    return np.where(n2 > 0, F32(1) / np.sqrt(n2, dtype=F32), F32(0)).astype(F32)


def grad_rows_f32(users, items, negs, X, Y, margin, negative_weight):
  """``grad_rows`` in f32, following the numerics block of rk_als_ccl_grad (no DI / count: see ``scatter_f32``)."""
  X, Y = np.asarray(X, F32), np.asarray(Y, F32)
  users = np.asarray(users).astype(np.int64)
  (n_users, h), n_items = X.shape, Y.shape[0]
  T, R = negs.shape
  E = 1 + R
  W = group_width(h)
  C = 64 // W
  cand, ok = candidates(users, items, negs, n_users, n_items)
  margin, ns = F32(margin), F32(F32(negative_weight) / F32(R))
  Xu = np.zeros((T, h), F32)
  Xu[ok] = X[users[ok]]
  pl = _lanes(Xu, W)                                           # [T, NT, W]
  inv_nu = _inv_norm(_chain(pl, pl))
  al = (pl * inv_nu[:, None, None]).astype(F32)
  yl = _lanes(np.concatenate([Y, np.zeros((1, h), F32)]), W)[cand]          # [T, E, NT, W]
  d = _chain(al[:, None], yl)
  iv = _inv_norm(_chain(yl, yl))
  cs = (d * iv).astype(F32)
  lv = ((cs - margin).astype(F32) > 0) & ok[:, None]
  lv[:, 0] = False
  w = np.where(lv, ns, F32(0)).astype(F32)
  w[:, 0] = np.where(ok, F32(-1), F32(0))
  used = (w != 0) & (iv > 0)                                   # what goes into the user's gradient
  wb = (w * iv).astype(F32)
  acc = np.zeros((T, C) + pl.shape[1:], F32)
  sc = np.zeros((T, C), F32)
  for e in range(E):                                           # ascending e within a group; group e mod C
    g, m = e % C, used[:, e]
    acc[:, g] = np.where(m[:, None, None], fma32(wb[:, e, None, None], yl[:, e], acc[:, g]), acc[:, g])
    sc[:, g] = np.where(m, fma32(w[:, e], cs[:, e], sc[:, g]), sc[:, g])
  if C > 1:                                                    # the groups' sums in ascending group, from +0
    tot, st = np.zeros_like(acc[:, 0]), np.zeros_like(sc[:, 0])
    for g in range(C):
      tot, st = (tot + acc[:, g]).astype(F32), (st + sc[:, g]).astype(F32)
  else:
    tot, st = acc[:, 0], sc[:, 0]
  du = (fma32(-st[:, None, None], al, tot) * inv_nu[:, None, None]).astype(F32)
  DU = du.reshape(T, -1)[:, :h]
  carries = (w != 0) & (iv > 0) & (inv_nu[:, None] > 0)
  coef = np.where(carries, ((w * inv_nu[:, None]).astype(F32) * iv).astype(F32), F32(0))
  self_ = np.where(carries, (((w * cs).astype(F32) * iv).astype(F32) * iv).astype(F32), F32(0))
  lanes = np.zeros((T, 64), F32)
  for e in range(1, E):                                        # lane e mod 64, its candidates in ascending e
    lanes[:, e % 64] = np.where(lv[:, e], (lanes[:, e % 64] + (cs[:, e] - margin).astype(F32)).astype(F32),
                                lanes[:, e % 64])
  loss = np.stack([np.where(ok, (F32(1) - cs[:, 0]).astype(F32), F32(0)), (ns * _butterfly(lanes)).astype(F32)], 1)
  key = np.where(carries, cand, n_items)
  assert coef.dtype == self_.dtype == DU.dtype == loss.dtype == F32
  return dict(cand=cand.astype(np.int32), key=key.astype(np.int32), coef=coef, self=self_, cos=cs, DU=DU,
              valid=ok.astype(F32), loss=loss, live=lv.sum(1).astype(np.int32))


def scatter_rows(key, coef, self_, users, X, Y, n_rows, dtype=F64):
  """(G [n_rows, h] at scale 1, count): rk_als_ccl_scatter over the entries (key, coef, self) [T, E].  float64: plain
  sums.  float32: the kernel's chains -- the coefficients' fmaf chain in ascending position (16 parts from LONG_KEY
  entries on), the self sums by lane and butterfly, the row as fmaf(-sum self, Y[key], sum)."""
  X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
  users = np.asarray(users).astype(np.int64)
  T, E = key.shape
  h = X.shape[1]
  G, count = np.zeros((n_rows, h), dtype), np.zeros(n_rows, np.int32)
  flat = key.ravel()
  order = np.argsort(flat, kind="stable")
  okv = (users >= 0) & (users < X.shape[0])
  for k in np.unique(flat[(flat >= 0) & (flat < n_rows)]):
    pos = order[np.searchsorted(flat[order], k, "left"):np.searchsorted(flat[order], k, "right")]
    good = okv[pos // E]
    count[k] = int((good & (pos % E == 0)).sum())
    cf = np.where(good, coef.ravel()[pos], 0).astype(dtype)
    sf = np.where(good, self_.ravel()[pos], 0).astype(dtype)
    rows = X[np.where(good, users[pos // E], 0)]
    if dtype == F64:
      G[k] = (cf[:, None] * rows).sum(0) - sf.sum() * Y[k]
      continue
    c = len(pos)
    part = -(-c // LONG_WAVES)
    parts = [(0, c)] if c < LONG_KEY else [(min(w * part, c), min((w + 1) * part, c)) for w in range(LONG_WAVES)]
    tot, st = None, None
    for lo, hi in parts:
      acc = np.zeros(h, F32)
      for j in range(lo, hi):
        acc = fma32(cf[j], rows[j], acc)
      lanes = np.zeros(64, F32)
      for j in range(lo, hi):
        lanes[(j - lo) % 64] = F32(lanes[(j - lo) % 64] + sf[j])
      ss = _butterfly(lanes)
      tot, st = (acc, ss) if tot is None else ((tot + acc).astype(F32), F32(st + ss))
    G[k] = fma32(-st, Y[k], tot)
  return G, count


# ----------------------------------------------------------------- fixtures
N = 40                                                         # rows of either table in the kernels' cases
SEED, STEP, MARGIN, NW = 5, 9, 0.4, 3.0
# (T, R, h) of the comparison against float64: every lane layout (h 1, 3 in groups of 16; 20 in groups of 32; the
# wave at 1, 2, 4 and 8 registers) x one slot, one block, more than one block; R = 5 and once R = 64 (two chunks)
CASES = tuple((T, 5, h) for T in (1, 2, 65, 257) for h in (1, 3, 20, 64, 65, 200, 512)) + ((65, 64, 64),)


def case(T, R, h):
  """Tables of N rows (random normal, f32 values) and T slots; from T = 65 on a slot with user -1, one with an item
  past the table, a zero user row and a zero item row in use (40 rows under 65 slots repeat users and items)."""
  rng = np.random.RandomState(1000 * T + 10 * R + h)
  X, Y = rng.randn(N, h).astype(F32), rng.randn(N, h).astype(F32)
  users, items = rng.randint(0, N, T).astype(np.int32), rng.randint(0, N, T).astype(np.int32)
  if T >= 65:
    X[7], Y[9] = 0, 0
    users[3], items[5], users[10], items[11] = -1, N, 7, 9
  return X, Y, users, items


# --------------------------------------------------------------------- step
def gradient(m, Eu, Ei, K, users, items, negs, margin, negative_weight, dtype=F64):
  """(H users, H items, counts users, counts items, (positive, negatives) summed over the slots, valid slots, live
  negatives): one step before Adam; the gradient of (1 / T) sum_valid L_t taken at the final tables and propagated
  back, the users' rows summed in ascending slots."""
  T = len(users)
  P, Q = lg.forward(m, Eu, Ei, K, dtype)
  if dtype == F64:
    r = grad_rows(users, items, negs, P, Q, margin, negative_weight)
    DI, ci = r["DI"], r["count"]
  else:
    r = grad_rows_f32(users, items, negs, P, Q, margin, negative_weight)
    DI, ci = scatter_rows(r["key"], r["coef"], r["self"], users, P, Q, Q.shape[0], F32)
  ok = r["valid"] > 0
  u = np.asarray(users)[ok].astype(np.int64)
  Gu = np.zeros_like(np.asarray(P, dtype))
  np.add.at(Gu, u, r["DU"][ok])
  cu = np.bincount(u, minlength=Gu.shape[0]).astype(np.int32)
  scale = dtype(1.0 / T)
  Gu, Gi = (Gu * scale, DI * scale) if dtype == F32 else (Gu / T, DI / T)
  Hu, Hi = lg.forward(m, Gu, Gi, K, dtype)
  return Hu, Hi, cu, ci, r["loss"].sum(0, dtype=F64), int(ok.sum()), int(r["live"].sum())


def step(m, state, K, users, items, negs, lr, reg, margin, negative_weight, dtype=F64):
  """One step on given slots and draws, on ``state`` in place: ((positive, negatives) summed, valid slots, live)."""
  Hu, Hi, cu, ci, loss, cnt, live = gradient(m, *state["E0"], K, users, items, negs, margin, negative_weight, dtype)
  lg.adam_both(state, Hu, Hi, cu, ci, len(users), lr, reg, dtype)
  return loss, cnt, live


def fit(m, Eu, Ei, K, num_epochs, batch_size, lr, reg, num_negatives, negative_weight, margin, seed=0, state=None,
        on_epoch=None):
  """(P, Q, state, history, stats): recoder_amd.ccl.fit restated (normalize=False) in float64, on the slots the
  kernel's sampler draws and the negatives of ``draws``; ``stats`` is the share of live negatives of each epoch."""
  m = sp.csr_matrix(m)
  state = lg.new_state(Eu, Ei) if state is None else state

  def one(users, pos, neg, s):
    negs = draws(seed, s, len(users), num_negatives, m.shape[1])
    loss, cnt, live = step(m, state, K, users, pos, negs, lr, reg, margin, negative_weight)
    return np.concatenate([loss, [cnt, live]])
  full = lg.epochs(m, state, num_epochs, batch_size, seed, on_epoch, one, np.zeros(4),
                   lambda sums, steps: tuple(sums[[0, 1, 3]] / sums[2]) if sums[2] else (float("nan"),) * 3)
  return lg.forward(m, *state["E0"], K) + (state, [e[:2] for e in full], [e[2] / num_negatives for e in full])


def unit_rows(V):
  return _unit(np.asarray(V, F64))[0]


quality = lg.quality


def fit_and_score(train, held_out, start, K=0, cosine=True, **kw):
  """(Recall@20, NDCG@100, history, stats) of the float64 fit from the tables ``start`` on (train, held out);
  ``cosine``: ranked by the cosine the fit trained (``train_ccl(normalize=True)``)."""
  P, Q, _, hist, stats = fit(train, start[0], start[1], K, **kw)
  if cosine:
    P, Q = unit_rows(P), unit_rows(Q)
  return quality(P, Q, train, held_out) + (hist, stats)
