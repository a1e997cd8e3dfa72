"""GPU: rk_als_ugcn_grad and rk_als_ugcn_scatter against the float64 restatement (tests/ultragcn_util.py) within
first-order bounds derived from the kernels' chains, their repeatability, the item graph on the device, one whole
step, and Recoder.train_ultragcn end to end on the ML-20M slice."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util, lightgcn_util as lg, ultragcn_util as uu

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
TINY = 2.0 ** -126                                             # (an f32 below it may be flushed to 0)
N = 40                                                         # rows of either table in the kernels' cases
SEED, STEP = 5, 9
W, NW, IW = (0.3, 1.0, 0.2, 0.7), 3.0, 0.4
RS, KS = (1, 63, 64, 65, 130), (0, 1, 10)
# profiles/ultragcn_quality.jsonl: the "ultragcn_seed_spread" record -> recall20_spread, the restatement's Recall@20
# over five seeds as tools/ultragcn_bench.py --cpu-grid measures it, which is at the grid's best cell (lr 0.01, R 32,
# weight 8, 20 epochs) and not at the cell SLICE_FIT fits below (R 64, weight 64, 2 epochs); and the
# "ultragcn_test_reference" record -> recall20, the float64 fit of SLICE_FIT itself
SEED_SPREAD, REFERENCE_RECALL20 = 0.0036, 0.1102
SLICE_FIT = dict(batch_size=1024, lr=0.01, reg=1e-3, num_negatives=64, negative_weight=64.0, neighbours=10,
                 item_weight=1e-3, w=uu.PAPER_W)


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, ld, fill=7.0):
  a = np.asarray(a, np.float32)
  full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  full[:, :a.shape[1]] = _t(a)
  return full, full[:, :a.shape[1]]


# ------------------------------------------------------------------ cases
def _case(T, R, K, h):
  """Tables of N rows (f32 values), T slots and lists of K neighbours with rows short of K; from T = 65 on a slot
  with user -1, one with an item past the table, a zero user row and a zero item row in use (40 rows under 65 slots
  repeat users and items by themselves)."""
  rng = np.random.RandomState(1000 * T + 10 * R + K + h)
  X, Y = (rng.randn(N, h) / np.sqrt(h) * 2).astype(np.float32), (rng.randn(N, h) / np.sqrt(h) * 2).astype(np.float32)
  users, items = rng.randint(0, N, T).astype(np.int32), rng.randint(0, N, T).astype(np.int32)
  if T >= 65:
    X[7], Y[9] = 0, 0
    users[3], items[5], users[10], items[11] = -1, N, 7, 9
    assert len(set(users.tolist())) < T - 1 and len(set(items.tolist())) < T - 1
  bu, bi = (rng.rand(N) + 0.1).astype(np.float32), (rng.rand(N) + 0.1).astype(np.float32)
  ids = rng.randint(0, N, (N, K)).astype(np.int32)
  wts = rng.rand(N, K).astype(np.float32)
  for i in range(0, N, 3):                                     # (rows short of K: the tail is absent)
    ids[i, K // 2:], wts[i, K // 2:] = -1, 0
  return X, Y, users, items, bu, bi, ids, wts


def _grad_gpu(users, items, R, X, Y, bu, bi, ids, wts, ld_pad=3):
  """(cand, coef, DU, valid, loss) after one rk_als_ugcn_grad; both tables with a padded leading dimension, every
  output filled with 7 first."""
  from recoder_amd import ultragcn
  T, h, K = len(users), X.shape[1], ids.shape[1]
  E = 1 + R + K
  Xfull, Xv = _padded(X, h + ld_pad)
  Yfull, Yv = _padded(Y, h + ld_pad + 2)
  cand = torch.full((T, E), 7, dtype=torch.int32, device=DEV)
  coef, DU = torch.full((T, E), 7.0, device=DEV), torch.full((T, h), 7.0, device=DEV)
  valid, loss = torch.full((T,), 7.0, device=DEV), torch.full((T, 3), 7.0, device=DEV)
  ultragcn.grad(_t(users, np.int32), _t(items, np.int32), R, K, SEED, STEP, Xv, Yv, _t(bu), _t(bi),
                _t(ids, np.int32) if K else None, _t(wts) if K else None, W, NW, IW, cand, coef, DU, valid, loss)
  assert bool((Xfull[:, h:] == 7.0).all()) and bool((Yfull[:, h:] == 7.0).all()), "a padding column was written"
  return tuple(a.cpu().numpy() for a in (cand, coef, DU, valid, loss))


def _scatter_gpu(cand, coef, users, X, n_rows, ld_pad=3, row_pad=0):
  """(G [n_rows, h], count) after one stable sort of the candidates and one rk_als_ugcn_scatter; G padded in its
  leading dimension (and by ``row_pad`` rows behind the table), zeroed first as the contract asks."""
  from recoder_amd import ultragcn
  h = X.shape[1]
  full = torch.zeros((n_rows + row_pad, h + ld_pad), device=DEV)
  full[:, h:] = 7.0
  count = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
  keys, order = torch.sort(_t(cand, np.int32).view(-1), stable=True)
  ultragcn.scatter(keys, order, cand.shape[1], _t(users, np.int32), _t(coef).contiguous(), _padded(X, h + 1)[1],
                   1.0 / len(users), full[:n_rows, :h], count)
  assert bool((full[:, h:] == 7.0).all()) and not bool(full[n_rows:, :h].any()), "written outside the rows' h columns"
  return full[:n_rows, :h].cpu().numpy(), count.cpu().numpy()


def _bounds(users, items, negs, X, Y, bu, bi, ids, wts, ref):
  """First-order bounds (u = 2^-24), doubled for the second-order terms, on |kernel - float64| for coef [T, E],
  loss [T, 3], DU [T, h] and the scattered item gradient [n_items, h] at scale 1 / T.

  With A_s = sum_k |p_k| |y_k| of a candidate and a its weight:
    s     one fmaf chain over ceil(h / 64) registers and a butterfly of at most 6 levels (or, below the wave, of
          log2 W levels): at most h + 2 roundings deep                                -> ds = (h + 2) u A_s
    a     the product b^U b^I, the fmaf with w, the scale negative_weight / R (itself one division of two f32) or
          item_weight omega: at most 4 roundings of non-negative terms                 -> 4 u a
    sigma expf within 1 ulp (2 u relative), 1 + e, one division (correctly rounded), and the input ds through a
          slope of at most 1 / 4                                                       -> 5 u sigma + ds / 4
    coef  (sign a) sigma, two more roundings                   -> B_coef = 12 u |coef| + a ds / 4
    term  a softplus: max(x, 0) + log1pf(e) with log1pf within 1 ulp of at most softplus, e within 2 u e <= 2 u,
          the sum's rounding, the slope sigma <= 1 on ds, then a's 4 u and the product  -> B_term = a (ds + 8 u sp + 2 u)
    loss  the terms of a lane over ceil(E / 64) chunks and wave_sum's 6 levels, all non-negative
                                                               -> sum B_term + (ceil(E / 64) + 6) u sum term
    DU    E terms coef y in ascending e, a product and a sum each (fmaf at the wave's width: one rounding)
                                                               -> sum_e B_coef |y| + (E + 2) u sum_e |coef y|
    G     the kernel's own coef (within B_coef) times the exact user row, one fmaf chain per key of c entries, or 16
          chains of c / 16 and their 15 sums for a long key, then the scale (1 / T rounded, one product)
                                                               -> sum_e B_coef |x| + (c + 18) u sum_e |coef x|, / T"""
  cand, coef, DU, valid, loss, DI, count = ref
  X64, Y64 = np.asarray(X, np.float64), np.asarray(Y, np.float64)
  T, E = cand.shape
  R, h, n_items = negs.shape[1], X.shape[1], Y.shape[0]
  ok = valid > 0
  Xu = np.zeros((T, h))
  Xu[ok] = np.abs(X64[np.asarray(users)[ok]])
  Ye = np.concatenate([np.abs(Y64), np.zeros((1, h))])
  c64 = cand.astype(np.int64)
  ds = (h + 2) * U24 * np.take_along_axis(Xu @ Ye.T, c64, 1)
  x = np.where(np.arange(E)[None, :] - 1 < R, 1.0, -1.0) * np.ones((T, 1))
  x[:, 0] = -1.0
  sig = np.where(np.abs(coef) > 0, 1.0, 0.0)
  # a and softplus back from the reference: coef = sign a sigma(x), term = a softplus(x)
  Xs = np.zeros((T, h))
  Xs[ok] = X64[np.asarray(users)[ok]]
  s = np.take_along_axis(Xs @ np.concatenate([Y64, np.zeros((1, h))]).T, c64, 1) * x
  from scipy.special import expit
  a = np.where(sig > 0, np.abs(coef) / np.maximum(expit(s), 1e-300), 0.0)
  spl = np.logaddexp(0.0, s)
  b_coef = 12 * U24 * np.abs(coef) + a * ds / 4
  b_term = a * (ds + 8 * U24 * spl + 2 * U24)
  term = a * spl
  chain = (-(-E // 64) + 6) * U24
  b_loss = np.stack([b_term[:, 0] + chain * term[:, 0],
                     b_term[:, 1:1 + R].sum(1) + chain * term[:, 1:1 + R].sum(1),
                     b_term[:, 1 + R:].sum(1) + chain * term[:, 1 + R:].sum(1)], 1)
  rows = np.repeat(np.arange(T), E)
  mat = lambda v: sp.csr_matrix((v.ravel(), (rows, c64.ravel())), shape=(T, n_items + 1))
  b_du = np.asarray(mat(b_coef) @ Ye) + (E + 2) * U24 * np.asarray(mat(np.abs(coef)) @ Ye)
  per_key = np.bincount(c64.ravel(), minlength=n_items + 1)[:n_items]
  b_g = (np.asarray(mat(b_coef).T @ Xu)[:n_items] +
         (per_key[:, None] + 18) * U24 * np.asarray(mat(np.abs(coef)).T @ Xu)[:n_items]) / T
  return tuple(2 * b + TINY for b in (b_coef, b_loss, b_du, b_g))


def _check(T, R, K, h, label):
  X, Y, users, items, bu, bi, ids, wts = _case(T, R, K, h)
  negs = uu.draws(SEED, STEP, T, R, N)
  ref = uu.grad_rows(users, items, negs, X, Y, bu, bi, ids if K else None, wts if K else None, W, NW, IW)
  cand, coef, DU, valid, loss = _grad_gpu(users, items, R, X, Y, bu, bi, ids, wts)
  b_coef, b_loss, b_du, b_g = _bounds(users, items, negs, X, Y, bu, bi, ids, wts, ref)
  assert np.array_equal(cand, ref[0]), label                   # exact: the draws, the neighbours, the sentinels
  assert np.array_equal(valid, ref[3]), label
  absent = ref[0] == N
  assert not coef[absent].any() and not np.signbit(coef[absent]).any(), label      # (+0, not -0)
  worst = {}
  for name, got, want, bound in (("coef", coef, ref[1], b_coef), ("loss", loss, ref[4], b_loss),
                                 ("DU", DU, ref[2], b_du)):
    err = np.abs(got.astype(np.float64) - want)
    worst[name] = float((err / bound).max())
    assert (err <= bound).all(), (label, name, worst[name])
  G, count = _scatter_gpu(cand, coef, users, X, N)
  err = np.abs(G.astype(np.float64) - ref[5] / T)
  worst["G"] = float((err / b_g).max())
  assert (err <= b_g).all(), (label, "G", worst["G"])
  assert np.array_equal(count, ref[6]), label
  untouched = np.bincount(ref[0].ravel(), minlength=N + 1)[:N] == 0
  assert not G[untouched].any(), label
  return worst


@pytest.mark.parametrize("h", [1, 3, 20, 64, 65, 200, 512])       # (20: the two-candidate lane groups of 32)
@pytest.mark.parametrize("T", [1, 2, 65, 257])
def test_grad_and_scatter_against_float64(T, h):
  worst = {}
  for R in RS:
    for K in KS:
      for name, v in _check(T, R, K, h, (T, R, K, h)).items():
        worst[name] = max(worst.get(name, 0.0), v)
  print("T %d h %d: largest error / bound %s" % (T, h, {k: round(v, 4) for k, v in worst.items()}))
  assert all(v > 0 for v in worst.values()) or T * h == 1      # (the comparison is not vacuous)


# ---------------------------------------------------------- scatter's edges
def test_scatter_of_a_key_with_more_than_4096_entries_takes_the_long_path():
  """Item 4 is the positive of every slot and a neighbour of every item: 2 T entries under one key, T = 2100."""
  from recoder_amd import ultragcn
  T, R, K, h = 2100, 2, 2, 33
  rng = np.random.RandomState(3)
  X, Y = (rng.randn(N, h) * 0.3).astype(np.float32), (rng.randn(N, h) * 0.3).astype(np.float32)
  users, items = rng.randint(0, N, T).astype(np.int32), np.full(T, 4, np.int32)
  bu, bi = (rng.rand(N) + 0.1).astype(np.float32), (rng.rand(N) + 0.1).astype(np.float32)
  ids, wts = rng.randint(0, N, (N, K)).astype(np.int32), rng.rand(N, K).astype(np.float32)
  ids[:, 0] = 4
  negs = uu.draws(SEED, STEP, T, R, N)
  ref = uu.grad_rows(users, items, negs, X, Y, bu, bi, ids, wts, W, NW, IW)
  assert (ref[0] == 4).sum() >= 2 * T > 4096 > ultragcn.LONG_KEY
  lengths = np.bincount(ref[0].ravel(), minlength=N)
  assert 0 < lengths[lengths < ultragcn.LONG_KEY].max()         # (short keys beside the long one)
  cand, coef, DU, valid, loss = _grad_gpu(users, items, R, X, Y, bu, bi, ids, wts)
  assert np.array_equal(cand, ref[0])
  b_g = _bounds(users, items, negs, X, Y, bu, bi, ids, wts, ref)[3]
  G, count = _scatter_gpu(cand, coef, users, X, N, row_pad=2)
  err = np.abs(G.astype(np.float64) - ref[5] / T)
  print("long key: %d entries, largest error / bound %.4f" % ((ref[0] == 4).sum(), (err / b_g).max()))
  assert (err <= b_g).all() and np.array_equal(count, ref[6]) and count[4] == T and count.sum() == T
  again, count2 = _scatter_gpu(cand, coef, users, X, N, ld_pad=9)
  assert np.array_equal(G, again) and np.array_equal(count, count2)


@pytest.mark.parametrize("h", [33, 130, 512])
def test_scatter_hands_keys_of_1023_and_1024_entries_to_the_right_kernel(h):
  """Sorted layout: key 0 holds exactly 1024 entries (long, from position 0), key 1 holds 1023 (short, beginning on
  the multiple 1024), key 2 holds 1024 (long, beginning at 2047: its first multiple is 2048), key 3 holds 2200 (long,
  three multiples inside: only the first workgroup takes it), 229 entries lie past the table.  One slot has user -1:
  its entries add nothing and are not counted."""
  from recoder_amd import ultragcn
  assert ultragcn.LONG_KEY == 1024
  T, E = 1100, 5
  rng = np.random.RandomState(h)
  lengths = [1024, 1023, 1024, 2200]
  flat = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(lengths)] +
                        [np.full(T * E - sum(lengths), N, np.int32)])
  cand = rng.permutation(flat).reshape(T, E)
  coef = rng.randn(T, E).astype(np.float32)
  X = (rng.randn(N, h) * 0.5).astype(np.float32)
  users = rng.randint(0, N, T).astype(np.int32)
  users[17] = -1
  G, count = _scatter_gpu(cand, coef, users, X, N, row_pad=2)
  live = (users >= 0)[:, None] & (cand < N)
  tt, ee = np.nonzero(live)
  want, mass = np.zeros((N, h)), np.zeros((N, h))
  np.add.at(want, cand[tt, ee], coef[tt, ee].astype(np.float64)[:, None] * X[users[tt]].astype(np.float64))
  np.add.at(mass, cand[tt, ee], np.abs(coef[tt, ee].astype(np.float64))[:, None] * np.abs(X[users[tt]].astype(np.float64)))
  # the chain of _bounds' G with exact coefficients: (c + 18) u sum |coef x| / T, doubled
  per_key = np.bincount(flat, minlength=N + 1)[:N]
  bound = 2 * (per_key[:, None] + 18) * U24 * mass / T + TINY
  err = np.abs(G.astype(np.float64) - want / T)
  print("h %d: keys of %s entries, largest error / bound %.4f" % (h, lengths, (err / bound).max()))
  assert (err <= bound).all() and err[:4].max() > 0 and not G[4:].any()
  first = (cand[:, 0] < N) & (users >= 0)
  assert np.array_equal(count, np.bincount(cand[first, 0], minlength=N + 1)[:N]) and count[:4].min() > 0
  again, count2 = _scatter_gpu(cand, coef, users, X, N, ld_pad=11)
  assert np.array_equal(G, again) and np.array_equal(count, count2)


def test_scatter_of_keys_past_the_table_writes_nothing():
  T, E, h = 70, 5, 9
  cand = np.full((T, E), N, np.int32)
  coef = np.ones((T, E), np.float32)
  X = np.ones((N, h), np.float32)
  G, count = _scatter_gpu(cand, coef, np.zeros(T, np.int32), X, N, row_pad=2)
  assert not G.any() and not count.any()
  G, count = _scatter_gpu(cand, coef, np.zeros(T, np.int32), X, 7, row_pad=2)         # (a shorter table: still past it)
  assert not G.any() and not count.any()


def test_a_batch_of_invalid_slots_gives_zeros_and_sentinels():
  X, Y, _, _, bu, bi, ids, wts = _case(65, 5, 1, 4)
  cand, coef, DU, valid, loss = _grad_gpu(np.array([-1, N, 3], np.int32), np.array([2, 2, N], np.int32), 5, X, Y, bu,
                                          bi, ids, wts)
  assert (cand == N).all() and not coef.any() and not DU.any() and not valid.any() and not loss.any()


@pytest.mark.parametrize("h", [3, 20, 64, 200])
def test_the_same_call_gives_the_same_bits_whatever_the_leading_dimensions(h):
  T, R, K = 65, 65, 10
  X, Y, users, items, bu, bi, ids, wts = _case(T, R, K, h)
  first = _grad_gpu(users, items, R, X, Y, bu, bi, ids, wts)
  for pad in (3, 0, 64):
    again = _grad_gpu(users, items, R, X, Y, bu, bi, ids, wts, ld_pad=pad)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), pad
  G, count = _scatter_gpu(first[0], first[1], users, X, N)
  for pad, rows in ((3, 0), (0, 0), (17, 5)):
    G2, count2 = _scatter_gpu(first[0], first[1], users, X, N, ld_pad=pad, row_pad=rows)
    assert np.array_equal(G, G2) and np.array_equal(count, count2), (pad, rows)
  # a row range: a table cut after row 20 receives the same rows 0..19 and ignores the keys behind them
  G3, count3 = _scatter_gpu(first[0], first[1], users, X, 20, row_pad=3)
  assert np.array_equal(G3, G[:20]) and np.array_equal(count3, count[:20])
  # the draws of a slot do not depend on T: the first slots of a longer batch give the same rows
  short = _grad_gpu(users[:9], items[:9], R, X, Y, bu, bi, ids, wts)
  assert all(np.array_equal(a[:9], b) for a, b in zip(first, short))


# ------------------------------------------------------------- item graph
def test_item_graph_on_the_device_against_the_restatement():
  from recoder_amd import als, ultragcn
  m = uu.graph_fixture()
  ucsr, icsr = als.csr_pair(m, *m.shape, DEV)
  for K in (1, 4, 25):
    want_ids, want_w = uu.item_graph(m, K)
    for pair in ((ucsr, K, icsr), (ucsr, K)):                 # (with the caller's transpose and with its own)
      ids, wts = ultragcn.item_graph(*pair)
      assert ids.dtype == torch.int32 and wts.dtype == torch.float32 and tuple(ids.shape) == (20, K)
      assert np.array_equal(ids.cpu().numpy(), want_ids), K
      got = wts.cpu().numpy().astype(np.float64)
      assert (np.abs(got - want_w) <= 4 * U24 * want_w).all() and not got[want_ids < 0].any(), K
  m2 = m.copy()
  m2.data[:] = np.random.RandomState(0).rand(m2.nnz) + 0.5      # (the stored values play no part)
  ids2, wts2 = ultragcn.item_graph(als.csr_pair(m2, *m2.shape, DEV)[0], 4)
  ids, wts = ultragcn.item_graph(ucsr, 4)
  assert torch.equal(ids, ids2) and torch.equal(wts, wts2)


# ---------------------------------------------------------------- one step
def test_one_full_step_against_the_restatement_on_the_same_draws():
  from recoder_amd import als, lightgcn, ultragcn
  tr, _ = bpr_util.planted()
  h, T, R, K, lr, reg = 24, 256, 64, 5, float(np.float32(0.05)), float(np.float32(1e-3))
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))
  state = ultragcn.new_state(X, Y, 0)
  ws = ultragcn.Workspace(200, 120, T, h, DEV, num_negatives=R, neighbours=K)
  ultragcn.step(X, Y, graph, state, ws, 11, 3, lr, reg, R, NW, K, IW, W)
  users, pos = ws.bpr.users.cpu().numpy(), ws.bpr.pos.cpu().numpy()
  wu, wp, _ = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and state["step"] == 1 and state["num_layers"] == 0
  cons = uu.Constraints(tr, K, IW)
  assert np.array_equal(ws.bu.cpu().numpy(), cons.bu) and np.array_equal(ws.bi.cpu().numpy(), cons.bi)
  assert np.array_equal(ws.nbr_ids.cpu().numpy(), cons.nbr_ids)
  negs = uu.draws(11, 3, T, R, 120)
  assert np.array_equal(ws.cand.cpu().numpy()[:, 1:1 + R], negs) and bool((ws.bpr.g == 1).all())
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  l64, cnt = uu.step(s64, users, pos, negs, cons, lr, reg, W, NW, IW)
  l32, _ = uu.step(s32, users, pos, negs, cons, lr, reg, W, NW, IW, np.float32)
  got = ws.loss.double().sum(0).cpu().numpy()
  print("losses: kernels %s, f32 restatement %s, float64 %s" % (got, l32, l64))
  assert cnt == T
  # the yardstick of tests/test_lightgcn.py: the kernels stay within 4 x the distance of the f32 restatement (every
  # operation of the step in f32) from float64
  for k in range(3):
    dist, err = abs(l32[k] - l64[k]), abs(got[k] - l64[k])
    print("loss[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (k, dist, err))
    assert dist > 0 and err <= 4 * dist, k
  counts = [np.bincount(users, minlength=200), np.bincount(pos, minlength=120)]
  for side in (0, 1):
    assert np.array_equal(ws.count[side].cpu().numpy(), counts[side])
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      dist = np.abs(s32[key][side] - s64[key][side]).max()
      err = np.abs(state[key][side].cpu().numpy() - s64[key][side]).max()
      print("step %s[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (key, side, dist, err))
      assert dist > 0 and err <= 4 * dist, (key, side)


# -------------------------------------------------------------- end to end
def _recoder(h=64):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _tables(rec):
  m = rec.model
  return tuple(p.detach().cpu().numpy().copy() for p in
               (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


def _train(tr, start, epochs=(2,), **kw):
  """train_ultragcn at SLICE_FIT from the tables ``start`` (set after an empty fit has built the model); more than
  one entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder(start[0].shape[1])
  ds = RecommendationDataset(tr)
  kw = dict(SLICE_FIT, seed=0, **kw)
  assert rec.train_ultragcn(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  hist = []
  for k, n in enumerate(epochs):
    hist += rec.train_ultragcn(ds, num_epochs=n, resume=k > 0, **kw)
  return rec, hist, _tables(rec)


@pytest.fixture(scope="module")
def slice_fit():
  tr, ho = bpr_util.load_slice()
  start = bpr_util.xavier_tables(tr.shape[0], tr.shape[1], 64, 0)[:2]
  rec, hist, tables = _train(tr, start)
  return tr, ho, start, rec, hist, tables


def test_train_ultragcn_lowers_the_loss_and_resumes_bit_for_bit(slice_fit):
  tr, _, start, rec, hist, tables = slice_fit
  assert len(hist) == 2 and rec.ultragcn_history == hist and np.all(np.isfinite(hist))
  assert all(len(e) == 3 for e in hist) and sum(hist[1]) < sum(hist[0]), hist
  st = rec.ultragcn_state
  assert st["num_layers"] == 0 and st["step"] == 2 * -(-tr.nnz // 1024) and st["E0"][0].is_cuda
  assert rec.lightgcn_state is None and rec.ssm_state is None and not tables[2].any()
  _, hist3, resumed = _train(tr, start, epochs=(1, 1))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist


def test_item_weight_zero_never_builds_the_item_graph(slice_fit, monkeypatch):
  from recoder_amd import ease, ultragcn
  tr, _, start, _, hist, tables = slice_fit

  def no_gram(*a, **k):
    raise AssertionError("the n x n Gram was built")
  monkeypatch.setattr(ease, "gram", no_gram)
  monkeypatch.setattr(ultragcn, "item_graph", no_gram)
  for kw in (dict(item_weight=0.0), dict(neighbours=0)):
    _, base, other = _train(tr, start, epochs=(1,), **kw)
    assert len(base) == 1 and np.all(np.isfinite(base)) and base[0][2] == 0 and base[0][0] > 0
    assert np.all(np.isfinite(other[0])) and not np.array_equal(other[0], start[0])
  with pytest.raises(AssertionError, match="Gram was built"):
    _train(tr, start, epochs=(1,))


def test_recall_of_the_fit_beside_the_float64_restatement(slice_fit):
  """The same configuration, seed and start as tools/ultragcn_bench.py --test-reference; the gap allowed is the
  restatement's own spread over five seeds (profiles/ultragcn_quality.jsonl)."""
  tr, ho, _, _, hist, tables = slice_fit
  assert SEED_SPREAD is not None and REFERENCE_RECALL20 is not None
  r20, n100 = uu.quality(tables[0], tables[1], tr, ho)
  print("slice: Recall@20 of train_ultragcn %.4f (NDCG@100 %.4f), float64 restatement %.4f, margin %.4f; history %s"
        % (r20, n100, REFERENCE_RECALL20, SEED_SPREAD, hist))
  assert abs(r20 - REFERENCE_RECALL20) <= SEED_SPREAD


def test_the_fitted_tables_plug_into_the_rest(slice_fit, tmp_path):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.metrics import Recall
  tr, ho, _, rec, _, tables = slice_fit
  users = np.arange(50)
  inp = UsersInteractions(users, tr[users])
  lists = rec.recommend(inp, 10)
  assert len(lists) == 50 and all(len(l) == 10 for l in lists)
  seen = tr[users].toarray() > 0
  assert not any(seen[u, l].any() for u, l in enumerate(lists)) and all(len(set(l)) == 10 for l in lists)
  sub = np.arange(1000)
  res = rec.evaluate(RecommendationDataset(tr[sub], ho[sub]), num_recommendations=20,
                     metrics=[Recall(k=20, normalize=True)], batch_size=500)
  assert np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)) > 20.0 / tr.shape[1]      # (above chance)
  f = rec.save_state(str(tmp_path / "ultragcn"))
  rec2 = _recoder()
  rec2.init_from_model_file(f)
  assert all(np.array_equal(a, b) for a, b in zip(tables, _tables(rec2)))
  assert np.array_equal(rec.recommend_array(inp, 10), rec2.recommend_array(inp, 10))
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
  bpr_hist = rec.train_bpr(RecommendationDataset(tr), num_epochs=1)                       # (a warm start)
  assert len(bpr_hist) == 1 and np.isfinite(bpr_hist[0])
