"""GPU: the rk_als_ials_* kernels and Recoder.train_ials against the float64 restatement of tests/ials_util.py.

Every kernel comparison is max |got - f64| <= bound * max |f64| with bound = 4 x the largest such error of the float32
restatement (numpy's own summation order) against the float64 one on the same inputs; the factor covers another
summation order.  The f32 errors were measured on the CPU from the restatement alone (tests/test_ials_host.py
re-measures them and checks these constants), never from the kernels:

  predict, panel (37 x 53):  h = 4: 6.7e-08, 9.7e-08   h = 20: 1.0e-07, 1.9e-07   h = 200: 1.2e-07, 2.2e-07
      h = 520 (above rk_als_gram's 512: the objective's Grams are stacked from panels): 2.9e-07, 2.2e-07
  objective: L is float64 on the device and takes the very f32 cache, Grams and tables the check reads back, so its
      bound is that of a float64 sum in another order, 1e-12
  block step (tables and cache, both sides):  BLOCK_F32_ERR below, per case
  the empty matrix's user step:  1.5e-07
  the fit on the slice subset (3 sweeps, the default alpha0 and reg):  tables 1.29e-06; L 1.29e-09 (the largest of the
      three sweeps); the Recall@20 cap of that test, from the restatement alone: 0 (none of the 1326 users with
      held-out items)
  the fit at h = 520 (60 x 80, blocks of 64, 2 sweeps):  tables 3.2e-06; L 1.33e-08
"""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from . import ials_util as U

pytestmark = pytest.mark.gpu

# 4 x the f32 restatement's error (above); h -> (predict, panel)
KERNEL_F32_ERR = {4: (6.7e-08, 9.7e-08), 20: (1.0e-07, 1.9e-07), 200: (1.2e-07, 2.2e-07), 520: (2.9e-07, 2.2e-07)}
KERNEL_BOUND = {h: (4 * ep, 4 * en) for h, (ep, en) in KERNEL_F32_ERR.items()}
OBJECTIVE_BOUND = 1e-12
# case -> the f32 restatement's largest error over (table, cache) on both sides
BLOCK_F32_ERR = {"h24_k8": 2.5e-07, "h20_tail": 2.3e-07, "h32_exact": 8.6e-07, "h128_exact": 7.0e-06,
                 "long_row": 7.0e-07, "row_range": 2.0e-07, "long_row_k64": 9.8e-06, "long_row_k128": 2.5e-05,
                 "h520_k64": 1.9e-06}
EMPTY_F32_ERR = 1.5e-07
# the fits: the f32 restatement's (tables, L) against float64, L the largest over the sweeps
SUB_F32_ERR = (1.29e-06, 1.29e-09)
BIG_F32_ERR = (3.2e-06, 1.33e-08)
TABLE_BOUND, L_BOUND = 4 * SUB_F32_ERR[0], 4 * SUB_F32_ERR[1]


def _dev(a, dtype=torch.float32):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _pair(m):
  from recoder_amd import ials
  return ials.Pair(m, m.shape[0], m.shape[1], torch.device("cuda"))


def _rel(got, want):
  want = np.asarray(want, np.float64)
  scale = np.abs(want).max()
  return float(np.abs(np.asarray(got, np.float64) - want).max() / (scale if scale else 1.0))


def _tables(n_users, n_items, h, seed, std=1.0):
  rng = np.random.RandomState(seed)
  return (std * rng.randn(n_users, h)).astype(np.float32), (std * rng.randn(n_items, h)).astype(np.float32)


@pytest.mark.parametrize("h", [4, 20, 200, 520])
def test_predict_panel_objective_against_float64(h):
  from recoder_amd import ials
  m, X, Y = U.kernel_problem(h)
  pair = _pair(m)
  # the item table lives in a wider allocation: its row stride exceeds h
  wide = torch.zeros(53, h + 3, device="cuda")
  wide[:, :h] = _dev(Y)
  Xd, Yd = _dev(X), wide[:, :h]
  bp, bn = KERNEL_BOUND[h]
  c = ials.predict(pair.ucsr, Xd, Yd)[:m.nnz].cpu().numpy()
  err = _rel(c, U.predict(m, X, Y))
  print("predict h=%d: %.3g (bound %.3g)" % (h, err, bp))
  assert err <= bp
  k = min(h, 64)
  for F, Fd in ((X, Xd), (Y, Yd)):
    for p0, kb in U.blocks(h, k)[-2:]:
      P = ials.gram_panel(Fd, p0, kb).cpu().numpy()
      err = _rel(P, U.gram_panel(F, p0, kb))
      print("panel h=%d p0=%d: %.3g (bound %.3g)" % (h, p0, err, bn))
      assert err <= bn
  lam64, mu64 = U.regularisers(m, 0.1, 0.05, 1.0)
  lam, mu = lam64.astype(np.float32), mu64.astype(np.float32)
  Gx, Gy = ials.full_gram(Xd, k), ials.full_gram(Yd.contiguous(), k)
  out = torch.zeros(1, dtype=torch.float64, device="cuda")
  cd = _dev(c)
  ials.objective(cd, m.nnz, Gx, Gy, Xd, _dev(lam), Yd, _dev(mu), 0.1, out)
  x64, y64 = X.astype(np.float64), Y.astype(np.float64)
  want = ((c.astype(np.float64) - 1) ** 2).sum() + np.float32(0.1).astype(np.float64) * \
      (Gx.cpu().numpy().astype(np.float64) * Gy.cpu().numpy().astype(np.float64)).sum() + \
      (lam * (x64 * x64).sum(1)).sum() + (mu * (y64 * y64).sum(1)).sum()
  err = abs(out.item() - want) / want
  print("objective h=%d: %.3g" % (h, err))
  assert err <= OBJECTIVE_BOUND
  # and against the restatement's L from the tables, within the cache's and the Grams' f32 bounds
  assert abs(out.item() - U.objective(m, X, Y, lam, mu, np.float32(0.1))) <= 2 * (bp + 2 * bn) * want


def test_empty_matrix():
  from recoder_amd import ials
  m, X, Y, lam, mu, _ = U.empty_problem()
  pair = _pair(m)
  Xd, Yd = _dev(X), _dev(Y)
  cache = ials.predict(pair.ucsr, Xd, Yd)
  lam, mu = _dev(lam), _dev(mu)
  status = torch.zeros(1, dtype=torch.int32, device="cuda")
  X64, Y64, c64 = X.astype(np.float64), Y.astype(np.float64), np.zeros(0)
  # (a block of 4 of the 8 coordinates: the full block's solution would be the zero row exactly)
  ials.block(pair.ucsr, None, Yd, Xd, ials.gram_panel(Yd, 4, 4), lam, 0.5, 4, 4, cache, status)
  U.block_step(m, None, Y64, X64, U.gram_panel(Y64, 4, 4), lam.cpu().numpy(), np.float32(0.5), 4, 4, c64)
  err = _rel(Xd.cpu().numpy(), X64)
  print("empty matrix: %.3g (bound %.3g)" % (err, 4 * EMPTY_F32_ERR))
  assert err <= 4 * EMPTY_F32_ERR and status.item() == 0
  out = torch.zeros(1, dtype=torch.float64, device="cuda")
  ials.objective(cache, 0, ials.full_gram(Xd, 8), ials.full_gram(Yd, 8), Xd, lam, Yd, mu, 0.5, out)
  want = U.objective(m, Xd.cpu().numpy(), Y, lam.cpu().numpy(), mu.cpu().numpy(), np.float32(0.5))
  # (L from the device's own tables in float64: only the Grams' f32 rounding separates the two; h = 8 sits between
  #  the measured panel errors of h = 4 and h = 20, the larger is taken)
  assert abs(out.item() - want) <= 2 * KERNEL_BOUND[20][1] * want


BLOCK_CASES = U.BLOCK_CASES


@pytest.mark.parametrize("case", sorted(BLOCK_CASES))
def test_block_step_against_float64(case):
  from recoder_amd import _als_lib, ials
  n_users, n_items, h, k, p0, density, empty_rows, full_cols, empty_cols, rng_rows = BLOCK_CASES[case]
  m, X, Y, lam, mu, a0 = U.block_problem(case)
  if case == "long_row":
    assert np.bincount(m.indices, minlength=n_items).max() >= _als_lib.IALS_LONG_ROW
  mt, perm = U.transpose_permutation(m)
  pair = _pair(m)
  assert np.array_equal(pair.perm.cpu().numpy()[:m.nnz], perm)
  Xd, Yd = _dev(X), _dev(Y)
  cache = ials.predict(pair.ucsr, Xd, Yd)
  c0 = cache.cpu().numpy()[:m.nnz].copy()
  status = torch.zeros(1, dtype=torch.int32, device="cuda")
  bound = 4 * BLOCK_F32_ERR[case]
  X64, Y64, c64 = X.astype(np.float64), Y.astype(np.float64), c0.astype(np.float64)

  def rows_of(n):
    return None if rng_rows is None else range(rng_rows[0], min(rng_rows[1], n))
  lo, hi = (0, None) if rng_rows is None else rng_rows
  # the user side
  Pd = ials.gram_panel(Yd, p0, k)
  ials.block(pair.ucsr, None, Yd, Xd, Pd, _dev(lam), a0, p0, k, cache, status, lo, hi)
  U.block_step(m, None, Y64, X64, Pd.cpu().numpy().astype(np.float64), lam, a0, p0, k, c64, rows=rows_of(n_users))
  got = Xd.cpu().numpy()
  outside = np.ones(h, bool)
  outside[p0:p0 + k] = False
  assert got[:, outside].tobytes() == X[:, outside].tobytes()
  if rng_rows is not None:
    keep = np.r_[0:lo, hi:n_users]
    assert got[keep].tobytes() == X[keep].tobytes()
    e_lo, e_hi = m.indptr[lo], m.indptr[hi]
    cg = cache.cpu().numpy()[:m.nnz]
    assert cg[:e_lo].tobytes() == c0[:e_lo].tobytes() and cg[e_hi:].tobytes() == c0[e_hi:].tobytes()
  for u in empty_rows:                                   # no entries: the dense part alone moves the row
    if rng_rows is not None and not lo <= u < hi:
      continue
    assert not np.array_equal(got[u, p0:p0 + k], X[u, p0:p0 + k])
  errs = [_rel(got, X64), _rel(cache.cpu().numpy()[:m.nnz], c64)]
  # the item side, on the tables and the cache the user side left
  Xn = got.copy()
  c_user = cache.cpu().numpy()[:m.nnz].copy()
  X64i, c64i = Xn.astype(np.float64), c_user.astype(np.float64)
  Pd = ials.gram_panel(Xd, p0, k)
  hi_i = None if rng_rows is None else min(hi, n_items)
  ials.block(pair.icsr, pair.perm, Xd, Yd, Pd, _dev(mu), a0, p0, k, cache, status, lo, hi_i)
  U.block_step(mt, perm, X64i, Y64, Pd.cpu().numpy().astype(np.float64), mu, a0, p0, k, c64i, rows=rows_of(n_items))
  goty = Yd.cpu().numpy()
  assert goty[:, outside].tobytes() == Y[:, outside].tobytes()
  assert Xd.cpu().numpy().tobytes() == Xn.tobytes()
  if rng_rows is not None:                               # the item rows outside the range and their cache entries
    keep = np.r_[0:lo, hi_i:n_items]
    assert goty[keep].tobytes() == Y[keep].tobytes()
    inside = np.zeros(m.nnz, bool)
    inside[perm[mt.indptr[lo]:mt.indptr[hi_i]]] = True
    assert inside.any() and not inside.all()
    assert cache.cpu().numpy()[:m.nnz][~inside].tobytes() == c_user[~inside].tobytes()
  errs += [_rel(goty, Y64), _rel(cache.cpu().numpy()[:m.nnz], c64i)]
  # the cache the item side leaves is a fresh predict of the tables, within the bound
  fresh = U.predict(m, Xn, goty)
  errs.append(_rel(cache.cpu().numpy()[:m.nnz], fresh))
  print("%s: table/cache errors %s (bound %.3g)" % (case, ["%.3g" % e for e in errs], bound))
  assert status.item() == 0
  assert max(errs) <= bound


def test_singular_rows_are_left_and_counted():
  """reg = 0 and alpha0 = 0: an empty row's system is the zero matrix; the row and the cache stay, status counts it."""
  from recoder_amd import ials
  m = U.random_csr(9, 11, 0.8, seed=2, empty_rows=(2, 6))
  counts = np.diff(m.indptr)
  assert counts[counts > 0].min() >= 6                    # (every other row's 4 x 4 system has full rank)
  X, Y = _tables(9, 11, 8, 5)
  pair = _pair(m)
  Xd, Yd = _dev(X), _dev(Y)
  cache = ials.predict(pair.ucsr, Xd, Yd)
  zero = torch.zeros(9, device="cuda")
  status = torch.zeros(1, dtype=torch.int32, device="cuda")
  ials.block(pair.ucsr, None, Yd, Xd, ials.gram_panel(Yd, 0, 4), zero, 0.0, 0, 4, cache, status)
  got = Xd.cpu().numpy()
  assert status.item() == 2
  assert got[[2, 6]].tobytes() == X[[2, 6]].tobytes()
  others = [u for u in range(9) if u not in (2, 6)]
  assert all(not np.array_equal(got[u, :4], X[u, :4]) for u in others)
  assert got[:, 4:].tobytes() == X[:, 4:].tobytes()


def _fit_bits(m, h, k, sweeps, seed=0, calls=1):
  from recoder_amd import ials
  X0, Y0 = U.init_tables(m.shape[0], m.shape[1], h, 0.5, seed)
  Xd, Yd = _dev(X0), _dev(Y0)
  pair = _pair(m)
  hist = []
  for _ in range(calls):
    hist += ials.fit(Xd, Yd, pair, 0.1, 0.01, 1.0, k, sweeps // calls)
  return Xd.cpu().numpy(), Yd.cpu().numpy(), hist


def test_two_runs_give_the_same_bits():
  """(1100 users with one item held by all of them: the item side takes the long-row kernel.)"""
  m = U.random_csr(1100, 40, 0.05, seed=8, empty_rows=(1,), full_cols=(9,))
  a, b = _fit_bits(m, 24, 8, 2), _fit_bits(m, 24, 8, 2)
  assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
  c = _fit_bits(m, 24, 8, 4)
  d = _fit_bits(m, 24, 8, 4, calls=2)
  assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes() and c[2] == d[2]


# ------------------------------------------------------------------------------------------------ Recoder.train_ials
SUB_H, SUB_BLOCK, SUB_SWEEPS = U.SUB_H, U.SUB_BLOCK, U.SUB_SWEEPS


@pytest.fixture(scope="module")
def subset():
  from recoder_amd import ials
  assert (ials.DEFAULT_ALPHA0, ials.DEFAULT_REG) == (U.SUB_ALPHA0, U.SUB_REG)
  x, y, X0, Y0 = U.subset_problem()
  X, Y, hist = U.fit(x, X0, Y0, U.SUB_ALPHA0, U.SUB_REG, 1.0, SUB_BLOCK, SUB_SWEEPS, fast=True)
  return x, y, X, Y, hist


def _recoder(h=SUB_H):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _dataset(x, y=None):
  from recoder_amd.data import RecommendationDataset
  return RecommendationDataset(x) if y is None else RecommendationDataset(x, y)


def test_train_ials_on_the_slice_subset(subset):
  from recoder_amd.metrics import Recall
  x, y, X, Y, hist = subset
  rec = _recoder()
  got = rec.train_ials(_dataset(x), num_sweeps=SUB_SWEEPS, block_size=SUB_BLOCK, init_std=0.1, seed=0)
  assert got == rec.ials_history and len(got) == SUB_SWEEPS
  errs = [abs(a - b) / b for a, b in zip(got, hist)]
  print("L history:", got, "restatement:", hist, "relative errors:", errs, "bound", L_BOUND)
  assert max(errs) <= L_BOUND
  tabs = [_rel(t.weight.data.cpu().numpy(), w) for t, w in ((rec.model.user_embedding_layer, X),
                                                             (rec.model.item_embedding_layer, Y))]
  print("tables:", tabs, "bound", TABLE_BOUND)
  assert max(tabs) <= TABLE_BOUND
  assert not rec.model.bias.data.any()
  # Recall@20: at most the users whose 20th and 21st restated scores lie closer than the table bound may differ
  S = X @ Y.T
  seen = sp.csr_matrix(x)
  for u in range(S.shape[0]):
    S[u, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]] = -np.inf
  top = -np.sort(-S, axis=1)[:, :21]
  # "closer than the table bound": the bound scaled to the largest restated score of an unseen item
  thr = TABLE_BOUND * np.abs(top[np.isfinite(top)]).max()
  has = np.diff(y.indptr) > 0
  close = (top[:, 19] - top[:, 20] < thr) & has
  cap = close.sum() / has.sum()
  want = U.recall_at(U.top_k(X @ Y.T, x, 20), y, 20)
  res = rec.evaluate(_dataset(x, y), num_recommendations=20, metrics=[Recall(k=20, normalize=True)], batch_size=500)
  value = float(np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)))
  print("Recall@20 %.5f restated %.5f cap %.5f" % (value, want, cap))
  assert cap < 0.01
  assert abs(value - want) <= cap + 1e-12          # (1e-12: the mean's own summation order)


def test_warm_start_and_the_states_consumers(subset, tmp_path):
  x = subset[0]
  ds = _dataset(x)
  a = _recoder()
  ha = a.train_ials(ds, num_sweeps=4, block_size=SUB_BLOCK, init_std=0.1, seed=3)
  b = _recoder()
  hb = b.train_ials(ds, num_sweeps=2, block_size=SUB_BLOCK, init_std=0.1, seed=3)
  hb += b.train_ials(ds, num_sweeps=2, block_size=SUB_BLOCK)
  assert ha == hb
  for name in ("user_embedding_layer", "item_embedding_layer"):
    assert torch.equal(getattr(a.model, name).weight.data, getattr(b.model, name).weight.data)
  assert all(l1 < l0 for l0, l1 in zip(ha, ha[1:]))
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  users = UsersInteractions(np.arange(64), x[:64])
  ids = a.recommend_array(users, 10)
  path = a.save_state(str(tmp_path / "ials"))
  c = Recoder(model=MatrixFactorization(SUB_H))
  c.init_from_model_file(path)
  assert np.array_equal(c.recommend_array(users, 10), ids)
  rows = a.fold_in(x[:32], alpha=1.0, reg=1.0)
  assert tuple(rows.shape) == (32, SUB_H) and bool(torch.isfinite(rows).all())
  als_hist = a.train_als(ds, num_iterations=1, reg=1.0)
  assert len(als_hist) == 1 and np.isfinite(als_hist[0])


def test_validation_leaves_the_bits_and_restores_the_best(subset):
  x, y = subset[0], subset[1]
  ds, val = _dataset(x), _dataset(x, y)
  kw = dict(block_size=SUB_BLOCK, init_std=0.1, seed=1)
  plain = _recoder()
  plain.train_ials(ds, num_sweeps=3, **kw)
  watched = _recoder()
  watched.train_ials(ds, num_sweeps=3, val_dataset=val, **kw)
  assert plain.ials_validation is None and len(watched.ials_validation["values"]) == 3
  for name in ("user_embedding_layer", "item_embedding_layer"):
    assert torch.equal(getattr(plain.model, name).weight.data, getattr(watched.model, name).weight.data)
  stopped = _recoder()
  hist = stopped.train_ials(ds, num_sweeps=12, val_dataset=val, patience=1, restore_best=True, **kw)
  v = stopped.ials_validation
  assert v["best_epoch"] is not None and len(hist) == len(v["values"]) <= 12
  best = _recoder()
  best.train_ials(ds, num_sweeps=v["best_epoch"], **kw)
  for name in ("user_embedding_layer", "item_embedding_layer"):
    assert torch.equal(getattr(best.model, name).weight.data, getattr(stopped.model, name).weight.data)


def test_train_ials_above_the_cg_solvers_embedding_size():
  """h = 520 > rk_als_gram's 512 through the public entry point: the L history (its Grams stacked from panels) and
  the tables against float64, then ``recommend_array`` against the float64 ranking of the trained tables wherever
  two neighbouring scores lie further apart than an f32 dot product of h terms can move them."""
  from recoder_amd.data import UsersInteractions
  m, X0, Y0 = U.big_problem()
  X, Y, hist = U.fit(m, X0, Y0, 0.1, 0.01, 1.0, U.BIG_BLOCK, U.BIG_SWEEPS)
  rec = _recoder(U.BIG_H)
  got = rec.train_ials(_dataset(m), num_sweeps=U.BIG_SWEEPS, block_size=U.BIG_BLOCK, alpha0=0.1, reg=0.01,
                       init_std=0.5, seed=4)
  Xg = rec.model.user_embedding_layer.weight.data.cpu().numpy()
  Yg = rec.model.item_embedding_layer.weight.data.cpu().numpy()
  errs = [abs(a - b) / b for a, b in zip(got, hist)]
  tabs = [_rel(Xg, X), _rel(Yg, Y)]
  print("h = 520: L errors", errs, "bound", 4 * BIG_F32_ERR[1], "tables", tabs, "bound", 4 * BIG_F32_ERR[0])
  assert max(errs) <= 4 * BIG_F32_ERR[1] and max(tabs) <= 4 * BIG_F32_ERR[0]
  k = 10
  ids = rec.recommend_array(UsersInteractions(np.arange(m.shape[0]), m), k)
  S = Xg.astype(np.float64) @ Yg.astype(np.float64).T
  # an f32 dot product of h terms, in any order, is within h 2^-24 sum |x_k y_k| of the exact one (to first order)
  thr = U.BIG_H * 2.0 ** -24 * (np.abs(Xg).astype(np.float64) @ np.abs(Yg).astype(np.float64).T).max()
  for u in range(m.shape[0]):
    S[u, m.indices[m.indptr[u]:m.indptr[u + 1]]] = -np.inf
  order = np.argsort(-S, axis=1, kind="stable")[:, :k + 1]
  top = np.take_along_axis(S, order, 1)
  sure = np.logical_and.accumulate(top[:, :k] - top[:, 1:] > 2 * thr, axis=1)    # (decided up to the first close pair)
  print("h = 520: %.1f %% of the top-%d positions decided" % (100 * sure.mean(), k))
  assert sure.mean() >= 0.9
  assert np.array_equal(ids[sure], order[:, :k][sure])
