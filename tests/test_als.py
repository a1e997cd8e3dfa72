"""GPU: implicit-feedback ALS (recoder_amd/als.py, librecoder_als.so) against the float64 restatement
of tests/als_util.py -- the Gram, one half-step on every path (stashed / streamed factor rows, G from
LDS / from memory), row ranges, the objective, a fit on the ML-20M slice and what the trained tables
plug into (checkpoints, Adam fine-tuning, the similarity index) -- and, without a measured tolerance, the solve
byte for byte against the f32 restatement in the kernels' order at both ends of every NT, the Gram on integer
tables, the objective within a counted rounding bound."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import als_util

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _slice():
  z = np.load(os.path.join(als_util.HERE, "golden", "real_ml20m_slice.npz"))
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


# ---------------------------------------------------------------------- gram
@pytest.mark.parametrize("rows", [0, 1, 37, 20108])
@pytest.mark.parametrize("h", [1, 7, 64, 200, 512])
def test_gram_against_float64(rows, h):
  from recoder_amd import als
  rng = np.random.RandomState(rows * 7 + h)
  F = rng.randn(rows, h).astype(np.float32)
  w = rng.randn(rows).astype(np.float32)
  reg = 3.5
  Ft, wt = _t(F).reshape(rows, h), _t(w)
  G, v = als.gram(Ft, reg, wt)
  G2, v2 = als.gram(Ft, reg, wt)
  Gs, s = als.gram(Ft, reg, None)
  G, v, G2, v2, Gs, s = (x.cpu().numpy() for x in (G, v, G2, v2, Gs, s))
  F64 = F.astype(np.float64)
  want = F64.T @ F64 + reg * np.eye(h)
  bound = 1e-6 * np.sqrt(max(rows, 1)) * (np.abs(F64).T @ np.abs(F64)) + 1e-6 * reg * np.eye(h)
  assert np.all(np.abs(G - want) <= bound)
  assert np.array_equal(G, G.T), "G not bitwise symmetric"
  assert np.array_equal(G, G2) and np.array_equal(v, v2), "not bitwise repeatable"
  assert np.array_equal(G, Gs)
  vb = 1e-6 * np.sqrt(max(rows, 1)) * (np.abs(F64).T @ np.abs(w.astype(np.float64))) + 1e-30
  assert np.all(np.abs(v - F64.T @ w) <= vb)
  sb = 1e-6 * np.sqrt(max(rows, 1)) * np.abs(F64).sum(0) + 1e-30
  assert np.all(np.abs(s - F64.sum(0)) <= sb)


# ------------------------------------------------------------------ half-step
def _problem(h, alpha, nonzero_bias, values, seed=0, n_users=90, n_items=70, long_row=0):
  csr = als_util.random_csr(n_users, n_items, 0.12, seed, values=values, empty_rows=(0, 5))
  if long_row:
    # one row of long_row interactions over a wider catalogue (the streaming path at h = 200)
    n_items = max(n_items, long_row + 10)
    rng = np.random.RandomState(seed + 1)
    lil = sp.lil_matrix((n_users, n_items), dtype=np.float32)
    lil[:, :csr.shape[1]] = csr
    cols = np.sort(rng.choice(n_items, long_row, replace=False))
    lil.rows[7] = list(cols)
    lil.data[7] = [1.0] * long_row
    # and one of 300: past every LDS stash at h >= 64, below the multi-wave threshold (512)
    mid = np.sort(rng.choice(n_items, 300, replace=False))
    lil.rows[8] = list(mid)
    lil.data[8] = [2.0] * 300
    csr = lil.tocsr()
    csr.sort_indices()
  rng = np.random.RandomState(seed + 2)
  X = (0.1 * rng.randn(n_users, h)).astype(np.float32)
  Y = (0.1 * rng.randn(n_items, h)).astype(np.float32)
  b = (0.3 * rng.randn(n_items)).astype(np.float32) if nonzero_bias else np.zeros(n_items, np.float32)
  return csr, X, Y, b


def _gpu_half_step(csr, F, X, b, alpha, reg, cg_steps, side, flags=0, row_lo=0, row_hi=None):
  from recoder_amd import als
  c = als.AlsCSR(csr, DEV)
  Ft, Xt, bt = _t(F), _t(X), _t(b)
  G, v = als.gram(Ft, reg, bt if side == "user" else None)
  als.solve(c, Ft, G, v, Xt, alpha, cg_steps, col_bias=bt if side == "user" else None,
            row_bias=bt if side == "item" else None, row_lo=row_lo, row_hi=row_hi, flags=flags)
  return Xt.cpu().numpy()


def _rel(got, want):
  return np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)


@pytest.mark.parametrize("h", [8, 64, 200])
@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("nonzero_bias", [False, True])
@pytest.mark.parametrize("values", ["binary", "counts"])
def test_half_step_against_float64(h, alpha, nonzero_bias, values):
  from recoder_amd import _als_lib
  csr, X, Y, b = _problem(h, alpha, nonzero_bias, values)
  reg = 5.0
  for side, M, F, rows in (("user", csr, Y, X), ("item", csr.T.tocsr(), X, Y)):
    want = als_util.half_step(M, F, rows, b, alpha, reg, 3, side)
    outs = [_gpu_half_step(M, F, rows, b, alpha, reg, 3, side, flags=f)
            for f in (0, _als_lib.FORCE_STREAM, _als_lib.G_GLOBAL, _als_lib.FORCE_STREAM | _als_lib.G_GLOBAL)]
    for f, got in zip((0, 1, 2, 3), outs):
      assert _rel(got, want) <= 1e-4, (side, f, _rel(got, want))
      assert np.array_equal(got, outs[0]), ("paths differ", side, f)


def test_half_step_long_row_streams():
  """A 5 000-interaction row at h = 200 (the multi-wave path of long rows) and a 300-interaction one (one
  wave, streamed: longer than the LDS stash)."""
  h = 200
  csr, X, Y, b = _problem(h, 10.0, True, "binary", n_users=12, n_items=60, long_row=5000)
  want = als_util.half_step(csr, Y, X, b, 10.0, 5.0, 3, "user")
  got = _gpu_half_step(csr, Y, X, b, 10.0, 5.0, 3, "user")
  assert _rel(got, want) <= 1e-4
  assert _rel(got[7], want[7]) <= 1e-4 and _rel(got[8], want[8]) <= 1e-4
  item = _gpu_half_step(csr.T.tocsr(), X, Y, b, 10.0, 5.0, 3, "item")
  assert _rel(item, als_util.half_step(csr.T.tocsr(), X, Y, b, 10.0, 5.0, 3, "item")) <= 1e-4


@pytest.mark.parametrize("h", [8, 64])
def test_half_step_many_cg_steps_is_the_exact_solve(h):
  csr, X, Y, b = _problem(h, 10.0, True, "counts", seed=3)
  for side, M, F, rows in (("user", csr, Y, X), ("item", csr.T.tocsr(), X, Y)):
    want = als_util.half_step(M, F, rows, b, 10.0, 5.0, 0, side, exact=True)
    got = _gpu_half_step(M, F, rows, b, 10.0, 5.0, 3 * h, side)
    assert _rel(got, want) <= 1e-3, (side, _rel(got, want))


def test_empty_rows_with_zero_bias_go_to_zero():
  csr, X, Y, b = _problem(8, 10.0, False, "binary")
  got = _gpu_half_step(csr, Y, X, b, 10.0, 5.0, 24, "user")
  assert np.abs(got[0]).max() < 1e-5 * np.abs(X[0]).max() and np.abs(got[5]).max() < 1e-5 * np.abs(X[5]).max()


# ------------------------------------------------------------------ row range
@pytest.mark.parametrize("h", [8, 200])
def test_row_range_is_bitwise_the_full_solve(h):
  csr, X, Y, b = _problem(h, 10.0, True, "counts", seed=5, long_row=3000 if h == 200 else 0)
  full = _gpu_half_step(csr, Y, X, b, 10.0, 5.0, 3, "user")
  lo, hi = 3, 41
  part = _gpu_half_step(csr, Y, X, b, 10.0, 5.0, 3, "user", row_lo=lo, row_hi=hi)
  assert np.array_equal(part[lo:hi], full[lo:hi])
  assert np.array_equal(part[:lo], X[:lo]) and np.array_equal(part[hi:], X[hi:])


def _fit_tables(seed, x, h=16, iters=2):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  torch.manual_seed(seed)
  rec = Recoder(model=MatrixFactorization(h), loss="mse", loss_params={"confidence": 10.0}, optimizer_type="adam")
  hist = rec.train_als(RecommendationDataset(x), num_iterations=iters, reg=100.0, cg_steps=3)
  m = rec.model
  return rec, hist, m.user_embedding_layer.weight.detach().cpu().numpy(), \
      m.item_embedding_layer.weight.detach().cpu().numpy()


def test_two_fits_from_one_seed_are_bitwise_equal():
  x, _ = _slice()
  _, h1, X1, Y1 = _fit_tables(0, x)
  _, h2, X2, Y2 = _fit_tables(0, x)
  assert np.array_equal(X1, X2) and np.array_equal(Y1, Y2) and h1 == h2


# ------------------------------------------------------------------ objective
def test_objective_matches_the_dense_mse_loss():
  """On a small problem with b != 0: L from the kernels equals MSELoss(confidence, 'sum') on the dense
  output in float64 plus the reg term, and the fit's history agrees with the restatement."""
  from recoder_amd import als
  from recoder_amd.losses import MSELoss
  csr, X, Y, b = _problem(24, 10.0, True, "counts", seed=7)
  alpha, reg = 10.0, 2.0
  Xt, Yt, bt = _t(X), _t(Y), _t(b)
  uc, ic = als.csr_pair(csr, csr.shape[0], csr.shape[1], DEV)
  Gx, sx = als.gram(Xt, reg)
  Gy, cy = als.gram(Yt, reg, bt)
  out = torch.zeros(1, dtype=torch.float64, device=DEV)
  als.objective(uc, Xt, Yt, bt, alpha, reg, Gx, sx, Gy, cy, out)
  X64, Y64, b64 = (torch.as_tensor(a, dtype=torch.float64) for a in (X, Y, b))
  R = torch.as_tensor(np.asarray(csr.todense()), dtype=torch.float64)
  want = MSELoss(confidence=alpha, reduction="sum")(X64 @ Y64.T + b64, R) + reg * ((X64 ** 2).sum() + (Y64 ** 2).sum())
  assert abs(out.item() - want.item()) <= 1e-5 * abs(want.item())
  hist = als.fit(Xt, Yt, bt, uc, ic, alpha, reg, 3, 3)
  _, _, want_hist = als_util.fit(csr, X, Y, b, alpha, reg, 3, 3)
  np.testing.assert_allclose(hist, want_hist, rtol=1e-4)


# ------------------------------------------------------------ bit for bit / exact
# The comparisons below carry no measured tolerance: the solve equals tests/als_util.solve_row32 (the kernels' own
# order of f32 operations) byte for byte, the Gram equals an integer product, the objective lies within a counted
# float64 rounding bound.  tests/test_als_host.py ties those restatements to the float64 model.
BITS_HS = [1, 64, 65, 90, 91, 128, 129, 256, 257, 512]     # both ends of every NT of dispatch_nt; G in LDS up to 90
BITS_COLS = 900
BITS_REG = 3.0
X_PAD = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]      # what the padding of X holds before and after
VARIANTS = ((10.0, True), (10.0, False), (0.0, True))            # (alpha, CSR values given; False: data = NULL)


def _bits_lengths(h):
  """Row lengths around SOLVE_UNROLL (4), the LDS stash and LONG_ROW_MIN (512).  Rows 0 and 1 and the last two are
  long ones; the first and the last lie outside [row_lo, row_hi) = [1, rows - 1)."""
  s = als_util.stash_rows(h)
  return [777, 512, 0, 1, 3, 4, 5] + ([s, s + 1] if s <= 511 else []) + [511, 777, 513, 512]


@functools.lru_cache(maxsize=None)
def _bits_problem(h):
  """alpha, the CSR values and the biases carry few bits, so coef = (1 + a) val - a b is exact however the compiler
  contracts it; F, X, G and v are generic f32.  G comes from the host: the solve does not depend on the Gram."""
  rng = np.random.RandomState(1000 + h)
  lens = _bits_lengths(h)
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  indices = np.concatenate([np.sort(rng.choice(BITS_COLS, n, replace=False)) for n in lens]).astype(np.int32)
  nnz = len(indices)
  vals = np.where(rng.rand(nnz) < 0.75, rng.randint(1, 17, nnz), rng.randint(-16, 1, nnz)) / 2.0
  csr = sp.csr_matrix((vals.astype(np.float32), indices, indptr), shape=(len(lens), BITS_COLS))
  ones = sp.csr_matrix((np.ones(nnz, np.float32), indices, indptr), shape=csr.shape)
  F = (0.1 * rng.randn(BITS_COLS, h)).astype(np.float32)
  X = (0.1 * rng.randn(len(lens), h)).astype(np.float32)
  F64 = F.astype(np.float64)
  G = F64.T @ F64 + BITS_REG * np.eye(h)
  G = (0.5 * (G + G.T)).astype(np.float32)
  v = rng.randn(h).astype(np.float32)
  col_bias = (rng.randint(-255, 256, BITS_COLS) / 256.0).astype(np.float32)
  row_bias = (rng.randint(-255, 256, len(lens)) / 256.0).astype(np.float32)
  return dict(lens=lens, csr=csr, ones=ones, F=F, X=X, G=G, v=v, col_bias=col_bias, row_bias=row_bias)


def _side_biases(p, side):
  return (p["col_bias"] if side == "user" else None), (p["row_bias"] if side == "item" else None)


@functools.lru_cache(maxsize=None)
def _bits_want(h, side, alpha, use_data):
  """{row: [x after 1, 2, 3 CG steps]} of the rows in range (computed once, shared by the cg_steps cases)."""
  p = _bits_problem(h)
  cb, rb = _side_biases(p, side)
  return als_util.solve32(p["csr"], p["F"], p["G"], p["v"], p["X"], alpha, 3, col_bias=cb, row_bias=rb,
                          rows=range(1, len(p["lens"]) - 1), use_data=use_data)


def _padded(a, pad, fill):
  out = np.full((a.shape[0], a.shape[1] + pad), fill, np.float32)
  out[:, :a.shape[1]] = a
  return out


def _solve_padded(csr, F, G, v, X, alpha, cg_steps, cb, rb, row_lo, row_hi, flags):
  """rk_als_solve on tables with ldf = h + 3 (NaN in the padding: a read of it poisons the row) and ldx = h + 5
  (X_PAD in the padding); returns the whole padded X."""
  from recoder_amd import als
  h = F.shape[1]
  Ft, Xt = _t(_padded(F, 3, np.nan)), _t(_padded(X, 5, X_PAD))
  als.solve(als.AlsCSR(csr, DEV), Ft[:, :h], _t(G), _t(v), Xt[:, :h], alpha, cg_steps,
            col_bias=None if cb is None else _t(cb), row_bias=None if rb is None else _t(rb),
            row_lo=row_lo, row_hi=row_hi, flags=flags)
  return Xt.cpu().numpy()


@pytest.mark.parametrize("cg_steps", [1, 3])
@pytest.mark.parametrize("side", ["user", "item", "no bias"])
@pytest.mark.parametrize("h", BITS_HS)
def test_solve_equals_the_f32_restatement_bit_for_bit(h, side, cg_steps):
  p = _bits_problem(h)
  lens, X = p["lens"], p["X"]
  rows = len(lens)
  cb, rb = _side_biases(p, side)
  before = _padded(X, 5, X_PAD)
  for alpha, use_data in VARIANTS:
    want = _bits_want(h, side, alpha, use_data)
    csr = p["csr"] if use_data else p["ones"]
    outs = [_solve_padded(csr, p["F"], p["G"], p["v"], X, alpha, cg_steps, cb, rb, 1, rows - 1, f) for f in (0, 1, 2, 3)]
    got = outs[0]
    wrong = [(r, lens[r]) for r in range(1, rows - 1) if got[r, :h].tobytes() != want[r][cg_steps - 1].tobytes()]
    assert wrong == [], ("(row, entries) that differ from solve_row32", alpha, use_data, wrong)
    assert got[0].tobytes() == before[0].tobytes() and got[-1].tobytes() == before[-1].tobytes(), "row out of range"
    assert got[:, h:].tobytes() == before[:, h:].tobytes(), "padding of X written"
    for f in (1, 2, 3):
      assert outs[f].tobytes() == got.tobytes(), ("flags change the bits", alpha, use_data, f)


def test_solve_stop_rules():
  """rs == 0 (an empty row at x = +0 with b = 0: no 0 / 0), a NaN in x (rs > 0 is false: the row is left as it is
  and no other row sees it) and p . q == 0 at rs > 0 (G = 0, the singular case of reg = 0: !(pq > 0) ends the loop)."""
  h = 65
  p = _bits_problem(h)
  lens, rows = p["lens"], len(p["lens"])
  empty, nan_row = lens.index(0), lens.index(5)
  zero_v = np.zeros(h, np.float32)
  X = p["X"].copy()
  X[empty] = 0.0
  run = lambda X, G, v: _solve_padded(p["csr"], p["F"], G, v, X, 10.0, 3, None, None, 0, rows, 0)[:, :h]
  clean = run(X, p["G"], zero_v)
  assert clean[empty].tobytes() == np.zeros(h, np.float32).tobytes()                     # bitwise +0
  Xn = X.copy()
  Xn[nan_row, 7] = np.nan
  got = run(Xn, p["G"], zero_v)
  lo, hi = p["csr"].indptr[nan_row], p["csr"].indptr[nan_row + 1]
  want = als_util.solve_row32(p["csr"].indices[lo:hi], p["csr"].data[lo:hi], p["F"], p["G"], zero_v, Xn[nan_row], 10.0, 3)
  assert got[nan_row].tobytes() == want.tobytes() == Xn[nan_row].tobytes()
  others = [r for r in range(rows) if r != nan_row]
  assert got[others].tobytes() == clean[others].tobytes()
  assert np.isfinite(got[others]).all()
  # G = 0: on the empty row q = G p = 0 and p . q = 0 while rs = |v|^2 > 0; x stays where it was
  zero_G = np.zeros((h, h), np.float32)
  got = run(p["X"], zero_G, p["v"])
  assert got[empty].tobytes() == p["X"][empty].tobytes()
  for r in (empty, lens.index(3), lens.index(513)):
    lo, hi = p["csr"].indptr[r], p["csr"].indptr[r + 1]
    want = als_util.solve_row32(p["csr"].indices[lo:hi], p["csr"].data[lo:hi], p["F"], zero_G, p["v"], p["X"][r], 10.0, 3)
    assert got[r].tobytes() == want.tobytes()


@pytest.mark.parametrize("h", [1, 31, 32, 33, 65, 512])
@pytest.mark.parametrize("rows", [1, 2, 511, 512, 513, 1025, 20108, 32770])
def test_gram_exact_on_integer_tables(rows, h):
  """F in {-3 .. 3}, w in {-2 .. 2}, an integer reg: every partial sum of any order is an integer below 2^24, so G
  and v must EQUAL the integer product.  A row dropped or doubled at a chunk boundary cannot pass (rows = 513 is two
  chunks of 258, 32770 is 64 of 514), nor can a read of the NaN padding (ldf = h + 3)."""
  from recoder_amd import als
  rng = np.random.RandomState(rows + 31 * h)
  F = rng.randint(-3, 4, (rows, h)).astype(np.float32)
  w = rng.randint(-2, 3, rows).astype(np.float32)
  reg = 3
  Ft, wt = _t(_padded(F, 3, np.nan))[:, :h], _t(w)
  assert Ft.stride(0) == h + 3
  G, v = (x.cpu().numpy() for x in als.gram(Ft, reg, wt))
  Gs, s = (x.cpu().numpy() for x in als.gram(Ft, reg, None))
  Gi, vi = als_util.gram_exact(F, w, reg)
  assert np.array_equal(G, Gi) and np.array_equal(G, G.T)
  assert np.array_equal(v, vi)
  assert np.array_equal(Gs, Gi) and np.array_equal(s, F.astype(np.int64).sum(0))


def _objective_case(rows, h, alpha, with_bias, use_data, seed):
  """(kernel's L, objective_parts' L, its bound) on padded tables, the Grams built on the host."""
  from recoder_amd import als
  cols, reg = 70, 2.0
  rng = np.random.RandomState(seed)
  csr = als_util.random_csr(rows, cols, 0.05, seed, values="counts", empty_rows=(1,)) if rows else \
      sp.csr_matrix((0, cols), dtype=np.float32)
  if not use_data:
    csr.data[:] = 1.0
  X, Y = (0.3 * rng.randn(rows, h)).astype(np.float32), (0.3 * rng.randn(cols, h)).astype(np.float32)
  b = (0.3 * rng.randn(cols)).astype(np.float32) if with_bias else None
  X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
  Gx, Gy = (X64.T @ X64 + reg * np.eye(h)).astype(np.float32), (Y64.T @ Y64 + reg * np.eye(h)).astype(np.float32)
  sx = X64.sum(0).astype(np.float32)
  cy = (Y64.T @ b.astype(np.float64)).astype(np.float32) if with_bias else Y64.sum(0).astype(np.float32)
  Xt = _t(_padded(X, 5, np.nan))[:, :h] if rows else torch.empty(0, h, dtype=torch.float32, device=DEV)
  Yt = _t(_padded(Y, 3, np.nan))[:, :h]
  out = torch.full((1,), np.nan, dtype=torch.float64, device=DEV)
  als.objective(als.AlsCSR(csr, DEV), Xt, Yt, None if b is None else _t(b), alpha, reg, _t(Gx), _t(sx), _t(Gy),
                _t(cy), out)
  want, bound = als_util.objective_parts(csr, X, Y, b, alpha, reg, Gx, sx, Gy, cy)
  return out.item(), want, bound


@pytest.mark.parametrize("use_data", [True, False])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 10.0])
@pytest.mark.parametrize("h", [1, 65, 200, 300, 512])
def test_objective_against_float64_at_every_nt(h, alpha, with_bias, use_data):
  """300 rows (thread t of the final kernel adds part[t] and part[t + 256]), ldx = h + 5 and ldy = h + 3 with NaN in
  the padding.  The bound is counted (als_util.objective_parts), not measured; the largest |error| / bound seen on
  the MI355X was 0.054 at h = 1, 0.022 at 65, 0.0045 at 200, 0.0015 at 300 and 0.00033 at 512."""
  got, want, bound = _objective_case(300, h, alpha, with_bias, use_data, seed=11 + h)
  print("objective h = %d alpha = %g bias = %s data = %s: |error| / bound = %.3g" %
        (h, alpha, with_bias, use_data, abs(got - want) / bound))
  assert abs(got - want) <= bound


def test_objective_with_no_rows():
  """rows = 0: no row kernel runs; L = reg tr(Y^T Y) from the Grams alone."""
  got, want, bound = _objective_case(0, 65, 10.0, True, True, seed=5)
  assert abs(got - want) <= bound and want > 0


def _quality_run():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x, y = _slice()
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(64), loss="mse", loss_params={"confidence": 10.0}, optimizer_type="adam")
  hist = rec.train_als(RecommendationDataset(x), num_iterations=10, reg=100.0, cg_steps=3)
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=20, metrics=[Recall(k=20, normalize=True)], batch_size=500)
  return rec, hist, float(np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64))), x, y


@pytest.fixture(scope="module")
def quality():
  return _quality_run()


def test_objective_does_not_increase_on_the_slice(quality):
  rec, hist, _, _, _ = quality
  assert len(hist) == 10 and rec.als_history == hist
  assert all(np.isfinite(hist))
  for a, b in zip(hist, hist[1:]):
    assert b <= a * (1 + 1e-6), hist


def test_recall_on_the_slice(quality):
  recall = quality[2]
  print("ALS Recall@20 on the ML-20M slice: %.4f" % recall)
  assert recall >= 0.12


# ---------------------------------------------------------------- integration
def test_checkpoint_round_trip_and_keys(quality, tmp_path):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  rec, _, _, x, _ = quality
  f = rec.save_state(str(tmp_path / "als"))
  rec2 = Recoder(model=MatrixFactorization(64))
  rec2.init_from_model_file(f)
  users = np.arange(300)
  inp = UsersInteractions(users, x[users])
  assert np.array_equal(rec.recommend_array(inp, 20), rec2.recommend_array(inp, 20))
  torch.manual_seed(1)
  adam = Recoder(model=MatrixFactorization(64), loss="mse", optimizer_type="adam")
  adam.train(RecommendationDataset(x[:500]), batch_size=250, num_epochs=1)
  f2 = adam.save_state(str(tmp_path / "adam"))
  k1 = torch.load(f, map_location="cpu", weights_only=False)
  k2 = torch.load(f2, map_location="cpu", weights_only=False)
  assert sorted(k1["model"]) == sorted(k2["model"])
  assert sorted(k1) == sorted(k2)


def test_adam_fine_tuning_and_similarity_on_als_tables():
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.recommender import SimilarityRecommender
  x, _ = _slice()
  rec, _, _, Y = _fit_tables(3, x, h=32, iters=2)
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
  users = np.arange(50)
  lists = SimilarityRecommender(index, 10, n=10).recommend(UsersInteractions(users, x[users]))
  assert len(lists) == 50 and all(0 < len(l) <= 10 for l in lists)      # (a short pool gives fewer)
  rec.train(RecommendationDataset(x), batch_size=500, lr=1e-3, num_epochs=1, negative_sampling=True)
  assert np.all(np.isfinite(rec.last_epoch_losses)) and len(rec.last_epoch_losses) == 20
