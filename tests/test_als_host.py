"""CPU: the kernel-order restatements of tests/als_util.py (wave_dot32, gemv32, solve_row32, gram_plan, stash_rows,
objective_parts) pinned to something that is not the kernel: the float64 model of the same file, exact rational
sums, and the launch constants the GPU cases of tests/test_als.py rely on."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from tests import als_util

U32 = 2.0 ** -24


def _exact_dot(a, b):
  return sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("h", [1, 63, 64, 65, 129, 300, 512])
def test_wave_dot32_against_the_exact_sum(h):
  """NT fmaf roundings on a lane's chain and 6 butterfly additions: |got - exact| <= gamma(NT + 6) sum |a_k b_k|."""
  rng = np.random.RandomState(h)
  a, b = rng.randn(3, h).astype(np.float32), rng.randn(h).astype(np.float32)
  got = als_util.wave_dot32(a, b, h)
  assert got.dtype == np.float32 and got.shape == (3,)
  n = als_util.nt_of(h) + 6
  for i in range(3):
    exact = _exact_dot(a[i], b)
    mag = _exact_dot(np.abs(a[i]), np.abs(b))
    assert abs(Fraction(float(got[i])) - exact) <= Fraction(n * U32 / (1 - n * U32)) * mag
    assert got[i] == als_util.wave_dot32(a[i], b, h)            # (a batch is its rows)


def test_wave_dot32_is_the_lane_layout():
  """h = 130: lane 0 owns k = 0 and lane 1 owns k = 1 and 65.  Lane 1's chain gives 2^-24 + 2^-24 = 2^-23 before
  the butterfly adds it to lane 0's 1: 1 + 2^-23.  One chain over k ascending would lose both (1 + 2^-24 -> 1)."""
  a = np.zeros(130, np.float32)
  a[[0, 1, 65]] = np.float32([1.0, 2.0 ** -24, 2.0 ** -24])
  assert als_util.wave_dot32(a, np.ones(130, np.float32), 130) == np.float32(1.0 + 2.0 ** -23)


@pytest.mark.parametrize("h", [1, 7, 90])
def test_gemv32_against_the_exact_sum(h):
  rng = np.random.RandomState(h)
  G, p = rng.randn(h, h).astype(np.float32), rng.randn(h).astype(np.float32)
  got = als_util.gemv32(G, p, h)
  assert got.dtype == np.float32
  for k in range(h):
    exact = _exact_dot(G[:, k], p)                              # (q_k = sum_j G[j][k] p_j: the kernel reads rows)
    mag = _exact_dot(np.abs(G[:, k]), np.abs(p))
    assert abs(Fraction(float(got[k])) - exact) <= Fraction(h * U32 / (1 - h * U32)) * mag


def _host_problem(h, seed):
  """30 x 700: short rows, and rows of 511 / 512 / 513 / 650 entries (the long kernel's from 512 on)."""
  rng = np.random.RandomState(seed)
  csr = als_util.random_csr(30, 700, 0.02, seed, values="counts", empty_rows=(0,)).tolil()
  for r, n in ((3, 511), (4, 512), (5, 513), (6, 650)):
    cols = np.sort(rng.choice(700, n, replace=False))
    csr.rows[r] = list(cols)
    csr.data[r] = list(np.where(rng.rand(n) < 0.8, rng.randint(1, 6, n), -0.5).astype(np.float32))
  csr = csr.tocsr()
  csr.sort_indices()
  X = (0.1 * rng.randn(30, h)).astype(np.float32)
  Y = (0.1 * rng.randn(700, h)).astype(np.float32)
  b = (0.3 * rng.randn(700)).astype(np.float32)
  return csr, X, Y, b


@pytest.mark.parametrize("h", [5, 70, 130])
@pytest.mark.parametrize("alpha", [0.0, 10.0])
def test_the_restatement_in_float64_is_the_model(h, alpha):
  """solve_row32's code path with dtype = float64 against normal_equations + cg, row by row, user and item side:
  relative distance <= kappa(A) h 2^-50 (the two sum in different orders; CG carries that through A)."""
  csr, X, Y, b = _host_problem(h, 3)
  reg, worst = 2.0, 0.0
  for side, M, F, T in (("user", csr, Y, X), ("item", csr.T.tocsr(), X, Y)):
    M.sort_indices()
    F64 = F.astype(np.float64)
    G = F64.T @ F64 + reg * np.eye(h)
    v = F64.T @ b.astype(np.float64) if side == "user" else F64.sum(0)
    rows = range(12) if side == "user" else np.argsort(-np.diff(M.indptr))[:6]      # (items: the longest rows)
    got = als_util.solve32(M, F64, G, v, T.astype(np.float64), alpha, 3, col_bias=b if side == "user" else None,
                           row_bias=b if side == "item" else None, rows=rows, dtype=np.float64)
    for r in rows:
      A, rhs = als_util.normal_equations(M, r, F, b, alpha, reg, side)
      want = als_util.cg(A, rhs, T[r], 3)
      bound = np.linalg.cond(A) * h * 2.0 ** -50
      rel = np.linalg.norm(got[r][-1] - want) / np.linalg.norm(want)
      worst = max(worst, rel / bound)
      assert rel <= bound, (side, r, rel, bound)
  print("h = %d alpha = %g: largest distance / (kappa h 2^-50) = %.3g" % (h, alpha, worst))


def test_history_is_the_result_at_fewer_steps():
  csr, X, Y, b = _host_problem(70, 5)
  G = (Y.astype(np.float64).T @ Y.astype(np.float64) + 2.0 * np.eye(70)).astype(np.float32)
  v = (Y.astype(np.float64).T @ b).astype(np.float32)
  together = als_util.solve32(csr, Y, G, v, X, 10.0, 3, col_bias=b, rows=(0, 1, 4))
  for r in (0, 1, 4):
    lo, hi = csr.indptr[r], csr.indptr[r + 1]
    hist = []
    x3 = als_util.solve_row32(csr.indices[lo:hi], csr.data[lo:hi], Y, G, v, X[r], 10.0, 3, col_bias=b, history=hist)
    x1 = als_util.solve_row32(csr.indices[lo:hi], csr.data[lo:hi], Y, G, v, X[r], 10.0, 1, col_bias=b)
    assert x3.dtype == np.float32 and len(hist) == 3
    assert x1.tobytes() == hist[0].tobytes() and x3.tobytes() == hist[2].tobytes()
    assert [t.tobytes() for t in together[r]] == [t.tobytes() for t in hist]     # (solve32 batches the G products only)


def test_launch_constants_the_gpu_cases_rely_on():
  assert als_util.g_in_lds(90) and not als_util.g_in_lds(91) and not als_util.g_in_lds(90, als_util.G_GLOBAL)
  assert als_util.stash_rows(90) == 23 and als_util.stash_rows(91) == 45 and als_util.stash_rows(512) == 8
  assert als_util.stash_rows(1) > 511 and als_util.stash_rows(64) == 48
  assert als_util.stash_rows(90, als_util.G_GLOBAL) == 45 and als_util.stash_rows(90, als_util.FORCE_STREAM) == 0
  assert [als_util.nt_of(h) for h in (1, 64, 65, 128, 129, 256, 257, 512)] == [1, 1, 2, 2, 4, 4, 8, 8]
  assert als_util.gram_plan(0) == (1, 0) and als_util.gram_plan(1) == (1, 2) and als_util.gram_plan(512) == (1, 512)
  assert als_util.gram_plan(513) == (2, 258) and als_util.gram_plan(1025) == (3, 342)
  assert als_util.gram_plan(20108) == (40, 504) and als_util.gram_plan(32770) == (64, 514)
  for rows in (1, 2, 511, 512, 513, 1025, 20108, 32770):
    nch, chunk = als_util.gram_plan(rows)
    assert chunk % 2 == 0 and nch * chunk >= rows > (nch - 1) * chunk         # (every chunk holds a row)


def test_gram_exact_is_the_integer_product():
  rng = np.random.RandomState(0)
  F, w = rng.randint(-3, 4, (50, 7)), rng.randint(-2, 3, 50)
  G, v = als_util.gram_exact(F.astype(np.float32), w.astype(np.float32), 4)
  assert G.dtype == np.int64 and np.array_equal(G, F.T @ F + 4 * np.eye(7, dtype=np.int64)) and np.array_equal(v, F.T @ w)
  assert np.array_equal(als_util.gram_exact(F, None, 0)[1], F.sum(0))
  with pytest.raises(AssertionError):
    als_util.gram_exact(F + 0.5, w, 4)


@pytest.mark.parametrize("with_bias", [False, True])
def test_objective_parts_is_the_dense_loss(with_bias):
  """With float64-accurate Grams rounded once to f32, objective_parts is the dense weighted loss of
  als_util.objective within 1e-5 (f32 scores, f32 Grams), and its bound is far below that."""
  rng = np.random.RandomState(2)
  csr = als_util.random_csr(40, 30, 0.15, 4, values="counts", empty_rows=(2,))
  h, alpha, reg = 70, 10.0, 2.0
  X, Y = (0.3 * rng.randn(40, h)).astype(np.float32), (0.3 * rng.randn(30, h)).astype(np.float32)
  b = (0.3 * rng.randn(30)).astype(np.float32) if with_bias else None
  X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
  Gx, Gy = (X64.T @ X64 + reg * np.eye(h)).astype(np.float32), (Y64.T @ Y64 + reg * np.eye(h)).astype(np.float32)
  sx = X64.sum(0).astype(np.float32)
  cy = (Y64.T @ b.astype(np.float64)).astype(np.float32) if with_bias else Y64.sum(0).astype(np.float32)
  L, bound = als_util.objective_parts(csr, X, Y, b, alpha, reg, Gx, sx, Gy, cy)
  want = als_util.objective(csr, X, Y, b, alpha, reg)
  assert abs(L - want) <= 1e-5 * abs(want)
  assert 0 < bound <= 1e-10 * abs(want)
  ones, _ = als_util.objective_parts(csr, X, Y, b, alpha, reg, Gx, sx, Gy, cy, use_data=False)
  m = sp.csr_matrix(csr, copy=True)
  m.data[:] = 1.0
  assert abs(ones - als_util.objective(m, X, Y, b, alpha, reg)) <= 1e-5 * abs(want)
