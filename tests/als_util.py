"""Float64 numpy restatement of implicit-feedback ALS (recoder_amd/als.py, include/recoder_als.h):
the same normal equations, the same warm-started CG with the same stopping rules, row by row -- and, below,
the kernels of csrc/als/solve.h restated in their own order of f32 operations (bit for bit)."""
import os

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))


def normal_equations(csr, r, F, bias, alpha, reg, side):
  """(A, rhs) of row r: A = F^T F + reg I + sum a_j f_j f_j^T, rhs as in include/recoder_als.h."""
  F = np.asarray(F, np.float64)
  h = F.shape[1]
  b = np.zeros(csr.shape[1] if side == "user" else csr.shape[0]) if bias is None else np.asarray(bias, np.float64)
  A = F.T @ F + reg * np.eye(h)
  lo, hi = csr.indptr[r], csr.indptr[r + 1]
  cols, vals = csr.indices[lo:hi], np.asarray(csr.data[lo:hi], np.float64)
  a = np.where(vals > 0, alpha, 0.0)
  f = F[cols]
  if side == "user":
    rhs = -(F.T @ b) + f.T @ ((1 + a) * vals - a * b[cols])
  else:
    rhs = -b[r] * F.sum(0) + f.T @ ((1 + a) * vals - a * b[r])
  A = A + (f * a[:, None]).T @ f
  return A, rhs


def cg(A, rhs, x, steps):
  x = np.array(x, np.float64)
  r = rhs - A @ x
  p = r.copy()
  rs = r @ r
  for _ in range(steps):
    if not rs > 0:
      break
    q = A @ p
    pq = p @ q
    if not pq > 0:
      break
    al = rs / pq
    x += al * p
    r -= al * q
    rsn = r @ r
    p = r + (rsn / rs) * p
    rs = rsn
  return x


def half_step(csr, F, X, bias, alpha, reg, cg_steps, side, exact=False):
  """Every row of X solved with F fixed (a new array); side 'user' (bias per column) or 'item'."""
  X = np.array(X, np.float64)
  for r in range(csr.shape[0]):
    A, rhs = normal_equations(csr, r, F, bias, alpha, reg, side)
    X[r] = np.linalg.solve(A, rhs) if exact else cg(A, rhs, X[r], cg_steps)
  return X


def objective(csr, X, Y, bias, alpha, reg):
  R = np.asarray(csr.todense(), np.float64)
  S = np.asarray(X, np.float64) @ np.asarray(Y, np.float64).T
  if bias is not None:
    S = S + np.asarray(bias, np.float64)[None, :]
  W = 1 + alpha * (R > 0)
  return float((W * (R - S) ** 2).sum() + reg * ((np.asarray(X, np.float64) ** 2).sum()
                                                   + (np.asarray(Y, np.float64) ** 2).sum()))


def fit(csr, X, Y, bias, alpha, reg, cg_steps, num_iterations):
  csr = sp.csr_matrix(csr)
  csc = csr.T.tocsr()
  X, Y = np.array(X, np.float64), np.array(Y, np.float64)
  hist = []
  for _ in range(num_iterations):
    X = half_step(csr, Y, X, bias, alpha, reg, cg_steps, "user")
    Y = half_step(csc, X, Y, bias, alpha, reg, cg_steps, "item")
    hist.append(objective(csr, X, Y, bias, alpha, reg))
  return X, Y, hist


def random_csr(n_rows, n_cols, density, seed, values="binary", empty_rows=()):
  rng = np.random.RandomState(seed)
  m = sp.random(n_rows, n_cols, density=density, random_state=rng, format="csr", dtype=np.float64)
  if values == "binary":
    m.data[:] = 1.0
  else:                     # counts and a few non-positive values (weight 1, as in MSELoss)
    m.data = np.round(m.data * 5, 1) - 0.5
    m.data[m.data == 0] = 2.0
  m = m.tolil()
  for r in empty_rows:
    m.rows[r] = []
    m.data[r] = []
  m = m.tocsr().astype(np.float32)
  m.sort_indices()
  return m


# ------------------------------------------------------------------------------------------------------------
# The kernels of recoder_amd/csrc/als/solve.h restated in their own order of operations (f32, bit for bit).
# dtype=np.float64 runs the same code path with a * b + c for fmaf: tests/test_als_host.py ties it to the model
# above, so that the restatement is more than a transliteration of the kernel.
LONG_ROW_MIN, LONG_WAVES, SOLVE_LDS_FLOATS, G_LDS_MAX_FLOATS = 512, 16, 64 * 1024 // 4, 32 * 1024 // 4
GR_MAX_CHUNKS, GR_MIN_CHUNK = 64, 512
FORCE_STREAM, G_GLOBAL = 1, 2
_LANE = np.arange(64)


def nt_of(h):
  """dispatch_nt: the registers a lane holds for a row of h floats."""
  return 1 if h <= 64 else 2 if h <= 128 else 4 if h <= 256 else 8


def gram_plan(rows):
  """(nch, chunk) of rk_als_gram: at most 64 chunks of at least 512 rows, the chunk rounded up to even."""
  nch = 1 if rows <= 0 else min(GR_MAX_CHUNKS, (rows + GR_MIN_CHUNK - 1) // GR_MIN_CHUNK)
  c = 0 if rows <= 0 else (rows + nch - 1) // nch
  return nch, (c + 1) & ~1


def g_in_lds(h, flags=0):
  return not (flags & G_GLOBAL) and h * h <= G_LDS_MAX_FLOATS


def stash_rows(h, flags=0):
  """The factor rows one wave of als_solve_kernel keeps in LDS (a longer row streams them on every step)."""
  if flags & FORCE_STREAM:
    return 0
  return (SOLVE_LDS_FLOATS - (h * h if g_in_lds(h, flags) else 0)) // 4 // h


def _fma(a, b, c, dtype):
  """fmaf(a, b, c) in f32 (exact: tests/ease_util.fmaf), a * b + c in float64.  The float64 sum of the exact
  product and c rounds to the f32 the fused operation gives unless it sits on an f32 rounding midpoint (rounding
  is monotone: off a midpoint both lie on its same side); only then ease_util.fmaf's TwoSum repair is needed."""
  if dtype != np.float32:
    return a * b + c
  s = np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
  if ((np.ascontiguousarray(s).view(np.int64) & 0x1FFFFFFF) == 0x10000000).any():
    from tests.ease_util import fmaf
    return fmaf(a, b, c)
  return s.astype(np.float32)


def wave_dot32(a, b, h, dtype=np.float32):
  """wave_dot: lane l owns k = l + 64 t; per lane one fmaf chain over t ascending from +0, then the xor butterfly
  s = s + s[lane ^ off] for off = 32 .. 1.  a, b: [..., h] (broadcast against each other); returns [...]."""
  a, b = np.broadcast_arrays(np.asarray(a, dtype), np.asarray(b, dtype))
  nt = nt_of(h)
  pad = [(0, 0)] * (a.ndim - 1) + [(0, 64 * nt - h)]
  a = np.pad(a[..., :h], pad).reshape(a.shape[:-1] + (nt, 64))
  b = np.pad(b[..., :h], pad).reshape(b.shape[:-1] + (nt, 64))
  s = np.zeros(a.shape[:-2] + (64,), dtype)
  with np.errstate(invalid="ignore", over="ignore"):
    for t in range(nt):
      s = _fma(a[..., t, :], b[..., t, :], s, dtype)
    for off in (32, 16, 8, 4, 2, 1):
      s = s + s[..., _LANE ^ off]
  assert s.dtype == dtype
  return s[..., 0]


def gemv32(G, p, h, dtype=np.float32):
  """gemv: q[k] = one fmaf(G[j][k], p[j], q[k]) chain over j ascending from +0.  p: [h], or [m, h] for m
  vectors at once (each its own chains)."""
  G, p = np.asarray(G, dtype), np.asarray(p, dtype)
  q = np.zeros(p.shape[:-1] + (h,), dtype)
  with np.errstate(invalid="ignore", over="ignore"):
    for j in range(h):
      q = _fma(G[j, :h], p[..., j:j + 1], q, dtype)
  return q


def _chain(w, f, acc, dtype):
  """acc = fmaf(w[j], f[j], acc) over j ascending."""
  for j in range(len(w)):
    acc = _fma(w[j], f[j], acc, dtype)
  return acc


def _pieces(w, f, sel, n, h, dtype):
  """The 16 waves of als_solve_long_kernel: wave i owns the entries [i piece, min(n, (i + 1) piece)), piece =
  ceil(n / 16); each wave's chain (over its entries with sel set) starts from +0.  Returns [16, h]."""
  piece = (n + LONG_WAVES - 1) // LONG_WAVES
  out = np.zeros((LONG_WAVES, h), dtype)
  for i in range(LONG_WAVES):
    jb = min(n, i * piece)
    je = min(n, jb + piece)
    idx = np.arange(jb, je)[sel[jb:je]]
    out[i] = _chain(w[idx], f[idx], out[i], dtype)
  return out


def _combine(parts, acc):
  """long_combine: the pieces added in wave order 0 .. 15."""
  for i in range(LONG_WAVES):
    acc = acc + parts[i]
  return acc


def _row_steps(cols, vals, F, v, x, alpha, cg_steps, col_bias, row_bias, dtype, history):
  """solve_row32 as a generator: it yields every vector it needs G times (x, then p of each CG step), is sent the
  product, and returns the new x.  (So that solve32 can take the products of many rows in one gemv32.)"""
  one = dtype(1)
  h = len(x)
  n = len(cols)
  alpha = dtype(alpha)
  x = np.array(x, dtype)
  f = np.asarray(F, dtype)[np.asarray(cols, np.int64), :h].reshape(n, h)
  vals = np.ones(n, dtype) if vals is None else np.asarray(vals, dtype)
  rb = dtype(0) if row_bias is None else dtype(row_bias)
  a = np.where(vals > 0, alpha, dtype(0)).astype(dtype)
  bsel = np.asarray(col_bias, dtype)[np.asarray(cols, np.int64)] if col_bias is not None else np.full(n, rb, dtype)
  coef = ((one + a) * vals - a * bsel).astype(dtype)
  live = a != 0
  long_row = n >= LONG_ROW_MIN
  allj = np.ones(n, bool)
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    r = -((rb if row_bias is not None else one) * np.asarray(v, dtype)[:h])
    q = yield x
    ad = (a * wave_dot32(f, x, h, dtype)).astype(dtype) if n else np.zeros(0, dtype)
    if long_row:
      r = _combine(_pieces(coef, f, allj, n, h, dtype), r)
      q = _combine(_pieces(ad, f, live, n, h, dtype), q)
    else:
      r = _chain(coef, f, r, dtype)
      q = _chain(ad[live], f[live], q, dtype)
    r = r - q
    p = r.copy()
    rs = wave_dot32(r, r, h, dtype)
    for _ in range(cg_steps):
      if not rs > 0:
        break
      q = yield p
      if alpha != 0:
        ad = (a * wave_dot32(f, p, h, dtype)).astype(dtype) if n else np.zeros(0, dtype)
        if long_row:
          q = _combine(_pieces(ad, f, live, n, h, dtype), q)
        else:
          q = _chain(ad[live], f[live], q, dtype)
      pq = wave_dot32(p, q, h, dtype)
      if not pq > 0:
        break
      al = dtype(rs / pq)
      x = _fma(al, p, x, dtype)
      r = _fma(-al, q, r, dtype)
      rsn = wave_dot32(r, r, h, dtype)
      beta = dtype(rsn / rs)
      p = _fma(beta, p, r, dtype)
      rs = rsn
      if history is not None:
        history.append(x.copy())
  assert x.dtype == dtype and r.dtype == dtype and p.dtype == dtype
  return x


def solve_row32(cols, vals, F, G, v, x, alpha, cg_steps, col_bias=None, row_bias=None, dtype=np.float32, history=None):
  """One row of rk_als_solve, op for op: als_solve_kernel for a row of fewer than 512 entries, als_solve_long_kernel
  from there on.  cols, vals: the row's CSR entries in order (vals None: all ones); F [>, >= h] the fixed table; G
  [h, h], v [h]; x [h] the row's current value; col_bias [columns] (user side) or row_bias (this row's own, item
  side).  Returns the new x; ``history`` (a list) receives x after every CG step taken, so that one run at
  cg_steps = 3 also gives the result at cg_steps = 1, 2."""
  steps = _row_steps(cols, vals, F, v, x, alpha, cg_steps, col_bias, row_bias, dtype, history)
  try:
    vec = next(steps)
    while True:
      vec = steps.send(gemv32(G, vec, len(x), dtype))
  except StopIteration as done:
    return done.value


def solve32(csr, F, G, v, X, alpha, cg_steps, col_bias=None, row_bias=None, rows=None, use_data=True,
            dtype=np.float32):
  """{row: [x after 1 step, ..., x after cg_steps steps]} for the given rows of the CSR (a row that stops early
  repeats its last value): solve_row32 on every row, the rows' G products taken together."""
  rows = list(range(csr.shape[0]) if rows is None else rows)
  h = np.asarray(X).shape[1]
  hist, last, steps, vec = {}, {}, {}, {}
  for r in rows:
    lo, hi = csr.indptr[r], csr.indptr[r + 1]
    hist[r] = []
    steps[r] = _row_steps(csr.indices[lo:hi], csr.data[lo:hi] if use_data else None, F, v, X[r], alpha, cg_steps,
                          col_bias, None if row_bias is None else row_bias[r], dtype, hist[r])
    vec[r] = next(steps[r])
  while vec:
    live = list(vec)
    q = gemv32(G, np.stack([vec[r] for r in live]), h, dtype)
    for i, r in enumerate(live):
      try:
        vec[r] = steps[r].send(q[i])
      except StopIteration as done:
        last[r] = done.value
        del vec[r]
  return {r: (hist[r] + [last[r]] * cg_steps)[:cg_steps] for r in rows}


def gram_exact(F, w, reg):
  """(G, v) of rk_als_gram as int64 for an integer table (|F| <= 3, |w| <= 2, rows <= 40 000, integer reg): every
  partial sum of any order lies below 2^24, so the kernel's f32 result must EQUAL these.  (The products run
  through float64 BLAS, exact at this size: int64 matmul in numpy is many times slower.)"""
  F64 = np.asarray(F, np.float64)
  assert np.array_equal(F64, np.rint(F64)) and np.abs(F64).max(initial=0) <= 3 and F64.shape[0] <= 40000
  w64 = np.ones(F64.shape[0]) if w is None else np.asarray(w, np.float64)
  assert np.array_equal(w64, np.rint(w64)) and np.abs(w64).max(initial=0) <= 2 and reg == int(reg)
  G = F64.T @ F64 + float(reg) * np.eye(F64.shape[1])
  v = F64.T @ w64
  assert np.abs(G).max() < 2 ** 24 and np.abs(v).max(initial=0) < 2 ** 24
  return G.astype(np.int64), v.astype(np.int64)


def objective_parts(csr, X, Y, bias, alpha, reg, Gx, sx, Gy, cy, use_data=True):
  """(L, bound) of rk_als_objective from its own inputs (the f32 Grams included).  s = (the wave_dot32 chain +
  b_i) in f32, as the kernel forms it; every term after that in float64, the terms summed exactly (math.fsum).
  bound >= |kernel - L| is counted, not measured: count * 2^-53 * sum |terms|."""
  import math
  csr = sp.csr_matrix(csr)
  rows, cols = csr.shape
  h = np.asarray(Y).shape[1]
  X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
  al, lam = float(np.float32(alpha)), float(np.float32(reg))
  terms, mags = [], []
  u_of = np.repeat(np.arange(rows), np.diff(csr.indptr))
  if csr.nnz:
    d = wave_dot32(Y[csr.indices, :h], X[u_of, :h], h)
    s32 = d + np.asarray(bias, np.float32)[csr.indices] if bias is not None else d
    assert s32.dtype == np.float32
    s = s32.astype(np.float64)
    val = (csr.data if use_data else np.ones(csr.nnz)).astype(np.float32).astype(np.float64)
    wt = 1.0 + np.where(val > 0, al, 0.0)
    err = val - s
    terms += [wt * err * err, -(s * s)]
    mags += [wt * err * err, s * s]
  Gx64, Gy64 = np.asarray(Gx, np.float32).astype(np.float64), np.asarray(Gy, np.float32).astype(np.float64)
  gx, gy = Gx64 - lam * np.eye(h), Gy64 - lam * np.eye(h)
  terms += [(gx * gy).ravel(), lam * (np.diag(gx) + np.diag(gy))]
  mags += [np.abs(gx * gy).ravel(), lam * (np.abs(np.diag(gx)) + np.abs(np.diag(gy)))]
  if bias is not None:
    b64 = np.asarray(bias, np.float32).astype(np.float64)
    t = 2.0 * np.asarray(sx, np.float32).astype(np.float64) * np.asarray(cy, np.float32).astype(np.float64)
    terms += [float(rows) * (b64 * b64), t]
    mags += [float(rows) * (b64 * b64), np.abs(t)]
  L = math.fsum(np.concatenate(terms))
  # The count.  A leaf (one entry's w e^2 and s^2, one gx gy, one reg (gx + gy), one rows b^2, one 2 sx cy) takes
  # at most 5 float64 roundings in the kernel before it is added: w = 1 + alpha, e = r - s, two products, the
  # subtraction of s^2 (s^2 itself is exact, a product of two f32); gx, gy, their sum, the product with reg; a
  # fused multiply-add only removes one.  After that a leaf passes through at most
  #   n_max                     additions of its row's chain over the entries (als_objective_rows_kernel)
  #   ceil(rows / 256)          of the strided partial sums of thread t: part[t], part[t + 256], ...
  #   2 ceil(h^2 / 256)         of that thread's Gram terms (gx gy, and reg (gx + gy) on the diagonal)
  #   ceil(cols / 256) + 2      of the bias' chain, its product with rows and its addition
  #   ceil(h / 256)             of the 2 sx cy terms
  #   8                         levels of the halving tree
  # each of relative error 2^-53 on a partial sum that is at most sum |leaves|.  The reference adds 6 of its own:
  # the same 5 on a leaf and the one rounding of fsum.  (First order in 2^-53; the factor 1 / (1 - count 2^-53)
  # covers the rest.)
  n_max = int(np.diff(csr.indptr).max(initial=0))
  count = 5 + n_max + -(-rows // 256) + 2 * -(-(h * h) // 256) + -(-cols // 256) + 2 + -(-h // 256) + 8 + 6
  u = 2.0 ** -53
  bound = count * u / (1 - count * u) * math.fsum(np.concatenate(mags))
  return L, bound
