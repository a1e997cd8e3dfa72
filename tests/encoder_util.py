"""Plain restatements for tests/test_encoder_fwd.py, tests/test_encoder_bwd.py and tests/test_row_kernels.py: the
counter-RNG keep draw of csrc/common.h in numpy uint64, the encoder forward and backward of csrc/encoder.hip in
float64, the backward's host dispatch, and the hand-made CSRs the encoder tests collate.  Nothing here touches the
GPU."""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)

ACT_NONE, ACT_TANH, ACT_SIGMOID, ACT_RELU, ACT_SELU, ACT_ELU = range(6)
ACTS = (ACT_NONE, ACT_TANH, ACT_SIGMOID, ACT_RELU, ACT_SELU, ACT_ELU)
SELU_A = 1.6732632423543772848170429916717
SELU_S = 1.0507009873554804934193349852946


def gamma(k):
  """gamma_k = k u / (1 - k u): the bound of a chain of k fp32 roundings."""
  return k * U / (1.0 - k * U)


# ------------------------------------------------------------------ counter RNG
def _u64(x):
  return np.asarray(x, dtype=np.uint64)


def mix64(z):
  """rk_mix64: wrapping 64-bit arithmetic."""
  z = _u64(z)
  with np.errstate(over="ignore"):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
  return z ^ (z >> np.uint64(31))


def keep_uniform(seed, step, a, b):
  """The 24-bit uniform of rk_keep_draw as float32 in [0, 1)."""
  with np.errstate(over="ignore"):
    z = mix64(_u64(seed) + np.uint64(0x9e3779b97f4a7c15) * (_u64(step) + np.uint64(1)))
    z = mix64(z ^ (_u64(a) * np.uint64(0xd1342543de82ef95) + _u64(b) + np.uint64(0x632be59bd9b4e019)))
  return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_draw(seed, step, a, b, p):
  """rk_keep_draw: kept iff u >= p, compared in float32."""
  return keep_uniform(seed, step, a, b) >= np.float32(p)


def keep_scale(p):
  """1 / (1 - p) as the host forms it: 1 - p in double, one conversion, an fp32 reciprocal."""
  return np.float32(1.0) / np.float32(1.0 - float(np.float32(p)))


# ------------------------------------------------------------- float64 encoder
def act64(x, act):
  x = np.asarray(x, dtype=np.float64)
  if act == ACT_TANH:
    return np.tanh(x)
  if act == ACT_SIGMOID:
    return 1.0 / (1.0 + np.exp(-x))
  if act == ACT_RELU:
    return np.where(x > 0, x, 0.0)
  if act == ACT_SELU:
    return SELU_S * np.where(x > 0, x, SELU_A * np.expm1(np.minimum(x, 0.0)))
  if act == ACT_ELU:
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
  return x


def svals64(indptr, vals, keep, p, norms=None):
  """s_j = v_j / max(||v_r||, 1e-12) * keep_j / (1 - p) per stored entry, in float64 (the scale constant
  as keep_scale forms it).  norms: per-row norm to use instead of the row's own."""
  v = np.asarray(vals, dtype=np.float64)
  s = np.zeros_like(v)
  scale = float(keep_scale(p)) if p > 0 else 1.0
  for r in range(len(indptr) - 1):
    a, b = int(indptr[r]), int(indptr[r + 1])
    nrm = float(norms[r]) if norms is not None else np.sqrt(np.sum(v[a:b] * v[a:b]))
    s[a:b] = v[a:b] / max(nrm, 1e-12) * scale
  if p > 0 and keep is not None:
    s = s * (np.asarray(keep) != 0)
  return s


def encode64(indptr, gcols, s, W, b=None, act=ACT_NONE):
  """(Z, A): Z[r] = act(sum_j s_j W[item_j] + b) in float64 and A[r] = sum_j |s_j| |W[item_j]| + |b|,
  the magnitude the rounding bound of the fp32 accumulation multiplies."""
  W = np.asarray(W, dtype=np.float64)
  s = np.asarray(s, dtype=np.float64)
  R, h = len(indptr) - 1, W.shape[1]
  Z = np.zeros((R, h))
  A = np.zeros((R, h))
  for r in range(R):
    a, e = int(indptr[r]), int(indptr[r + 1])
    rows = W[np.asarray(gcols[a:e], dtype=np.int64)]
    Z[r] = s[a:e] @ rows
    A[r] = np.abs(s[a:e]) @ np.abs(rows)
  if b is not None:
    Z += np.asarray(b, dtype=np.float64)
    A += np.abs(np.asarray(b, dtype=np.float64))
  return act64(Z, act), A


# -------------------------------------------------------------- exact-length CSR
def csr_with_row_lengths(lengths, users, n_users, n_items, seed, ratings=False):
  """A [n_users, n_items] CSR whose row users[i] holds exactly lengths[i] distinct items (every other
  row is empty); values 1.0, or random ratings in (0.5, 5]."""
  rng = np.random.RandomState(seed)
  rows, cols = [], []
  for u, n in zip(users, lengths):
    c = np.sort(rng.choice(n_items, size=int(n), replace=False))
    rows.append(np.full(int(n), int(u), dtype=np.int64))
    cols.append(c)
  rows, cols = np.concatenate(rows), np.concatenate(cols)
  vals = (0.5 + 4.5 * rng.rand(len(cols))).astype(np.float32) if ratings else np.ones(len(cols), np.float32)
  m = sp.csr_matrix((vals, (rows, cols)), shape=(n_users, n_items))
  m.sort_indices()
  return m


def csr_with_column_rows(n_rows, n_items, col_rows, seed=0, ratings=False):
  """A [n_rows, n_items] CSR whose column `item` holds exactly the rows col_rows[item] (every other column is
  empty); values 1.0, or random ratings in (0.5, 5]."""
  rows = np.concatenate([np.asarray(r, dtype=np.int64) for r in col_rows.values()])
  cols = np.concatenate([np.full(len(r), int(c), dtype=np.int64) for c, r in col_rows.items()])
  rng = np.random.RandomState(seed)
  vals = (0.5 + 4.5 * rng.rand(len(cols))).astype(np.float32) if ratings else np.ones(len(cols), np.float32)
  m = sp.csr_matrix((vals, (rows, cols)), shape=(n_rows, n_items))
  m.sort_indices()
  assert m.nnz == len(cols), "a (row, column) pair was listed twice"
  return m


# ------------------------------------------------------------- float64 encoder backward
def act_dy64(y, act):
  """act'(x) written in the OUTPUT y = act(x), in float64: the formulas of rk_act_dy (csrc/common.h), which
  rk_act_grad and the slab reduces apply."""
  y = np.asarray(y, dtype=np.float64)
  if act == ACT_TANH:
    return 1.0 - y * y
  if act == ACT_SIGMOID:
    return (1.0 - y) * y
  if act == ACT_RELU:
    return np.where(y > 0, 1.0, 0.0)
  if act == ACT_SELU:
    return np.where(y > 0, SELU_S, y + SELU_S * SELU_A)
  if act == ACT_ELU:
    return np.where(y > 0, 1.0, y + 1.0)
  return np.ones_like(y)


def encode_bwd64(indptr, cols, s, dZ, row_off, B, n_b):
  """(G, A, n, gb, gA) of rows [row_off, row_off + B) of a block in float64: G[c] = sum_r s[r, c] dZ[r - row_off],
  A[c] = sum_r |s[r, c]| |dZ[r - row_off]| (the magnitude the rounding bound multiplies), n[c] = the column's stored
  entries in the window (dropped ones included), gb = the column sums of dZ and gA those of |dZ|."""
  indptr = np.asarray(indptr, dtype=np.int64)
  lo, hi = int(indptr[row_off]), int(indptr[row_off + B])
  ip = indptr[row_off:row_off + B + 1] - lo
  c = np.asarray(cols[lo:hi], dtype=np.int64)
  sv = np.asarray(s[lo:hi], dtype=np.float64)
  dz = np.asarray(dZ, dtype=np.float64)
  S = sp.csr_matrix((sv, c, ip), shape=(B, n_b))
  G = np.asarray(S.T.dot(dz))
  A = np.asarray(abs(S).T.dot(np.abs(dz)))
  n = np.bincount(c, minlength=n_b).astype(np.int64)
  return G, A, n, dz.sum(0), np.abs(dz).sum(0)


BWD_WINDOW = 4064         # rows per window of the window recursion (127 bitmap words)


def bwd_route(blk, row_off, B, h):
  """(route, HV, light): the kernel rk_ae_encode_bwd (csrc/encoder.hip) launches for rows [row_off, row_off + B)
  of a block (anything with n_cap and nnz_cap), restated from the host entry's conditions.  route is "cols1" /
  "cols2" (a wave per column, one / two bitmap words per lane), "windows" (the recursion over windows of
  BWD_WINDOW rows) or "wg" (a workgroup per column); light only selects a kernel on the cols routes."""
  hv = -(-h // 256)
  HV = 1 if hv == 1 else 2 if hv == 2 else 4
  words = ((row_off + B + 31) >> 5) - (row_off >> 5)
  light = blk.n_cap >= 4096 and blk.nnz_cap <= 2 * blk.n_cap
  if words <= 64:
    return "cols1", HV, light
  if blk.n_cap >= 4096:
    return ("cols2" if words <= 128 else "windows"), HV, light
  return "wg", HV, False


def ulp_distance(got, ref64):
  """|got - ref| in units of the fp32 spacing at ref (got: float32, ref: float64)."""
  ref32 = np.asarray(ref64, dtype=np.float64).astype(np.float32)
  sp_ = np.spacing(np.abs(ref32)).astype(np.float64)
  return np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)) / sp_
