"""Plain restatements for tests/test_linear_host.py and tests/test_linear_kernels.py: a hidden nn.Linear layer's
forward and backward in float64 with the sums of absolute products their rounding bounds multiply, the host's
choice of kernels (rk_linear_fwd and linear_bwd_impl of csrc/gemm.hip, rk_small_gemm_fits of csrc/linear.hip),
counted error bounds of rk_act_dy, and the generators of the shapes the GPU tests run.  Every generator asserts
that its cases reach the route and the edge it is named for.  Nothing here touches the GPU.

W is always given the way the kernels take it: [N, K] (nn.Linear), or [K, N] when `wt` (w_transposed); dW and
dW0 have W's layout."""
import numpy as np

from tests.encoder_util import (ACT_ELU, ACT_NONE, ACT_RELU, ACT_SELU, ACT_SIGMOID, ACT_TANH, ACTS, SELU_A,  # noqa: F401
                                SELU_S, U, act64, act_dy64, gamma, ulp_distance)

# Lipschitz constants of the activations (the largest |act'|)
LIPSCHITZ = {ACT_NONE: 1.0, ACT_TANH: 1.0, ACT_RELU: 1.0, ACT_ELU: 1.0, ACT_SIGMOID: 0.25, ACT_SELU: SELU_S * SELU_A}


def _f64(a):
  return np.asarray(a, dtype=np.float64)


def _wn(W, wt):
  """W as [N, K] whatever its layout."""
  return _f64(W).T if wt else _f64(W)


# ------------------------------------------------------------------ float64 layer
def linear_fwd64(X, W, b, wt, act):
  """(pre, out, S): pre = X W^T + b and out = act(pre) in float64, S = |X| |W|^T + |b|."""
  X, Wn = _f64(X), _wn(W, wt)
  pre = X @ Wn.T
  S = np.abs(X) @ np.abs(Wn).T
  if b is not None:
    pre = pre + _f64(b)
    S = S + np.abs(_f64(b))
  return pre, act64(pre, act), S


def linear_bwd64(dY, Y, X, W, wt, act, dW0=None, dx_act_y=None):
  """(dYpre, dX, dW, db, SX, SW, Sb) in float64.  dYpre = dY * act'(Y) with act' written in the OUTPUT Y, as the
  kernels take it (Y = None: dY already is dYpre, rk_linear_bwd_pre); dX = dYpre W (times act'(dx_act_y) when
  given), dW = dYpre^T X (+ dW0 when accumulating) in W's layout, db the column sums.  SX, SW and Sb are the same
  sums over absolute values (SX before the act' factor, SW with |dW0|)."""
  dYpre = _f64(dY) if Y is None else _f64(dY) * act_dy64(Y, act)
  X, Wn = _f64(X), _wn(W, wt)
  dX = dYpre @ Wn
  SX = np.abs(dYpre) @ np.abs(Wn)
  if dx_act_y is not None:
    dX = dX * act_dy64(dx_act_y, act)
  dWn = dYpre.T @ X
  SWn = np.abs(dYpre).T @ np.abs(X)
  dW, SW = (dWn.T, SWn.T) if wt else (dWn, SWn)
  if dW0 is not None:
    dW = dW + _f64(dW0)
    SW = SW + np.abs(_f64(dW0))
  return dYpre, dX, dW, dYpre.sum(0), SX, SW, np.abs(dYpre).sum(0)


# ------------------------------------------------------------------ counted bounds
def act_dy_err(y, act):
  """Absolute error bound of rk_act_dy(y) (csrc/common.h) against act_dy64(y), y an fp32 value, u = 2^-24:
    tanh    fl(1 - fl(y y)):  u y^2, then u |1 - fl(y y)|            <= u (y^2 (1 + u) + |1 - y^2|)
    sigmoid fl(fl(1 - y) y):  u |1 - y| |y|, then u |fl(1 - y) y|    <= (2 u + u^2) |(1 - y) y|
    elu     y > 0: 1 exactly; else fl(y + 1)                         <= u |y + 1|
    selu    y > 0: fl(S) for S                                       <= u S
            else fl(y + c), c = fl(fl(S) fl(A)): |c - S A| <= S A ((1 + u)^3 - 1) =: e, then u |y + c|
                                                                     <= e (1 + u) + u |y + S A|
    relu, none: 0 or 1 exactly.
  A fused multiply-add in place of two operations drops a rounding and stays inside these."""
  y = _f64(y)
  if act == ACT_TANH:
    return U * (y * y * (1 + U) + np.abs(1 - y * y))
  if act == ACT_SIGMOID:
    return (2 * U + U * U) * np.abs((1 - y) * y)
  if act == ACT_ELU:
    return np.where(y > 0, 0.0, U * np.abs(y + 1))
  if act == ACT_SELU:
    e = SELU_S * SELU_A * ((1 + U) ** 3 - 1)
    return np.where(y > 0, U * SELU_S, e * (1 + U) + U * np.abs(y + SELU_S * SELU_A))
  return np.zeros_like(y)


def times_act_dy_bound(v, ev, y, act):
  """Bound of |fl(v_hat * rk_act_dy(y)) - v * act_dy64(y)| where |v_hat - v| <= ev: the factor's own error on
  |v|, v's error on the computed factor, and the product's one rounding."""
  d, ed = np.abs(act_dy64(y, act)), act_dy_err(y, act)
  v = np.abs(_f64(v))
  return v * ed + ev * (d + ed) + U * (v + ev) * (d + ed)


def dypre_bound(dY, Y, act):
  """|dYpre_hat - dY act'(Y)| for dYpre_hat = fl(dY * rk_act_dy(Y)), dY exact."""
  return times_act_dy_bound(dY, 0.0, Y, act)


# ------------------------------------------------------------------ the host's routes
def small_fits(M, N, K):
  """rk_small_gemm_fits of csrc/linear.hip: the 32 x 32 split-K tiles take the contraction."""
  return M > 0 and N > 0 and K > 0 and N <= 1024 and K <= 4096 and (-(-M // 32)) * (-(-N // 32)) <= 4096


def route(B, N, K, wt):
  """{"fwd": (family, AMODE, BMODE), "dx": ..., "dw": ...}: the kernels rk_linear_fwd and linear_bwd_impl
  (csrc/gemm.hip) launch.  family "small" = small_gemm_kernel<AMODE, BMODE> of csrc/linear.hip (dx and dw in
  small_gemm_pair_kernel when both are asked for and RK_TUNE_LINEAR_PAIR is set), "gemm" =
  gemm_kernel<2, 2, 1, 1, AMODE, BMODE, EPI_STORE, VEC>.  The backward asks rk_small_gemm_fits twice: for dX
  [B, K] over N and for dW ([N, K] or [K, N]) over B, and takes the small kernels only if both fit."""
  fwd = ("small" if small_fits(B, N, K) else "gemm", 0, 1 if wt else 0)
  fam = "small" if small_fits(B, K, N) and small_fits(K if wt else N, N if wt else K, B) else "gemm"
  # dX = dY . Weff[N, K]: W[N, K] is k-major for it, Wst[K, N] contiguous along the reduction
  return {"fwd": fwd, "dx": (fam, 0, 0 if wt else 1), "dw": (fam, 1, 1)}


def vec_loads(B, N, K, wt, offs):
  """{"fwd": .., "dx": .., "dw": ..}: whether the 16-byte loads are taken (small route: of any operand), given the
  bases' offsets from 16-byte alignment in floats, offs = (X, W, dY)."""
  ax, aw, ay = (o % 4 == 0 for o in offs)
  r = route(B, N, K, wt)
  ldw = N if wt else K
  if r["fwd"][0] == "small":
    fwd = (ax and K % 4 == 0) or (not wt and aw and K % 4 == 0)
  else:
    fwd = ax and aw and K % 4 == 0 and ldw % 4 == 0
  if r["dx"][0] == "small":
    dx = (ay and N % 4 == 0) or (bool(wt) and aw and N % 4 == 0)
    dw = False                    # both operands k-major: straight from global memory, one value per lane
  else:
    dx = ay and aw and N % 4 == 0 and ldw % 4 == 0
    dw = ay and ax and N % 4 == 0 and K % 4 == 0
  return {"fwd": bool(fwd), "dx": bool(dx), "dw": bool(dw)}


# ------------------------------------------------------------------ operands
def int_operands(B, N, K, wt, seed, top=8):
  """Integer operands in [-top, top] as float32: any partial sum of their products is an integer below 2^24 (see
  int_sum_bound) and so exact in fp32 in any order."""
  rng = np.random.RandomState(seed)
  f = lambda *s: rng.randint(-top, top + 1, size=s).astype(np.float32)
  wshape = (K, N) if wt else (N, K)
  return dict(X=f(B, K), W=f(*wshape), b=f(N), dY=f(B, N), Y=f(B, N), dW0=f(*wshape))


def int_sum_bound(B, N, K, top=8):
  """The largest sum of absolute products any of the four contractions can reach on int_operands."""
  return max(K * top * top + top,     # forward, with the bias
             N * top * top,           # dX
             B * top * top + top,     # dW, with dW0
             B * top)                 # db


def log_uniform(rng, shape, lo=-10.0, hi=4.0):
  """Signed values with magnitudes log-uniform in [2^lo, 2^hi] as float32 (no subnormals, no zeros)."""
  mag = 2.0 ** rng.uniform(lo, hi, size=shape)
  return (mag * np.where(rng.rand(*shape) < 0.5, -1.0, 1.0)).astype(np.float32)


def outputs_of(act, rng, shape):
  """Values an activation can have returned, as float32: the Y of a backward call."""
  if act == ACT_TANH:
    return np.clip(log_uniform(rng, shape, -10.0, 0.0), -1 + 2.0 ** -24, 1 - 2.0 ** -24).astype(np.float32)
  if act == ACT_SIGMOID:
    return np.clip(np.abs(log_uniform(rng, shape, -10.0, 0.0)), 2.0 ** -10, 1 - 2.0 ** -24).astype(np.float32)
  if act in (ACT_SELU, ACT_ELU):
    floor = SELU_S * SELU_A if act == ACT_SELU else 1.0
    pos = np.abs(log_uniform(rng, shape))
    neg = -floor * (1.0 - np.abs(log_uniform(rng, shape, -10.0, -0.01)))
    return np.where(rng.rand(*shape) < 0.5, pos, neg).astype(np.float32)
  return log_uniform(rng, shape)


def real_operands(B, N, K, wt, act, seed):
  rng = np.random.RandomState(seed)
  wshape = (K, N) if wt else (N, K)
  return dict(X=log_uniform(rng, (B, K)), W=log_uniform(rng, wshape), b=log_uniform(rng, (N,)),
              dY=log_uniform(rng, (B, N)), Y=outputs_of(act, rng, (B, N)), dW0=log_uniform(rng, wshape),
              Xact=outputs_of(act, rng, (B, K)))


def fwd_specials(act):
  """Pre-activations at the activations' edges (the inputs of test_bias_act_against_float64)."""
  s = [0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0]
  if act in (ACT_NONE, ACT_RELU, ACT_TANH):     # (the exp-based ones: expf(88) / its reciprocal leave fp32's normal range)
    s += [88.0, -88.0]
  return np.asarray(s, dtype=np.float32)


def bwd_specials(act):
  """Outputs Y at which act'(Y) sits at an edge: saturation, the sign test's two sides, the negative branch's floor."""
  s = [0.0, -0.0]
  if act == ACT_TANH:
    s += [1.0, -1.0]
  elif act == ACT_SIGMOID:
    s += [1.0]
  elif act == ACT_SELU:
    floor = np.float32(-SELU_S * SELU_A)
    s += [floor, np.nextafter(floor, np.float32(0.0))]
  elif act == ACT_ELU:
    s += [-1.0]
  elif act == ACT_RELU:
    s += [1e-30, -1e-30, 2.0 ** -126, -2.0 ** -126]     # (the smallest normal numbers: no subnormals here)
  s += [0.5, -0.25]
  if act == ACT_SIGMOID:
    s = [v for v in s if v >= 0]
  return np.asarray(s, dtype=np.float32)


# ------------------------------------------------------------------ case generators
AXIS = (1, 31, 32, 33, 65)                      # B and N: the 32-row / 32-column tile's edges
REDUCTIONS = (1, 3, 4, 7, 8, 9, 31, 32, 33, 127, 128, 129, 132, 255, 256, 257, 260)
# (k-quads 4, k-blocks 8, a wave's first block 32, the 128-deep chunk and its prefetched successor, 256)


def covering_cases():
  """(B, N, K, offs) over the small route, not the full cube: every reduction length once as K (forward), once as N
  (dX) and once as B (dW), the other two sizes walking AXIS, and the three bases' alignments walking all eight
  combinations.  offs = the offsets of X, W and dY from a 16-byte boundary, in floats."""
  cases = []
  for i, r in enumerate(REDUCTIONS):
    a, b = AXIS[i % 5], AXIS[(2 * i + 1) % 5]
    for j, (B, N, K) in enumerate(((a, b, r), (a, r, b), (r, a, b))):
      n = 3 * i + j
      cases.append((B, N, K, (n & 1, (n >> 1) & 1, (n >> 2) & 1)))
  # the vector path of each K-contiguous operand, switched off by the base alone (shape allows it) and on
  for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
    cases.append((33, 32, 132, offs))
    cases.append((33, 132, 32, offs))
  check_covering(cases)
  return cases


def check_covering(cases):
  for B, N, K, offs in cases:
    for wt in (0, 1):
      r = route(B, N, K, wt)
      assert r["fwd"][0] == r["dx"][0] == r["dw"][0] == "small", (B, N, K, wt)
    assert int_sum_bound(B, N, K) < 2 ** 24
  for axis, col in ((AXIS, 0), (AXIS, 1)):
    assert set(axis) <= {c[col] for c in cases}
  for col in (2, 1, 0):             # the reduction of the forward, of dX, of dW
    assert set(REDUCTIONS) <= {c[col] for c in cases}
  # each of X, W (both layouts' K-contiguous uses) and dY: vector loads on by shape and base, off by base alone
  seen = set()
  for B, N, K, offs in cases:
    if K % 4 == 0:
      seen.add(("X", offs[0] == 0))
      seen.add(("W fwd", offs[1] == 0))
    if N % 4 == 0:
      seen.add(("dY", offs[2] == 0))
      seen.add(("W dx", offs[1] == 0))
  assert seen == {(o, a) for o in ("X", "W fwd", "dY", "W dx") for a in (True, False)}, seen
  # the 4-modes of small_gemm_kernel over the two layouts
  modes = {route(B, N, K, wt)[g][1:] for B, N, K, _ in cases for wt in (0, 1) for g in ("fwd", "dx", "dw")}
  assert modes == {(0, 0), (0, 1), (1, 1)}, modes     # (<1, 0> is instantiated but no entry point asks for it)


def seam_cases():
  """(name, what, B, N, K, top): pairs of shapes on the two sides of each limit of rk_small_gemm_fits, forward and
  backward; top = the largest integer magnitude, chosen so that the sums stay exact."""
  cases = [
    ("fwd_N", "fwd", 5, 1024, 8, 8), ("fwd_N", "fwd", 5, 1025, 8, 8),
    ("fwd_K", "fwd", 2, 3, 4096, 1), ("fwd_K", "fwd", 2, 3, 4097, 1),
    ("fwd_tiles", "fwd", 4096, 1024, 4, 8), ("fwd_tiles", "fwd", 4097, 1024, 4, 8),
    ("bwd_K", "bwd", 5, 8, 1024, 8), ("bwd_K", "bwd", 5, 8, 1025, 8),
    ("bwd_B", "bwd", 4096, 5, 8, 1), ("bwd_B", "bwd", 4097, 5, 8, 1),
  ]
  for i in range(0, len(cases), 2):
    (name, what, B, N, K, top), (_, _, B2, N2, K2, _) = cases[i], cases[i + 1]
    for wt in (0, 1):
      g = "fwd" if what == "fwd" else "dx"
      assert route(B, N, K, wt)[g][0] == "small" and route(B2, N2, K2, wt)[g][0] == "gemm", name
      assert route(B2, N2, K2, wt)["dw" if what == "bwd" else "fwd"][0] == "gemm"
    assert int_sum_bound(B2, N2, K2, top) < 2 ** 24
  return cases


FB_EDGE = (63, 64, 65)                         # the fallback's 64 x 64 tile
FB_BIG = (1087, 1088, 1089)                    # the same three residues past rk_small_gemm_fits' N <= 1024
FB_RED = (1, 15, 16, 17, 33)                   # its 16-deep k-tile, two tiles and a tail


def fallback_cases():
  """(what, B, N, K, offs) that reach gemm_kernel<2, 2, 1, 1, ..> BY SHAPE.  One size has to be past a limit of
  rk_small_gemm_fits, so it carries the tile residues 63 / 0 / 1 at 1087 / 1088 / 1089: the forward with N past
  1024 (M = B on the edge, reduction K), the backward with K past 1024 (dX: M = B, N = K, reduction N; dW: M = N or
  K, reduction B).  Vector loads need every base aligned and every leading dimension a multiple of 4."""
  cases = []
  for i, r in enumerate(FB_RED):
    cases.append(("fwd", FB_EDGE[i % 3], FB_BIG[(i + 1) % 3], r, (0, 0, 0)))
    cases.append(("bwd", FB_EDGE[i % 3], r, FB_BIG[i % 3], (0, 0, 0)))            # dX's reduction = N = r
    cases.append(("bwd", r, FB_EDGE[(i + 1) % 3], FB_BIG[(i + 2) % 3], (0, 0, 0)))  # dW's reduction = B = r
  for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
    cases.append(("fwd", 64, 1088, 16, offs))
    cases.append(("bwd", 64, 16, 1088, offs))
    cases.append(("bwd", 16, 64, 1088, offs))
  reached = set()
  for what, B, N, K, offs in cases:
    for wt in (0, 1):
      r, v = route(B, N, K, wt), vec_loads(B, N, K, wt, offs)
      for g in (("fwd",) if what == "fwd" else ("dx", "dw")):
        assert r[g][0] == "gemm", (what, B, N, K, wt)
        reached.add((r[g][1:], v[g]))
    assert int_sum_bound(B, N, K) < 2 ** 24
  assert reached == {(m, v) for m in ((0, 0), (0, 1), (1, 1)) for v in (True, False)}, reached
  fb = {c[1:4] for c in cases}
  assert {63, 64, 65} <= {s[0] for s in fb} and set(FB_RED) <= {s[2] for s in fb if s[1] > 1024}
  assert set(FB_RED) <= {s[1] for s in fb if s[2] > 1024} and set(FB_RED) <= {s[0] for s in fb if s[2] > 1024}
  assert set(FB_BIG) <= {s[1] for s in fb} and set(FB_BIG) <= {s[2] for s in fb}
  return cases


def real_cases():
  """(B, N, K, act, offs) for the float64 comparison: a subset of the shapes above over both routes, every
  activation, chunk seams (129, 257, 260) in each of the three reductions."""
  cases = [
    (33, 65, 129, ACT_TANH, (0, 0, 0)), (65, 33, 260, ACT_SIGMOID, (1, 0, 1)), (31, 257, 32, ACT_SELU, (0, 1, 0)),
    (257, 31, 33, ACT_ELU, (0, 0, 1)), (1, 1, 1, ACT_RELU, (0, 0, 0)), (65, 132, 128, ACT_NONE, (0, 0, 0)),
    (9, 8, 7, ACT_TANH, (1, 1, 1)),
    # the fallback: forward by N, backward by K
    (63, 1089, 17, ACT_TANH, (0, 0, 0)), (64, 1088, 16, ACT_SELU, (0, 0, 0)),
    (65, 17, 1089, ACT_SIGMOID, (0, 0, 0)), (16, 64, 1088, ACT_ELU, (0, 0, 0)), (33, 63, 1087, ACT_RELU, (0, 1, 0)),
  ]
  fams = {route(B, N, K, wt)[g][0] for B, N, K, _, _ in cases for wt in (0, 1) for g in ("fwd", "dx", "dw")}
  assert fams == {"small", "gemm"} and {c[3] for c in cases} == set(ACTS)
  return cases


AGC_ROWS = (1, 31, 32, 33, 511, 512, 513, 545)  # act_grad_colsum_kernel: 32 slices, a second round of 16 above 512
AGC_COLS = (1, 31, 32, 33, 65)
SGC_ROWS = (1, 7, 8, 9, 33)                     # sg_colsum_tile: 8 slices, a 4-way unroll and its tail
CS_ROWS = (1, 15, 16, 17, 65)                   # colsum_kernel: 16 slices
CS_COLS = (1, 63, 64, 65)


def check_reduction_cases():
  per = lambda rows, slices: -(-rows // slices)
  assert max(per(r, 32) for r in AGC_ROWS) > 16 >= per(512, 32)        # 513 and 545 start a second round
  assert {per(r, 8) for r in SGC_ROWS} >= {1, 2, 5}                    # tail only, and the unrolled loop plus its tail
  assert {per(r, 16) for r in CS_ROWS} >= {1, 2, 5}
  for B in SGC_ROWS:
    for N in AGC_COLS:
      assert route(B, N, 5, 0)["dx"][0] == "small"                     # the paired launch that carries sg_colsum_tile
