"""The hidden nn.Linear stack's kernels through the C ABI (rk_linear_fwd, rk_linear_bwd, rk_linear_bwd_dact,
rk_linear_bwd_pre, rk_act_grad, rk_colsum), each against tests/linear_util.py's float64 restatement at the
shapes where the tiles, the K chunks, the row slices and the host's routes have their edges.

Every operand sits at a chosen alignment inside a NaN-filled buffer; every output is NaN where the call must
overwrite it and is followed by a canary; whatever a call leaves outside its outputs' live regions must keep its
bits (`Buf.get`).  Integer operands make every partial sum exact in fp32 in any order, so those comparisons are
equalities; real-valued ones (magnitudes log-uniform in [2^-10, 2^4], no subnormals) are held to counted bounds,
u = 2^-24, g(n) = n u / (1 - n u):

  pre      |pre_hat - pre| <= g(K + 4) S, S = |X| |W|^T + |b|: a K-term sum in any order, the bias add and the
           three cross-wave adds of small_gemm_tile.
  act(pre) that bound times the activation's Lipschitz constant, plus BIAS_ACT_ULP[act] ulps of the result
           (test_row_kernels.py's measured figure of the same rk_act).
  dYpre    fl(dY * rk_act_dy(Y)): rk_act_dy is at most two roundings on operands no larger than max(1, |y|)
           (linear_util.act_dy_err lists each formula's bound e(y)), then the product rounds once:
           |dYpre_hat - dY act'(Y)| <= |dY| (e (1 + u) + u |act'(Y)|)              (linear_util.dypre_bound).
  dX dW db g(n + 4) times their sums of absolute products (dW's with |dW0|), n = N, B, B, taken on the kernel's
           own dYpre as exact input, so that each bound covers one chain.  With act'(dx_act_y) folded into dX:
           linear_util.times_act_dy_bound on top of dX's bound.

Largest error / bound ratios observed on an MI355X (each test prints its own under -s): pre 0.391, act(pre) 0.181,
dYpre 0.777, dX 0.291, dW 0.379 (onto dW0: 0.339), db 0.139; dX at the activation edges 0.242; db alone 0.103
(act_grad_colsum_kernel), 0.200 (sg_colsum_tile), 0.148 (colsum_kernel).  Forward at the activation edges, in ulps
against BIAS_ACT_ULP: sigmoid 0.333, selu 0.624, elu 0.017, none / tanh / relu 0.

These tests found that the fallback's scalar loads of a k-major operand read the row's FIRST four columns in place
of a ragged last group (leading dimension no multiple of 4): test_exact_fallback, test_route_seams and test_real
failed 33 cases on it before csrc/gemm.hip's `a_rem` / `b_rem` stopped those loads at the row's last element.

Kernel -> test:
  small_gemm_kernel<0,0> / <0,1> / <1,1>      test_exact_small (forward wt = 0 / 1, dX wt = 1 / 0, dW; un-paired at
                                              RK_TUNE_LINEAR_PAIR = 0 and for a lone dX or dW in test_null_arguments)
  small_gemm_kernel<1,0>                      no entry point selects it
  small_gemm_pair_kernel, both orders         test_exact_small (pair = 1, RK_TUNE_PAIR_ORDER 0 / 1), test_real
  sg_colsum_tile                              test_sg_colsum, test_null_arguments (rk_linear_bwd_pre, paired)
  act_grad_colsum_kernel                      test_act_grad_colsum, every rk_linear_bwd with db
  act_grad_kernel                             test_null_arguments (db = NULL), test_activation_edges_backward
  colsum_kernel                               test_colsum, rk_linear_bwd_pre un-paired
  gemm_kernel<2,2,1,1,0,0 / 0,1 / 1,1, VEC>   test_exact_fallback, test_route_seams, test_real (vector loads on and off)
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recoder_amd import _lib
from recoder_amd._lib import check
from recoder_amd.device import Block, DeviceCSR, current_stream
from tests import linear_util as lu
from tests.encoder_util import ACT_NONE, ACT_RELU, ACT_TANH, ACTS, U, gamma, ulp_distance
from tests.test_row_kernels import BIAS_ACT_ULP

pytestmark = pytest.mark.gpu

CANARY = 12345.0
PAD = 64                 # floats of NaN in front of a live region (a multiple of four: the alignment is `off` alone)
RK_TUNE_PAIR_ORDER = 9   # include/recoder_hip_probe.h


class Buf:
  """A live region of float32 at `off` floats past a 16-byte boundary, NaN in front of it and, behind it, NaN (an
  operand) or a canary (an output)."""

  def __init__(self, live, off=0, out=False):
    live = np.asarray(live, dtype=np.float32)
    self.shape, self.lo = live.shape, PAD + off
    self.hi = self.lo + live.size
    host = np.full(self.hi + PAD, np.nan, dtype=np.float32)
    host[self.lo:self.hi] = live.ravel()
    if out:
      host[self.hi:] = CANARY
    self.host = host
    self.t = torch.from_numpy(host).to("cuda")
    assert self.t.data_ptr() % 16 == 0
    self.ptr = self.t.data_ptr() + 4 * self.lo

  def get(self):
    g = self.t.cpu().numpy()
    bits = lambda a: a.view(np.int32)
    assert np.array_equal(bits(g[:self.lo]), bits(self.host[:self.lo])), "written in front of the live region"
    assert np.array_equal(bits(g[self.hi:]), bits(self.host[self.hi:])), "written past the live region"
    return g[self.lo:self.hi].reshape(self.shape).copy()


def out_buf(shape, init=None):
  """An output: NaN where the call must overwrite it, or the values it accumulates onto."""
  return Buf(np.full(shape, np.nan, np.float32) if init is None else init, out=True)


def P(b):
  return None if b is None else b.ptr


class Tune:
  """The two knobs of the paired backward launch, restored to their defaults on the way out."""

  def __init__(self, pair, order=0):
    self.pair, self.order = pair, order

  def __enter__(self):
    lib = _lib.load()
    lib.rk_linear_pair(self.pair)
    lib.rk_tune(RK_TUNE_PAIR_ORDER, self.order)

  def __exit__(self, *exc):
    lib = _lib.load()
    lib.rk_linear_pair(1)
    lib.rk_tune(RK_TUNE_PAIR_ORDER, 0)


def fwd(o, B, N, K, wt, act, offs=(0, 0, 0), bias=True):
  lib = _lib.load()
  X, W = Buf(o["X"], offs[0]), Buf(o["W"], offs[1])
  b = Buf(o["b"]) if bias else None
  Y = out_buf((B, N))
  check(lib.rk_linear_fwd(X.ptr, W.ptr, P(b), B, N, K, wt, act, Y.ptr, current_stream()), "rk_linear_fwd")
  torch.cuda.synchronize()
  for x in (X, W) + ((b,) if bias else ()):
    x.get()
  y = Y.get()
  assert not np.isnan(y).any(), "a NaN from outside the live operands, or an element left unwritten"
  return y


def bwd(o, B, N, K, wt, act, offs=(0, 0, 0), acc=0, entry="bwd", dx=True, dw=True, db=True, dact=False):
  """One backward call; returns dict(dYpre, dX, dW, db) of what was asked for.  entry: "bwd" (rk_linear_bwd),
  "dact" (rk_linear_bwd_dact) or "pre" (rk_linear_bwd_pre: o["dY"] already is dYpre, Y is not read)."""
  lib = _lib.load()
  X, W, dY = Buf(o["X"], offs[0]), Buf(o["W"], offs[1]), Buf(o["dY"], offs[2])
  Y = Buf(o["Y"]) if entry != "pre" else None
  ya = Buf(o["Xact"]) if dact else None
  dX = out_buf((B, K)) if dx else None
  dW = out_buf(o["W"].shape, o["dW0"] if acc else None) if dw else None
  dB = out_buf((N,)) if db else None
  st = current_stream()
  if entry == "bwd":
    assert not dact
    check(lib.rk_linear_bwd(dY.ptr, Y.ptr, X.ptr, W.ptr, B, N, K, wt, act, P(dX), P(dW), acc, P(dB), st),
          "rk_linear_bwd")
  elif entry == "dact":
    check(lib.rk_linear_bwd_dact(dY.ptr, Y.ptr, X.ptr, W.ptr, B, N, K, wt, act, P(dX), P(dW), acc, P(dB), P(ya), st),
          "rk_linear_bwd_dact")
  else:
    check(lib.rk_linear_bwd_pre(dY.ptr, X.ptr, W.ptr, B, N, K, wt, act, P(dX), P(dW), acc, P(dB), P(ya), st),
          "rk_linear_bwd_pre")
  torch.cuda.synchronize()
  for x in (X, W, Y, ya):
    if x is not None:
      x.get()
  res = {"dYpre": dY.get()}
  for name, buf in (("dX", dX), ("dW", dW), ("db", dB)):
    if buf is not None:
      res[name] = buf.get()
      assert not np.isnan(res[name]).any(), name + ": a NaN from outside the live operands, or an element left unwritten"
  return res


def same_bits(a, b):
  return np.array_equal(a.view(np.int32), b.view(np.int32))


def ratio(got, ref, bound):
  """The largest |got - ref| / bound (0 / 0 counts as 0: an exact result under a zero bound)."""
  err = np.abs(np.asarray(got, dtype=np.float64) - ref)
  with np.errstate(divide="ignore", invalid="ignore"):
    r = np.where(err == 0, 0.0, err / bound)
  return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------ a, b: exact on integers
def exact_forward(B, N, K, wt, offs, top=8):
  o = lu.int_operands(B, N, K, wt, seed=B * 7 + N * 3 + K, top=top)
  pre, _, _ = lu.linear_fwd64(o["X"], o["W"], o["b"], wt, ACT_NONE)
  got = fwd(o, B, N, K, wt, ACT_NONE, offs)
  assert np.array_equal(got, pre), "forward: %d elements differ" % int((got != pre).sum())


def exact_backward(B, N, K, wt, offs, top=8, tunes=((0, 0), (1, 0), (1, 1))):
  o = lu.int_operands(B, N, K, wt, seed=B * 7 + N * 3 + K, top=top)
  for acc in (0, 1):
    dYpre, dX, dW, db, _, _, _ = lu.linear_bwd64(o["dY"], o["Y"], o["X"], o["W"], wt, ACT_NONE, o["dW0"] if acc else None)
    for pair, order in tunes:
      with Tune(pair, order):
        r = bwd(o, B, N, K, wt, ACT_NONE, offs, acc=acc)
      tag = "pair %d order %d acc %d" % (pair, order, acc)
      assert np.array_equal(r["dYpre"], dYpre), tag
      for name, want in (("dX", dX), ("dW", dW), ("db", db)):
        assert np.array_equal(r[name], want), "%s, %s: %d elements differ" % (name, tag, int((r[name] != want).sum()))


COVERING = lu.covering_cases()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("case", COVERING, ids=["%dx%dx%d-%d%d%d" % (c[:3] + c[3]) for c in COVERING])
def test_exact_small(case, wt):
  """The small route's tiles, K blocks, chunks and alignments: forward, dX, dW (with and without dW0) and db EQUAL
  the integer products, un-paired and paired in both orders."""
  B, N, K, offs = case
  exact_forward(B, N, K, wt, offs)
  exact_backward(B, N, K, wt, offs)


SEAMS = lu.seam_cases()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("case", SEAMS, ids=["%s-%dx%dx%d" % ((c[0],) + c[2:5]) for c in SEAMS])
def test_route_seams(case, wt):
  """The two sides of each limit of rk_small_gemm_fits, forward and backward (its roles permuted)."""
  _, what, B, N, K, top = case
  if what == "fwd":
    exact_forward(B, N, K, wt, (0, 0, 0), top)
  else:
    exact_backward(B, N, K, wt, (0, 0, 0), top, tunes=((1, 0),))


FALLBACK = lu.fallback_cases()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("case", FALLBACK, ids=["%s-%dx%dx%d-%d%d%d" % (c[:4] + c[4]) for c in FALLBACK])
def test_exact_fallback(case, wt):
  """gemm_kernel<2, 2, 1, 1, AM, BM, EPI_STORE, VEC> reached by shape: its 64 x 64 tile's and 16-deep k-tile's edges
  in all three operand modes, vector loads on and off."""
  what, B, N, K, offs = case
  if what == "fwd":
    exact_forward(B, N, K, wt, offs)
  else:
    exact_backward(B, N, K, wt, offs, tunes=((1, 0),))


# ------------------------------------------------------------------ c: real values against float64
REAL = lu.real_cases()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("case", REAL, ids=["%dx%dx%d-act%d" % c[:4] for c in REAL])
def test_real(case, wt):
  B, N, K, act, offs = case
  o = lu.real_operands(B, N, K, wt, act, seed=B + 3 * N + 5 * K + wt)
  # ---- forward: the pre-activation alone, then through the activation
  pre, out, S = lu.linear_fwd64(o["X"], o["W"], o["b"], wt, act)
  tol = gamma(K + 4) * S
  r_pre = ratio(fwd(o, B, N, K, wt, ACT_NONE, offs), pre, tol)
  tol_act = lu.LIPSCHITZ[act] * tol + BIAS_ACT_ULP[act] * np.spacing(np.abs(out.astype(np.float32))).astype(np.float64)
  r_act = ratio(fwd(o, B, N, K, wt, act, offs), out, tol_act)
  # ---- backward, Y an input; dX, dW and db on the kernel's own dYpre
  ratios = {}
  for acc in (0, 1):
    r = bwd(o, B, N, K, wt, act, offs, acc=acc)
    ratios["dYpre"] = ratio(r["dYpre"], o["dY"].astype(np.float64) * lu.act_dy64(o["Y"], act),
                            lu.dypre_bound(o["dY"], o["Y"], act))
    _, dX, dW, db, SX, SW, Sb = lu.linear_bwd64(r["dYpre"], None, o["X"], o["W"], wt, act, o["dW0"] if acc else None)
    ratios["dX"] = ratio(r["dX"], dX, gamma(N + 4) * SX)
    ratios["dW acc %d" % acc] = ratio(r["dW"], dW, gamma(B + 4) * SW)
    ratios["db"] = ratio(r["db"], db, gamma(B + 4) * Sb)
  print("linear %dx%dx%d wt %d act %d: error / bound  pre %.3f  act %.3f  %s" % (
      B, N, K, wt, act, r_pre, r_act, "  ".join("%s %.3f" % kv for kv in ratios.items())))
  assert r_pre <= 1.0 and r_act <= 1.0, (r_pre, r_act)
  assert all(v <= 1.0 for v in ratios.values()), ratios


# ------------------------------------------------------------------ d: activation edges
@pytest.mark.parametrize("N_tiles", [1, 180], ids=["small", "fallback"])
@pytest.mark.parametrize("act", ACTS)
def test_activation_edges_forward(act, N_tiles):
  """Rows of X are zero and the bias carries the specials: pre IS the special, whatever W holds."""
  sp_ = lu.fwd_specials(act)
  B, K, N = 3, 5, len(sp_) * N_tiles
  assert lu.route(B, N, K, 0)["fwd"][0] == ("small" if N_tiles == 1 else "gemm")
  rng = np.random.RandomState(act)
  o = dict(X=np.zeros((B, K), np.float32), W=lu.log_uniform(rng, (N, K)), b=np.tile(sp_, N_tiles))
  got = fwd(o, B, N, K, 0, act)
  ref = np.broadcast_to(lu.act64(o["b"], act), (B, N))
  d = ulp_distance(got, ref)
  print("forward edges act %d: largest ulp distance %.3f" % (act, d.max()))
  i = np.unravel_index(int(d.argmax()), d.shape)
  assert d.max() <= BIAS_ACT_ULP[act], "act %d at pre = %r: %r, float64 %r" % (act, o["b"][i[1]], got[i], ref[i])


@pytest.mark.parametrize("entry", ["dact", "pre"])
@pytest.mark.parametrize("act", ACTS)
def test_activation_edges_backward(act, entry):
  """Y and dx_act_y at the edges of act': saturated, on both sides of the sign tests, at the negative branch's floor."""
  sp_ = lu.bwd_specials(act)
  B, N, K = 9, 2 * len(sp_) + 1, 2 * len(sp_) + 3
  rng = np.random.RandomState(act + 20)
  o = lu.real_operands(B, N, K, 0, act, seed=act)
  o["Y"] = np.resize(sp_, (B, N)).astype(np.float32)
  o["Xact"] = np.resize(sp_[::-1], (B, K)).astype(np.float32)
  want_pre = o["dY"].astype(np.float64) * lu.act_dy64(o["Y"], act)
  if entry == "pre":
    o["dY"] = want_pre.astype(np.float32)
  for db in (True, False):          # (without db: rk_act_grad in place of rk_act_grad_colsum)
    r = bwd(o, B, N, K, 0, act, entry=entry, db=db, dact=True)
    if entry == "pre":
      assert same_bits(r["dYpre"], o["dY"])
    else:
      assert ratio(r["dYpre"], want_pre, lu.dypre_bound(o["dY"], o["Y"], act)) <= 1.0
    _, dX, _, _, SX, _, _ = lu.linear_bwd64(r["dYpre"], None, o["X"], o["W"], 0, act)
    tol = lu.times_act_dy_bound(dX, gamma(N + 4) * SX, o["Xact"], act)
    rx = ratio(r["dX"], dX * lu.act_dy64(o["Xact"], act), tol)
    print("backward edges act %d %s db %d: dX error / bound %.3f" % (act, entry, db, rx))
    assert rx <= 1.0


# ------------------------------------------------------------------ e: the reductions alone
@pytest.mark.parametrize("rows", lu.AGC_ROWS)
def test_act_grad_colsum(rows):
  """act_grad_colsum_kernel alone: rk_linear_bwd with dX = dW = NULL launches nothing else."""
  worst = 0.0
  for cols in lu.AGC_COLS:
    rng = np.random.RandomState(rows * 100 + cols)
    # integers, and relu's 0 / 1 factor on them: exact
    oi = lu.int_operands(rows, cols, 4, 0, seed=rows + cols)
    for act in (ACT_NONE, ACT_RELU):
      r = bwd(oi, rows, cols, 4, 0, act, dx=False, dw=False)
      want = oi["dY"].astype(np.float64) * lu.act_dy64(oi["Y"], act)
      assert np.array_equal(r["dYpre"], want) and np.array_equal(r["db"], want.sum(0)), (cols, act)
    o = lu.real_operands(rows, cols, 4, 0, ACT_TANH, seed=rows + 7 * cols)
    r = bwd(o, rows, cols, 4, 0, ACT_TANH, dx=False, dw=False)
    assert ratio(r["dYpre"], o["dY"].astype(np.float64) * lu.act_dy64(o["Y"], ACT_TANH),
                 lu.dypre_bound(o["dY"], o["Y"], ACT_TANH)) <= 1.0
    v = r["dYpre"].astype(np.float64)
    worst = max(worst, ratio(r["db"], v.sum(0), gamma(rows + 4) * np.abs(v).sum(0)))
  print("act_grad_colsum rows %d: db error / bound %.3f" % (rows, worst))
  assert worst <= 1.0


@pytest.mark.parametrize("rows", lu.SGC_ROWS)
def test_sg_colsum(rows):
  """sg_colsum_tile: the third workgroup range of rk_linear_bwd_pre's paired launch, in both orders."""
  worst = 0.0
  for cols in lu.AGC_COLS:
    for order in (0, 1):
      oi = lu.int_operands(rows, cols, 5, 0, seed=rows + cols)
      with Tune(1, order):
        r = bwd(oi, rows, cols, 5, 0, ACT_NONE, entry="pre")
      _, dX, dW, db, _, _, _ = lu.linear_bwd64(oi["dY"], None, oi["X"], oi["W"], 0, ACT_NONE)
      assert np.array_equal(r["db"], db) and np.array_equal(r["dX"], dX) and np.array_equal(r["dW"], dW)
      o = lu.real_operands(rows, cols, 5, 0, ACT_NONE, seed=rows + 7 * cols)
      with Tune(1, order):
        r = bwd(o, rows, cols, 5, 0, ACT_NONE, entry="pre")
      v = o["dY"].astype(np.float64)
      worst = max(worst, ratio(r["db"], v.sum(0), gamma(rows + 4) * np.abs(v).sum(0)))
  print("sg_colsum rows %d: db error / bound %.3f" % (rows, worst))
  assert worst <= 1.0


@pytest.fixture(scope="module")
def collated_counts():
  """(counts, cols, ld): the device-resident sizes of a collated block over 65 live columns (no sampling)."""
  n = max(lu.CS_COLS)
  csr = sp.csr_matrix(np.ones((2, n), np.float32))
  users = torch.arange(2, dtype=torch.int64, device="cuda")
  blk = Block(2, csr.nnz, n, "cuda", negative_sampling=False).collate(DeviceCSR(csr), users)
  n_b, _, ld, _ = blk.counts_host()
  assert n_b == n and ld > n
  return blk, n_b, ld


@pytest.mark.parametrize("rows", lu.CS_ROWS)
def test_colsum(rows, collated_counts):
  """colsum_kernel called directly, ld > cols; the sizes from the host, and once from a collated block's counts."""
  lib = _lib.load()
  blk, n_b, ld_b = collated_counts
  worst = 0.0
  for cols, ld, counts in [(c, c + 3, None) for c in lu.CS_COLS] + [(n_b, ld_b, blk.counts)]:
    for real in (False, True):
      rng = np.random.RandomState(rows * 10 + cols)
      live = lu.log_uniform(rng, (rows, cols)) if real else rng.randint(-8, 9, size=(rows, cols)).astype(np.float32)
      full = np.full((rows, ld), np.nan, np.float32)
      full[:, :cols] = live
      X, out = Buf(full), out_buf((cols,))
      # (with counts the kernel takes cols and ld from the device: the host's ld is then 0, as its callers pass it)
      check(lib.rk_colsum(X.ptr, rows, cols, 0 if counts is not None else ld,
                          None if counts is None else counts.data_ptr(), out.ptr, current_stream()), "rk_colsum")
      torch.cuda.synchronize()
      X.get()
      got, v = out.get(), live.astype(np.float64)
      if real:
        worst = max(worst, ratio(got, v.sum(0), gamma(rows + 4) * np.abs(v).sum(0)))
      else:
        assert np.array_equal(got, v.sum(0)), (cols, ld)
  print("colsum rows %d: error / bound %.3f" % (rows, worst))
  assert worst <= 1.0


# ------------------------------------------------------------------ f: NULL arguments, repeats, the three entries
NULL_SHAPES = [(33, 65, 129, 0, ACT_TANH), (65, 33, 260, 1, ACT_TANH), (1, 1, 1, 0, ACT_RELU), (9, 31, 8, 1, ACT_NONE),
               (63, 17, 1089, 0, ACT_TANH), (17, 65, 1087, 1, ACT_TANH)]


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("B,N,K,wt,act", NULL_SHAPES, ids=["%dx%dx%d-wt%d-act%d" % s for s in NULL_SHAPES])
def test_null_arguments(B, N, K, wt, act, pair):
  """Each NULL argument leaves the remaining outputs' bits as the full call gives them; every route repeats bit for
  bit; rk_linear_bwd, rk_linear_bwd_dact + rk_act_grad and rk_linear_bwd_pre agree as they are documented to."""
  lib = _lib.load()
  o = lu.real_operands(B, N, K, wt, act, seed=B + N + K)
  with Tune(pair):
    # ---- forward: bias = NULL adds 0.f in the same place
    assert same_bits(fwd(o, B, N, K, wt, act, bias=False), fwd(dict(o, b=np.zeros(N, np.float32)), B, N, K, wt, act))
    assert same_bits(fwd(o, B, N, K, wt, act), fwd(o, B, N, K, wt, act))
    for acc in (0, 1):
      full = bwd(o, B, N, K, wt, act, acc=acc)
      again = bwd(o, B, N, K, wt, act, acc=acc)
      assert all(same_bits(full[k], again[k]) for k in full), "a second run differs"
      for drop in ("db", "dx", "dw"):          # db = NULL: rk_act_grad; a lone dX or dW: the un-paired small_gemm_kernel
        part = bwd(o, B, N, K, wt, act, acc=acc, **{drop: False})
        assert set(part) == set(full) - {{"db": "db", "dx": "dX", "dw": "dW"}[drop]}
        for k in part:
          assert same_bits(part[k], full[k]), "%s differs without %s" % (k, drop)
      # ---- _dact == the plain call followed by rk_act_grad on dX; dYpre, dW and db unchanged
      dact = bwd(o, B, N, K, wt, act, acc=acc, entry="dact", dact=True)
      dX, ya = Buf(full["dX"]), Buf(o["Xact"])
      check(lib.rk_act_grad(dX.ptr, ya.ptr, B * K, act, current_stream()), "rk_act_grad")
      torch.cuda.synchronize()
      assert same_bits(dact["dX"], dX.get())
      assert all(same_bits(dact[k], full[k]) for k in ("dYpre", "dW", "db"))
      # ---- _pre on that dYpre: the same dX and dW; db in another slice order, so within its bound
      pre = bwd(dict(o, dY=full["dYpre"]), B, N, K, wt, act, acc=acc, entry="pre", dact=True)
      again = bwd(dict(o, dY=full["dYpre"]), B, N, K, wt, act, acc=acc, entry="pre", dact=True)
      assert all(same_bits(pre[k], again[k]) for k in pre), "a second run differs"
      assert same_bits(pre["dX"], dact["dX"]) and same_bits(pre["dW"], dact["dW"])
      assert same_bits(pre["dYpre"], full["dYpre"])
      v = full["dYpre"].astype(np.float64)
      assert ratio(pre["db"], v.sum(0), gamma(B + 4) * np.abs(v).sum(0)) <= 1.0
