"""The small row kernels, each against a plain float64 / exact restatement of its definition:
rk_bias_act, rk_adam_rows (csrc/optim.hip), rk_scatter_pos, rk_rows_to_dense, rk_mnll_row_stats,
rk_loss_reduce (csrc/gemm.hip) and rk_densify (csrc/collate.hip).  Tolerances are counted rounding bounds;
the one measured figure is the ulp distance of the device's tanhf / expf-based activations (BIAS_ACT_ULP)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recoder_amd import _lib
from recoder_amd._lib import check, ptr
from recoder_amd.device import Block, DeviceCSR, current_stream
from tests import encoder_util as eu
from tests.adam_util import E, sadam64  # noqa: F401  (the error-carrying float64 and sadam1's restatement)
from tests.encoder_util import ACT_ELU, ACT_NONE, ACT_RELU, ACT_SELU, ACT_SIGMOID, ACT_TANH, ACTS, U, gamma

pytestmark = pytest.mark.gpu

CANARY = 12345.0
# Largest ulp distance of rk_bias_act from the float64 activation of the fp32 sum, measured on an MI355X over
# the inputs of test_bias_act_against_float64 (all shapes, with and without bias):
#   tanh 1.246   sigmoid 2.036   selu 1.904   elu 0.840   (none / relu: 0, exact)
# asserted: twice the measured value rounded up, never more than 8
BIAS_ACT_ULP = {ACT_NONE: 0, ACT_RELU: 0, ACT_TANH: 3, ACT_SIGMOID: 5, ACT_SELU: 4, ACT_ELU: 2}
# expf's own figure, for the sums of exponentials below: sigmoid(x) = 1 / (1 + expf(-x)) carries expf's relative
# error (plus two roundings) wherever expf(-x) >> 1, so the sigmoid figure bounds it.  1 ulp <= 2 u relative.
EXP_ULP = BIAS_ACT_ULP[ACT_SIGMOID]
EXP_REL = 2 * EXP_ULP * U


def dev_t(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ------------------------------------------------------------------ rk_bias_act
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (37, 200)])
@pytest.mark.parametrize("act", ACTS)
def test_bias_act_against_float64(rows, cols, act):
  """Measured on an MI355X (largest ulp distance over all shapes, bias and no bias): tanh 1.246, sigmoid 2.036,
  selu 1.904, elu 0.840; none and relu exact.  selu / elu go through expm1f: expf(x) - 1 in fp32 gives
  elu(-1e-30) = 0 (all of the result lost) and, by the same arithmetic in numpy, up to 5.6e5 ulp over this
  test's small negative inputs."""
  lib = _lib.load()
  n = rows * cols
  rng = np.random.RandomState(rows * 7 + act)
  special = [0.0, 1e-30, -1e-30, 20.0, -20.0]
  if act in (ACT_NONE, ACT_RELU, ACT_TANH):      # (the exp-based ones: expf(88) / its reciprocal leave fp32's normal range)
    special += [88.0, -88.0]
  vals = np.concatenate([np.asarray(special), rng.randn(n) * 3, -np.abs(rng.randn(n)) * 0.01]).astype(np.float32)
  vals = np.concatenate([vals, np.zeros(-len(vals) % n, np.float32)]).reshape(-1, n)
  worst = 0.0
  for bias in (None, (rng.randn(cols) * 0.5).astype(np.float32)):
    for x in vals:
      X = torch.full((n + 64,), CANARY, dtype=torch.float32, device="cuda")
      X[:n] = dev_t(x)
      bd = dev_t(bias) if bias is not None else None
      check(lib.rk_bias_act(ptr(X), ptr(bd), rows, cols, act, current_stream()), "rk_bias_act")
      torch.cuda.synchronize()
      got = X.cpu().numpy()
      assert np.all(got[n:] == CANARY)
      pre = x if bias is None else (x.reshape(rows, cols) + bias).reshape(-1)        # the fp32 sum
      ref = eu.act64(pre.astype(np.float64), act)
      d = eu.ulp_distance(got[:n], ref)
      worst = max(worst, float(d.max()))
      i = int(d.argmax())
      assert d.max() <= BIAS_ACT_ULP[act], "act %d at x = %r: %r, float64 %r" % (act, pre[i], got[i], ref[i])
  print("rk_bias_act %dx%d act %d: largest ulp distance %.3f" % (rows, cols, act, worst))


# ------------------------------------------------------------------ rk_adam_rows
@pytest.mark.parametrize("h", [1, 3, 64, 200])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("wide", [False, True])
def test_adam_rows_against_float64(h, step, wide):
  lib = _lib.load()
  n_rows, n_cap, n_live = 40, 8, 5
  rng = np.random.RandomState(h * 13 + step)
  W = rng.randn(n_rows, h).astype(np.float32)
  m = (rng.randn(n_rows, h) * 0.1).astype(np.float32)
  v = (rng.rand(n_rows, h) * 0.01).astype(np.float32)
  G = rng.randn(n_cap, h).astype(np.float32)
  # 5 live rows (the table's last row among them: the largest id it allows) and 3 listed past n_dev
  idx = np.array([39, 4, 17, 0, 22, 8, 9, 30])
  # g = 0 with v = 0: the denominator is eps alone (once with a first moment, once without)
  G[0, 0] = 0.0; v[39, 0] = 0.0; m[39, 0] = 1e-6
  G[1, 0] = 0.0; v[4, 0] = 0.0; m[4, 0] = 0.0
  Wd, md, vd, Gd = dev_t(W), dev_t(m), dev_t(v), dev_t(G)
  idxd = dev_t(idx.astype(np.int64 if wide else np.int32))
  n_dev = dev_t(np.array([n_live], np.int32))
  lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
  check(lib.rk_adam_rows(ptr(Wd), ptr(md), ptr(vd), h, None if wide else ptr(idxd), ptr(idxd) if wide else None,
                         ptr(n_dev), n_cap, ptr(Gd), lr, b1, b2, eps, step, current_stream()), "rk_adam_rows")
  torch.cuda.synchronize()
  live = idx[:n_live]
  rest = np.setdiff1d(np.arange(n_rows), live)
  outs = []
  for name, dev, host in (("W", Wd, W), ("m", md, m), ("v", vd, v)):
    got = dev.cpu().numpy()
    # unlisted rows and the rows listed past n_dev keep their bits
    assert np.array_equal(got[rest].view(np.int32), host[rest].view(np.int32)), name
    outs.append(got[live])
  ref = sadam64(W[live], m[live], v[live], G[:n_live], lr, b1, b2, eps, step)
  for name, got, r in zip("Wmv", outs, ref):
    assert np.all(np.isfinite(got)), name
    err = np.abs(got.astype(np.float64) - r.v)
    assert np.all(err <= r.e), "%s: worst excess at %r" % (name, np.unravel_index((err - r.e).argmax(), err.shape))
  assert outs[0][0, 0] != W[39, 0] and outs[0][1, 0] == W[4, 0]


# ------------------------------------------------------------------ rk_scatter_pos / rk_rows_to_dense
@pytest.mark.parametrize("B", [1, 65, 300])
def test_scatter_pos_sets_and_clears(B):
  lib = _lib.load()
  users = np.random.RandomState(B).permutation(1000)[:B].astype(np.int64)
  pos = torch.full((1000,), -1, dtype=torch.int32, device="cuda")
  ud = dev_t(users)
  check(lib.rk_scatter_pos(ptr(pos), ptr(ud), B, 0, current_stream()), "rk_scatter_pos")
  want = np.full(1000, -1, np.int32)
  want[users] = np.arange(B)
  assert np.array_equal(pos.cpu().numpy(), want)
  check(lib.rk_scatter_pos(ptr(pos), ptr(ud), B, 1, current_stream()), "rk_scatter_pos")
  assert bool((pos == -1).all())


@pytest.mark.parametrize("n_items", [5, 257])
@pytest.mark.parametrize("h", [1, 4, 64])
def test_rows_to_dense_is_its_definition(n_items, h):
  lib = _lib.load()
  rng = np.random.RandomState(n_items + h)
  rows_pad = n_items + 7
  n_b = max(1, (2 * n_items) // 3)
  pos = np.full(n_items, -1, np.int32)
  pos[rng.permutation(n_items)[:n_b]] = rng.permutation(n_b)
  G = rng.randn(n_b, h).astype(np.float32)
  D = torch.full((rows_pad * h + 64,), CANARY, dtype=torch.float32, device="cuda")
  Gd, posd = dev_t(G), dev_t(pos)
  check(lib.rk_rows_to_dense(ptr(Gd), ptr(posd), n_items, rows_pad, h, ptr(D), current_stream()), "rk_rows_to_dense")
  torch.cuda.synchronize()
  want = np.zeros((rows_pad, h), np.float32)
  want[:n_items][pos >= 0] = G[pos[pos >= 0]]
  got = D.cpu().numpy()
  assert np.array_equal(got[:rows_pad * h].reshape(rows_pad, h), want)
  assert np.all(got[rows_pad * h:] == CANARY)


# ------------------------------------------------------------------ rk_mnll_row_stats / rk_mnll_finish
def _mnll_block(csr, B):
  """Rows 0..B of `csr` as a block over the WHOLE column range (no sampling: every column is live)."""
  users = torch.arange(B, dtype=torch.int64, device="cuda")
  return Block(B, max(1, csr.nnz), csr.shape[1], "cuda", negative_sampling=False).collate(DeviceCSR(csr), users)


def _row_stats(blk, logits, B, n):
  """rk_mnll_row_stats of logits [B, n] laid out with the block's ld > n, the padding columns at 1e30."""
  lib = _lib.load()
  n_b, _, ld, _ = blk.counts_host()
  assert n_b == n and ld > n
  L = torch.full((B, ld), 1e30, dtype=torch.float32, device="cuda")
  L[:, :n] = dev_t(logits)
  stats = torch.full((2 * B + 8,), CANARY, dtype=torch.float32, device="cuda")
  check(lib.rk_mnll_row_stats(ptr(L), B, blk.ref, ptr(stats), current_stream()), "rk_mnll_row_stats")
  torch.cuda.synchronize()
  st = stats.cpu().numpy()
  assert np.all(st[2 * B:] == CANARY)
  return L, st[:2 * B].reshape(B, 2)


def _finish(blk, L, B, inv_B, ext=None):
  lib = _lib.load()
  dO = L.clone()
  part = torch.zeros(B + 8, dtype=torch.float32, device="cuda")
  e = [dev_t(a) for a in ext] if ext else [None] * 3
  check(lib.rk_mnll_finish(ptr(dO), B, blk.ref, 0, inv_B, ptr(e[0]), ptr(e[1]), ptr(e[2]), ptr(part),
                           current_stream()), "rk_mnll_finish")
  torch.cuda.synchronize()
  return dO.cpu().numpy(), part[:B].cpu().numpy()


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("n_b", [1, 33, 300])
def test_mnll_row_stats_and_sharded_finish(B, n_b):
  n2 = 40                           # the second column shard; the first one holds the n_b columns under test
  N = n_b + n2
  rng = np.random.RandomState(B * 1000 + n_b)
  dense = (rng.rand(B, N) < 0.15) * (0.5 + 4.5 * rng.rand(B, N))
  dense[0, 0] = 2.0
  dense[B - 1, N - 1] = 3.0
  csr = sp.csr_matrix(dense.astype(np.float32))
  logits = rng.uniform(-60, 60, size=(B, N)).astype(np.float32)
  inv_B = float(np.float32(1.0 / B))          # (the argument is fp32)
  shards = [(0, n_b), (n_b, N)]
  blocks = [_mnll_block(csr[:, lo:hi].tocsr(), B) for lo, hi in shards]
  whole = _mnll_block(csr, B)

  # ---- the statistics of every shard and of the whole rows
  stats, Ls = [], []
  for blk, (lo, hi) in zip(blocks + [whole], shards + [(0, N)]):
    n = hi - lo
    L, st = _row_stats(blk, logits[:, lo:hi], B, n)
    x = logits[:, lo:hi]
    mx = x.max(axis=1)
    assert np.array_equal(st[:, 0], mx)                       # the maximum is exact
    S64 = np.exp((x - mx[:, None]).astype(np.float64)).sum(axis=1)      # exp of the fp32 differences
    # n - 1 adds in whatever order (gamma_n) and expf's measured figure per term; terms below fp32's normal
    # range may be flushed (2^-126 each)
    tol = ((1 + gamma(n)) * (1 + EXP_REL) - 1) * S64 + n * 2.0 ** -126
    assert np.all(np.abs(st[:, 1] - S64) <= tol), "n_b = %d" % n
    stats.append(st)
    Ls.append(L)

  # ---- the shards' statistics combined on the host (float64), then rk_mnll_finish per shard
  (sa, sb), t = stats[:2], dense.astype(np.float32).astype(np.float64)
  gmax = np.maximum(sa[:, 0], sb[:, 0])
  gsum = sa[:, 1].astype(np.float64) * np.exp(sa[:, 0].astype(np.float64) - gmax) + \
         sb[:, 1].astype(np.float64) * np.exp(sb[:, 0].astype(np.float64) - gmax)
  ext = (gmax.astype(np.float32), np.log(gsum).astype(np.float32), t.sum(axis=1).astype(np.float32))
  dO_w, part_w = _finish(whole, Ls[2], B, inv_B)
  got = [_finish(blk, L, B, inv_B, ext) for blk, L in zip(blocks, Ls[:2])]
  dO_s = np.concatenate([g[0][:, :hi - lo] for g, (lo, hi) in zip(got, shards)], axis=1)
  part_s = got[0][1].astype(np.float64) + got[1][1].astype(np.float64)

  # float64: log-softmax, loss per row, gradient
  x64 = logits.astype(np.float64)
  m64 = x64.max(axis=1, keepdims=True)
  lse = np.log(np.exp(x64 - m64).sum(axis=1, keepdims=True))          # relative to the maximum, as the kernels hold it
  lsm = x64 - m64 - lse
  tsum = t.sum(axis=1, keepdims=True)
  e64 = np.exp(lsm)
  Gs = tsum * inv_B                                                    # |sum_g|
  go64 = -t * inv_B + e64 * Gs
  d_abs = np.abs(x64 - m64)
  # Relative error of a path's sum of exponentials: the whole-row kernel chains 16 roundings and 3 expf (the
  # term, two rescales of the online softmax: one quad per thread up to 1024 columns); a shard's statistics
  # gamma_n and one expf, the host combination in float64.  lsum = log(sum) then carries that absolutely,
  # plus logf (taken at expf's figure) and the conversion: (EXP_REL + u) |lsum|.
  d_whole = gamma(16) + 3 * EXP_REL
  d_shard = gamma(max(n_b, n2)) + EXP_REL
  lerr = lambda d: d + (EXP_REL + U) * np.abs(lse)
  # e = expf((x - max) - lsum): both subtractions round (u |x - max|, then u (|x - max| + |lsum|)), expf adds its figure
  rho = lambda d: lerr(d) + U * (2 * d_abs + np.abs(lse)) + EXP_REL
  # sum_g: 11 roundings in the whole-row kernel (the products, one strided add, wave sum, 3 combines), 2 from row_tsum
  # dO = g - e * sum_g: two roundings per path (one if contracted), results below 2^-126 may be flushed
  tol_pair = e64 * Gs * (np.expm1(rho(d_whole)) + np.expm1(rho(d_shard)) + gamma(13)) * 1.001 + \
             2 * U * (e64 * Gs + np.abs(go64)) * 1.001 + 2.0 ** -125
  assert np.all(np.abs(dO_s.astype(np.float64) - dO_w[:, :N]) <= tol_pair)
  # against float64: one path, sum_g from row_tsum (2 roundings), and g = -t * inv_B rounds too
  tol_one = e64 * Gs * (np.expm1(rho(d_shard)) + gamma(2)) * 1.001 + U * (e64 * Gs + np.abs(go64) + t * inv_B) * 1.001 + \
            2.0 ** -126
  assert np.all(np.abs(dO_s - go64) <= tol_one)
  # the loss per row: -sum_t t lsm; lsm = (x - max) - lsum carries u |x - max| + u |lsm| + lerr; the product and the
  # sum over the row's entries (one strided add, wave sum, 3 combines, the add of the two shards): gamma_12
  loss64 = -(t * lsm).sum(axis=1)
  for part, d in ((part_s, d_shard), (part_w.astype(np.float64), d_whole)):
    tol = (t * (U * d_abs + U * np.abs(lsm) + lerr(d))).sum(axis=1) * 1.001 + gamma(12) * (t * np.abs(lsm)).sum(axis=1)
    assert np.all(np.abs(part - loss64) <= tol)


# ------------------------------------------------------------------ rk_loss_reduce
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_loss_reduce_sums_in_double_and_rezeroes(n):
  lib = _lib.load()
  rng = np.random.RandomState(n)
  x = (10.0 ** rng.uniform(-8, 4, size=n + 5) * np.where(rng.rand(n + 5) < 0.3, -1.0, 1.0)).astype(np.float32)
  denom = 37.0
  exact = math.fsum(float(a) for a in x[:n])
  # (the inputs leave the double sum's own error, n 2^-53 sum |x|, far below an fp32 ulp of the result)
  assert n * 2.0 ** -53 * float(np.abs(x[:n].astype(np.float64)).sum()) <= 2.0 ** -30 * abs(exact)
  part = dev_t(x)
  loss = torch.full((4,), CANARY, dtype=torch.float32, device="cuda")
  check(lib.rk_loss_reduce(ptr(part), n, denom, ptr(loss), current_stream()), "rk_loss_reduce")
  torch.cuda.synchronize()
  got = loss.cpu().numpy()
  # the double sum converted and divided in fp32: two roundings, at most one ulp off the rounded quotient
  assert eu.ulp_distance(got[:1], np.array([exact / denom]))[0] <= 1.0
  assert np.all(got[1:] == CANARY)
  p = part.cpu().numpy()
  assert np.all(p[:n] == 0) and np.array_equal(p[n:], x[n:])


# ------------------------------------------------------------------ rk_densify
def test_densify_equals_the_csr_rows():
  lib = _lib.load()
  lens = [0, 1, 7, 64, 65, 130, 20, 33, 2, 9]
  users_np = np.array([100 + 3 * r for r in range(len(lens))], dtype=np.int64)
  csr = eu.csr_with_row_lengths(lens, users_np, 140, 300, seed=3, ratings=True)
  users = dev_t(users_np)
  blk = Block(len(lens), sum(lens), 300, "cuda").collate(DeviceCSR(csr), users)
  n, nnz, _, _ = blk.counts_host()
  items = blk.items[:n].cpu().numpy().astype(np.int64)
  row_off, B, ld = 3, 5, n + 9
  out = torch.full((B * ld + 64,), CANARY, dtype=torch.float32, device="cuda")
  check(lib.rk_densify(blk.ref, row_off, B, n, ptr(out), ld, current_stream()), "rk_densify")
  torch.cuda.synchronize()
  got = out.cpu().numpy()
  dense = got[:B * ld].reshape(B, ld)
  want = csr[users_np[row_off:row_off + B]][:, items].toarray()
  assert want.any() and np.array_equal(dense[:, :n], want)
  # the kernel writes the n live columns only: columns [n, ld) are the caller's (the generic path passes
  # ld == n and relies on nothing behind the live columns)
  assert np.all(dense[:, n:] == CANARY) and np.all(got[B * ld:] == CANARY)
