"""GPU: ELSA (recoder_amd/elsa.py, rk_ease_elsa_* and rk_ease_csr_sub in librecoder_ease.so, LowRankShallowAutoencoder)
against the restatements of tests/elsa_util.py.

Tolerances.  normalize: 3 x 2^-24 relative, from the header's roundings (the sum of squares rounded once, halved by
the root; the root; the divide: 2.5 x 2^-24, and the second-order terms).  rows: the final f32 rounding of E and F,
2^-24 relative, against the float64 formulas with z2 and q summed in the header's order, plus 16 x 2^-52 of the terms
for the float64 roundings of the row scalars.  scatter and adam: bits.  serving: csr_scores against torch_forward within (h + 4) 2^-24 sum|terms|, the terms of a
score being |Z_uk A_jk| over k and |x_uj|; against float64 the f32 chain of Z adds nnz_u 2^-24 (|X| |A|) |A^T|.  One step's gradient:
at most 8 times the max-norm error of the float32 dense restatement against float64 on the same inputs (the ADMM fit
test's precedent for two f32 chains of different order).  On the slice: the golden interval of
tests/golden/elsa_slice.json (tools/elsa_bench.py --cpu-grid), inside which the float32 restatement lies as well."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import ease_util, elsa_util as eu

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(ease_util.SLICE), "elsa_slice.json")
# (n, h, B): every n of {1, 33, 129, 257}, every h of {1, 4, 63, 64, 65, 200, 512}, every B of {1, 37, 257}; the
# largest together once
SHAPES = [(1, 1, 1), (33, 4, 37), (129, 63, 37), (33, 64, 1), (129, 65, 257), (257, 200, 37), (257, 512, 257)]


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(rows, cols, pad=3, fill=-7.0, a=None):
  """A device buffer [rows + 1, cols + pad] filled with a sentinel (``a`` in its corner); (buffer, the [rows, cols] view)."""
  buf = torch.full((rows + 1, cols + pad), fill, dtype=torch.float32, device=DEV)
  if a is not None:
    buf[:rows, :cols] = _t(a)
  return buf, buf[:rows, :cols]


def _untouched(buf, rows, cols, fill=-7.0):
  h = buf.cpu().numpy()
  return bool(np.all(h[rows:] == fill) and np.all(h[:, cols:] == fill))


def _pair(m):
  from recoder_amd import als
  return als.csr_pair(m, m.shape[0], m.shape[1], DEV)


def _factors(n, h, seed=0):
  W = eu.initial_factors(n, h, seed)
  if n > 2:
    W[n // 2] = 0.0                              # (a zero-norm row)
  return W


# ------------------------------------------------------------------ normalize
@pytest.mark.parametrize("n,h,B", SHAPES)
def test_normalize_against_float64(n, h, B):
  from recoder_amd import elsa
  W = _factors(n, h) * np.float32(3.0)
  Wb, Wv = _padded(n, h, a=W)
  Ab, Av = _padded(n, h, pad=5)
  Tb, Tv = _padded(h, n, pad=2)
  norms = torch.full((n + 2,), -7.0, device=DEV)
  elsa.normalize(Wv, Av, norms[:n], Tv)
  A, T, nrm = Av.cpu().numpy(), Tv.cpu().numpy(), norms.cpu().numpy()
  assert _untouched(Ab, n, h) and _untouched(Tb, h, n) and np.all(nrm[n:] == -7.0) and _untouched(Wb, n, h)
  assert np.array_equal(Wv.cpu().numpy(), W)
  want_n = np.sqrt((W.astype(np.float64) ** 2).sum(1))
  want = W.astype(np.float64) / np.maximum(want_n, 1e-12)[:, None]
  assert np.all(np.isfinite(A)) and np.all(np.abs(A - want) <= 3 * U24 * np.abs(want))
  assert np.all(np.abs(nrm[:n] - want_n) <= 2 * U24 * want_n)
  if n > 2:
    assert not A[n // 2].any() and nrm[n // 2] == 0.0, "a zero row gives zeros"
  assert np.array_equal(_bits(T), _bits(A.T)), "A^T is not bitwise the transpose"
  wA, wn = eu.normalize_f32(W)
  assert np.array_equal(_bits(A), _bits(wA)) and np.array_equal(_bits(nrm[:n]), _bits(wn)), "the header's order"


# ----------------------------------------------------------------------- rows
def _rows_case(n, h, B, seed):
  """Z, Q, t2 (f32) of a real batch at random factors, with two constructed dead rows: t2 = 0 and p2 <= 0."""
  rng = np.random.RandomState(seed)
  X = eu.sparse_matrix(B, n, seed, values=True)
  A = eu.unit_rows(rng.randn(n, h)).astype(np.float32)
  Z = np.asarray(X @ A, np.float32)
  Q = (Z.astype(np.float64) @ (A.T.astype(np.float64) @ A)).astype(np.float32)
  t2 = np.asarray(X.multiply(X).sum(1)).ravel().astype(np.float32)
  dead = []
  if B > 1:                                     # (the empty row: t2 = 0; give it a Z that must not matter)
    assert t2[1] == 0
    Z[1] = 1.0
    dead.append(1)
  if B > 2:                                     # (Q = Z = ones, t2 = h / 2: p2 = h - 2 h + h / 2 < 0 with t2 > 0)
    Z[2], Q[2], t2[2] = 1.0, 1.0, np.float32(0.5 * h)
    dead.append(2)
  return Z, Q, t2, dead


@pytest.mark.parametrize("n,h,B", SHAPES)
def test_rows_against_the_float64_formulas(n, h, B):
  from recoder_amd import elsa
  Z, Q, t2, dead = _rows_case(n, h, B, seed=n + h + B)
  Eb, Ev = _padded(B, h)
  Fb, Fv = _padded(B, h, pad=1)
  _, Zv = _padded(B, h, pad=2, a=Z)
  _, Qv = _padded(B, h, pad=4, a=Q)
  rl = torch.full((B + 1,), -7.0, dtype=torch.float64, device=DEV)
  acc = torch.tensor([0.25, -7.0], dtype=torch.float64, device=DEV)
  elsa.rows(Zv, Qv, _t(t2), n, Ev, Fv, rl[:B], acc[:1])
  E, F, rl, acc = Ev.cpu().numpy(), Fv.cpu().numpy(), rl.cpu().numpy(), acc.cpu().numpy()
  assert _untouched(Eb, B, h) and _untouched(Fb, B, h) and rl[B] == -7.0 and acc[1] == -7.0
  # the reference takes z2 and q in the header's order (float64 sums in another order differ by h 2^-52 of their terms,
  # which the cancellation in p2 would carry into every entry): what is left is the final rounding of E and F to f32,
  # 2^-24 relative, and the float64 roundings of the row scalars, 16 x 2^-52 of the two terms of E
  wE, wF, wl, p2, ce, b = eu.rows64(Z, Q, t2, n, z2=eu.row_dot64(Z, Z), q=eu.row_dot64(Z, Q))
  assert np.all(np.isfinite(E)) and np.all(np.isfinite(F)) and np.all(np.isfinite(rl))
  for u in dead:
    assert p2[u] <= 0 or t2[u] == 0
    assert not E[u].any() and not F[u].any() and not np.signbit(E[u]).any(), "a dead row is exactly +0"
    assert rl[u] == (1.0 if t2[u] > 0 else 0.0)
  Z64, Q64 = Z.astype(np.float64), Q.astype(np.float64)
  mag = np.abs(ce)[:, None] * np.abs(Z64) + np.abs(b)[:, None] * np.abs(Q64)
  mag[dead] = 0.0
  assert np.all(np.abs(E - wE) <= U24 * np.abs(wE) + 16 * 2.0 ** -52 * mag + 1e-300)
  assert np.all(np.abs(F - wF) <= U24 * np.abs(wF) + 16 * 2.0 ** -52 * np.abs(wF) + 1e-300)
  assert np.all(np.abs(rl[:B] - wl) <= 1e-14)
  assert acc[0] == 0.25 + eu.loss_sum(rl[:B], float(B) * n), "the loss accumulator is not the fixed-order sum"


def test_rows_never_write_a_value_that_is_not_finite():
  """A live row by the letter whose factors leave the f32 range: Z = 1e-3, Q = 2 Z (q = 2 z2 exactly) and t2 the
  smallest f32 above 0, so p2 = t2 and b = 2 c / (B n p2) is of the order of 1e84.  The row is dead: E = F = +0; beside
  it an ordinary row keeps its values."""
  from recoder_amd import elsa
  Z = np.array([[1e-3], [0.5]], np.float32)
  Q = np.array([[2e-3], [0.5]], np.float32)
  t2 = np.array([np.nextafter(np.float32(0), np.float32(1)), 1.0], np.float32)
  E, F = torch.full((2, 1), -7.0, device=DEV), torch.full((2, 1), -7.0, device=DEV)
  rl = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
  acc = torch.zeros(1, dtype=torch.float64, device=DEV)
  elsa.rows(_t(Z), _t(Q), _t(t2), 5, E, F, rl, acc)
  E, F, rl, acc = E.cpu().numpy(), F.cpu().numpy(), rl.cpu().numpy(), acc.cpu().numpy()
  assert np.all(np.isfinite(E)) and np.all(np.isfinite(F)) and np.all(np.isfinite(rl)) and np.isfinite(acc[0])
  assert E[0, 0] == 0 and F[0, 0] == 0 and rl[0] in (0.0, 1.0)
  wE, wF, wl, _, _, _ = eu.rows64(Z[1:], Q[1:], t2[1:], 5)
  assert abs(E[1, 0] - wE[0, 0] / 2) <= U24 * abs(wE[0, 0]) and F[1, 0] != 0 and abs(rl[1] - wl[0]) <= 1e-14


# -------------------------------------------------------------------- scatter
def _scatter(X, lo, hi, E, n, h):
  """G of the range [lo, hi) of the item-major CSR of X, into a padded buffer; (G, untouched?)."""
  from recoder_amd import elsa
  _, icsr = _pair(X)
  Gb, Gv = _padded(n, h)
  Ev = None if lo == hi else _padded(hi - lo, h, pad=1, a=E)[1]
  elsa.scatter(icsr, lo, hi, Ev, Gv)
  return Gv.cpu().numpy(), _untouched(Gb, n, h)


@pytest.mark.parametrize("n,h,B", SHAPES)
def test_scatter_bit_for_bit(n, h, B):
  rng = np.random.RandomState(n + h)
  U = 2 * B + 5                                 # (the batch is a range in the middle, and a ragged tail)
  X = eu.sparse_matrix(U, n, seed=h + B, density=0.3, values=True)
  for lo, hi in ((3, 3 + B), (U - (B + 1) // 2, U), (4, 4)):
    E = rng.randn(max(hi - lo, 1), h).astype(np.float32)[:hi - lo]
    G, clean = _scatter(X, lo, hi, E, n, h)
    assert clean, "the padding of G was written"
    want = eu.scatter_chain(X[lo:hi], E) if hi > lo else np.zeros((n, h), np.float32)
    assert np.array_equal(_bits(G), _bits(want)), (lo, hi)
    if n >= 3:
      assert not G[n - 1].any(), "an item nobody holds gets zeros"
  # a row does not depend on the range's neighbours: other users around the same batch
  lo, hi = 3, 3 + B
  E = rng.randn(B, h).astype(np.float32)
  Y = sp.vstack([eu.sparse_matrix(3, n, 99, 0.5), X[lo:hi], eu.sparse_matrix(7, n, 98, 0.5)]).tocsr()
  assert np.array_equal(_bits(_scatter(X, lo, hi, E, n, h)[0]), _bits(_scatter(Y, 3, 3 + B, E, n, h)[0]))


def test_scatter_long_rows_take_the_same_chain():
  """An item every batch user holds: at B = 257 its row is past RK_EASE_ELSA_LONG (128) and goes to the workgroup
  path, at B = 100 the same users go to the wave path; both are the ascending chain."""
  n, h = 33, 65
  X = eu.sparse_matrix(300, n, seed=1, density=0.4, values=True).tolil()
  X[:, 0] = 2.0                                 # (every user, the empty one included)
  X = X.tocsr()
  E = np.random.RandomState(2).randn(257, h).astype(np.float32)
  for B in (257, 100):
    G, clean = _scatter(X, 20, 20 + B, E[:B], n, h)
    assert clean and np.array_equal(_bits(G), _bits(eu.scatter_chain(X[20:20 + B], E[:B]))), B


@pytest.mark.parametrize("h", [200, 512, 64])
def test_scatter_float4_path_bit_for_bit(h):
  """The path every fit takes: h a multiple of 4 and every row of E and G on a 16-byte boundary (paddings of 4 and 8
  columns, sentinels around both).  h = 512 uses both float4 chunks of a lane, h = 200 ends inside the first; the
  range of 257 sends the item everybody holds to the workgroup path and the others to the wave path, the range of 100
  sends all to the wave path; the scalar template (an odd stride) gives the same bits."""
  from recoder_amd import elsa
  n = 33
  X = eu.sparse_matrix(300, n, seed=1, density=0.4, values=True).tolil()
  X[:, 0] = 2.0
  X = X.tocsr()
  _, icsr = _pair(X)
  E = np.random.RandomState(h).randn(257, h).astype(np.float32)
  for B in (257, 100):
    Eb, Ev = _padded(B, h, pad=8, a=E[:B])
    Gb, Gv = _padded(n, h, pad=4)
    assert Ev.stride(0) % 4 == 0 and Gv.stride(0) % 4 == 0 and Ev.data_ptr() % 16 == 0 and Gv.data_ptr() % 16 == 0
    elsa.scatter(icsr, 20, 20 + B, Ev, Gv)
    G = Gv.cpu().numpy()
    assert _untouched(Gb, n, h) and _untouched(Eb, B, h), "the padding was written"
    assert np.array_equal(_bits(G), _bits(eu.scatter_chain(X[20:20 + B], E[:B]))), B
    assert np.array_equal(_bits(G), _bits(_scatter(X, 20, 20 + B, E[:B], n, h)[0])), "the scalar template differs"
    assert not G[n - 1].any()


# ----------------------------------------------------------------------- adam
@pytest.mark.parametrize("n,h,B", SHAPES)
@pytest.mark.parametrize("t", [1, 1000])
def test_adam_bit_for_bit(n, h, B, t):
  from recoder_amd import elsa
  rng = np.random.RandomState(n + h + t)
  W = _factors(n, h, 1)
  dA = (rng.randn(n, h) * 1e-4).astype(np.float32)
  m0 = (rng.randn(n, h) * 1e-4).astype(np.float32) if t > 1 else np.zeros((n, h), np.float32)
  v0 = (rng.rand(n, h) * 1e-8).astype(np.float32) if t > 1 else np.zeros((n, h), np.float32)
  A0, n0 = eu.normalize_f32(W)
  Wb, Wv = _padded(n, h, a=W)
  Ab, Av = _padded(n, h, pad=2, a=A0)
  _, dv = _padded(n, h, pad=1, a=dA)
  norms, M, V = _t(np.r_[n0, -7.0]), _t(m0), _t(v0)
  # the projection alone first: it is the g of the step
  dWb, dWv = _padded(n, h)
  elsa.project(dv, Av, norms[:n], dWv)
  assert _untouched(dWb, n, h)
  assert np.array_equal(_bits(dWv.cpu().numpy()), _bits(eu.project_f32(dA, A0, n0)))
  elsa.adam(Wv, dv, Av, norms[:n], M, V, 0.1, t)
  wW, wA, wn, wm, wv = eu.adam_f32(W, dA, A0, n0, m0, v0, t, 0.1)
  assert _untouched(Wb, n, h) and _untouched(Ab, n, h) and float(norms[n]) == -7.0
  for name, got, want in (("m", M, wm), ("v", V, wv), ("W", Wv, wW), ("A", Av, wA), ("norms", norms[:n], wn)):
    got = got.cpu().numpy()
    assert np.all(np.isfinite(got)), name
    assert np.array_equal(_bits(got), _bits(want)), name
  assert np.array_equal(dv.cpu().numpy(), dA), "dA was written"


# ------------------------------------------------------------ csr_sub, serving
@pytest.mark.parametrize("n,h,B", SHAPES)
def test_serving_strips_and_torch_forward(n, h, B):
  from recoder_amd import elsa
  from recoder_amd.nn import LowRankShallowAutoencoder
  X = eu.sparse_matrix(B, n, seed=n + B, values=True)
  ucsr, _ = _pair(X)
  # csr_sub alone: only the stored entries of the strip move, by exactly x
  lo, hi = (n // 3, n - n // 4) if n > 3 else (0, n)
  buf, view = _padded(B, hi - lo, a=np.full((B, hi - lo), 0.5, np.float32))
  elsa.csr_sub(ucsr, lo, hi, view, buf.stride(0), B)
  want = 0.5 - np.asarray(X.todense(), np.float32)[:, lo:hi]
  assert _untouched(buf, B, hi - lo) and np.array_equal(view.cpu().numpy(), want)
  m = LowRankShallowAutoencoder(h)
  m.init_model(num_items=n)
  m.to(DEV)
  m.item_factors.data.copy_(_t(_factors(n, h, 2)))
  m._weights_written()
  whole = m.csr_scores(ucsr, 0, n, None, None, B).cpu().numpy()
  cuts = sorted({0, n // 3, n // 2 + 1, n} - {n + 1}) if n > 3 else [0, n]
  out = torch.full((B, n + 3), -7.0, device=DEV)
  for a, b in zip(cuts[:-1], cuts[1:]):
    strip = torch.full((B + 1, (b - a) + 2), -7.0, device=DEV)
    m.csr_scores(ucsr, a, b, strip, strip.stride(0), B)
    s = strip.cpu().numpy()
    assert np.all(s[B:] == -7.0) and np.all(s[:, b - a:] == -7.0)
    assert np.array_equal(_bits(s[:B, :b - a]), _bits(whole[:, a:b])), "a strip is not the whole call's bits"
  A = eu.normalize_f32(m.item_factors.data.cpu().numpy())[0].astype(np.float64)
  X64 = np.asarray(X.todense(), np.float64)
  Z = X64 @ A
  want = Z @ A.T - X64
  terms = np.abs(Z) @ np.abs(A.T) + np.abs(X64)          # (sum_k |Z_uk A_jk| + |x_uj|: the terms of one score)
  fwd = m.torch_forward(torch.as_tensor(np.asarray(X.todense(), np.float32), device=DEV)).cpu().numpy()
  bound = (h + 4) * U24 * terms
  print("serving n=%d h=%d B=%d: max |csr_scores - torch_forward| / ((h + 4) 2^-24 terms) = %.3g; against float64 %.3g"
        % (n, h, B, (np.abs(whole - fwd) / np.maximum(bound, 1e-300)).max(),
           (np.abs(whole - want) / np.maximum(bound, 1e-300)).max()))
  assert np.all(np.abs(whole - fwd) <= bound), "csr_scores and torch_forward differ by more than the product's bound"
  # against float64 the chain of Z counts too: nnz_u roundings of sum |x_uj A_jk| <= |X| |A|, carried through the product,
  # beside the product's h + 4 (of which the subtraction is one)
  chain = (X.getnnz(1)[:, None] * U24 * (np.abs(X64) @ np.abs(A))) @ np.abs(A.T)
  assert np.all(np.abs(whole - want) <= bound + chain)
  dense = m(torch.as_tensor(np.asarray(X.todense(), np.float32), device=DEV)).cpu().numpy()
  assert np.array_equal(_bits(dense), _bits(whole)), "forward() of a dense batch is csr_scores"


# ------------------------------------------------------- one step's gradient
@pytest.mark.parametrize("n,h,B", SHAPES)
def test_one_steps_gradient_against_the_float64_dense_formulation(n, h, B):
  """Measured on an MI355X, the kernels' max-norm error over the float32 dense restatement's on the same inputs, by
  (n, h, B): (33, 4, 37) 1.09, (129, 63, 37) 0.98, (33, 64, 1) 1.14, (129, 65, 257) 1.60, (257, 200, 37) 1.00,
  (257, 512, 257) 2.03; at (1, 1, 1) both errors are 0.  The bound is 8."""
  from recoder_amd import elsa
  U = B + 4
  X = eu.sparse_matrix(U, n, seed=n + h + B, density=0.3, values=True)
  W = eu.initial_factors(n, h, 3)
  lo, hi = 2, 2 + B
  loss64, g64 = eu.dense(X[lo:hi], W.astype(np.float64))
  loss32, g32 = eu.dense(X[lo:hi], W, torch.float32)
  loss, dW = elsa.gradient(_pair(X), _t(W), lo, hi)
  dW = dW.cpu().numpy()
  assert np.all(np.isfinite(dW)) and np.isfinite(loss)
  e32, egpu = np.abs(g32 - g64).max(), np.abs(dW - g64).max()
  print("gradient n=%d h=%d B=%d: kernels %.3g, f32 dense %.3g (ratio %.2f); loss %.3g vs %.3g"
        % (n, h, B, egpu, e32, egpu / max(e32, 1e-300), abs(loss - loss64), abs(loss32 - loss64)))
  if e32 == 0.0:                                 # (n = 1 or h = 1: the gradient is exactly zero in every precision)
    assert np.abs(g64).max() <= 1e-12 * max(np.abs(X[lo:hi]).max(), 1.0) and egpu <= 8 * U24 * 1e-3
  else:
    assert egpu <= 8 * e32
  assert abs(loss - loss64) <= 8 * max(abs(loss32 - loss64), U24 * abs(loss64))


# ---------------------------------------------------------------- determinism
def test_two_fits_with_one_seed_give_the_same_bits():
  from recoder_amd import elsa
  X = eu.sparse_matrix(300, 129, seed=5, density=0.2, values=True)
  fits = [elsa.fit(_pair(X), 65, 2, 128, 0.1, seed) for seed in (7, 7, 8)]
  W = [f[0].cpu().numpy() for f in fits]
  assert np.all(np.isfinite(W[0])) and np.array_equal(_bits(W[0]), _bits(W[1])) and fits[0][1] == fits[1][1]
  assert not np.array_equal(_bits(W[0]), _bits(W[2]))
  assert len(fits[0][1]) == 2 and fits[0][1][1] < fits[0][1][0], "the loss goes down"


# ---------------------------------------------------------------- on the slice
def _slice():
  z = np.load(ease_util.SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


@pytest.fixture(scope="module")
def golden():
  return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def fitted(golden):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  x, y = _slice()
  p = golden["point"]
  rec = Recoder(model=LowRankShallowAutoencoder(p["embedding_size"]))
  hist = rec.train_elsa(RecommendationDataset(x), num_epochs=p["num_epochs"], batch_size=p["batch_size"], lr=p["lr"])
  return rec, hist, x, y


def test_the_fit_on_the_slice_lies_in_the_golden_interval(fitted, golden):
  """The float64 restatement's values for the seeds 0..4, their range widened by its own width on each side: another
  rounding is treated as another seed.  The float32 restatement lies inside it (golden["float32_inside"])."""
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  rec, hist, x, y = fitted
  assert golden["float32_inside"] is True
  assert golden["point"] == {"embedding_size": 64, "num_epochs": 5, "lr": 0.1, "batch_size": 1024}
  assert hist == rec.elsa_history and len(hist) == 5 and all(np.isfinite(hist)) and hist[-1] < hist[0]
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
  r20, n100 = got[str(Recall(k=20))], got[str(NDCG(k=100))]
  print("ELSA on the slice (h 64, 5 epochs): Recall@20 %.6f in %s; NDCG@100 %.6f in %s; loss %s"
        % (r20, golden["recall20_interval"], n100, golden["ndcg100_interval"], hist))
  for name, v in (("recall20", r20), ("ndcg100", n100)):
    lo, hi = min(golden[name]), max(golden[name])
    assert golden[name + "_interval"] == [lo - (hi - lo), hi + (hi - lo)]
    assert lo - (hi - lo) <= v <= hi + (hi - lo), name


def test_checkpoint_round_trip_and_what_the_model_plugs_into(fitted, tmp_path):
  from recoder_amd.data import UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  rec, _, x, _ = fitted
  f = rec.save_state(str(tmp_path / "elsa"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == {"embedding_size": 64} and list(st["model"]) == ["item_factors"]
  rec2 = Recoder(model=LowRankShallowAutoencoder(9))
  rec2.init_from_model_file(f)
  assert rec2.model.model_params() == rec.model.model_params()
  inp = UsersInteractions(np.arange(300), x[:300])
  lists = rec.recommend_array(inp, 20)
  assert np.array_equal(lists, rec2.recommend_array(inp, 20))
  seen = x[:300]
  for u in range(300):
    assert not set(lists[u]) & set(seen.indices[seen.indptr[u]:seen.indptr[u + 1]]), "recommend masks seen items"
  # strips give the same lists
  rec.eval_strip_items = 3000
  try:
    assert np.array_equal(rec.recommend_array(inp, 20), lists)
  finally:
    del rec.eval_strip_items
  # predict is x (A A^T - I) from the stored factors
  scores = rec.predict(UsersInteractions(np.arange(50), x[:50]))[0].cpu().numpy()
  W = rec.model.item_factors.data.cpu().numpy()
  want = eu.scores(x[:50], W)
  assert np.abs(scores[:, :x.shape[1]] - want).max() <= (64 + 4) * U24 * 4 * np.abs(want).max()
  with pytest.raises(ValueError, match="train_elsa"):
    from recoder_amd.data import RecommendationDataset
    rec.train(RecommendationDataset(x))


def test_a_refit_reuses_the_buffer_and_refreshes_the_images():
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  X = eu.sparse_matrix(300, 129, seed=5, density=0.2)
  rec = Recoder(model=LowRankShallowAutoencoder(8))
  ds = RecommendationDataset(X)
  h1 = rec.train_elsa(ds, num_epochs=1, batch_size=64, lr=0.1)
  where = rec.model.item_factors.data_ptr()
  inp = UsersInteractions(np.arange(40), X[:40])
  p1 = rec.predict(inp)[0].cpu().numpy().copy()
  h3 = rec.train_elsa(ds, num_epochs=3, batch_size=64, lr=0.1)
  assert rec.model.item_factors.data_ptr() == where and len(h3) == 3 and h3[0] == h1[0] and rec.elsa_history == h3
  p3 = rec.predict(inp)[0].cpu().numpy()
  want = eu.scores(X[:40], rec.model.item_factors.data.cpu().numpy())
  assert not np.array_equal(p1, p3) and np.abs(p3[:, :129] - want).max() <= 1e-5, "the images were not taken again"
