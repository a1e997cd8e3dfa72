"""GPU: the SimGCL kernels (rk_als_gcl_* of librecoder_als.so) and recoder_amd/simgcl.py against the restatement of
tests/simgcl_util.py -- the noisy propagation against float64 within the rounding of its own f32 chain and bit for
bit against rk_als_lgcn_propagate at eps = 0, the contrast against float64 within a bound worked out from its
chains, one whole step, and Recoder.train_simgcl end to end with what the fitted tables plug into."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util, lightgcn_util as lg, simgcl_util as sg

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
f32 = lambda v: float(np.float32(v))                           # (f32 values: the kernels take floats)
LR, REG, W, EPS, TAU = f32(0.05), f32(1e-3), f32(0.5), f32(0.1), f32(0.2)


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, ld, fill=7.0):
  """A [rows, h] view with leading dimension ld of a tensor filled with ``fill`` (the padding must stay so)."""
  a = np.asarray(a, np.float32)
  full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  full[:, :a.shape[1]] = _t(a)
  return full, full[:, :a.shape[1]]


def _csr(m):
  from recoder_amd import als
  return als.AlsCSR(m, DEV)


# ---------------------------------------------------------------- propagate
def _hand_matrix():
  """37 x 23: row 5 empty, column 7 empty, row 9 holds one entry, row 12 every column but the empty one."""
  rng = np.random.RandomState(7)
  m = (rng.rand(37, 23) < 0.3).astype(np.float32)
  m[5, :] = 0
  m[9, :] = 0
  m[9, 4] = 1
  m[12, :] = 1
  m[:, 7] = 0
  return m


def _long_matrix():
  """8 x (LONG_ROW + 5): rows 3, 4, 5 hold LONG_ROW - 1, LONG_ROW, LONG_ROW + 1 entries, row 6 none."""
  from recoder_amd.lightgcn import LONG_ROW
  rng = np.random.RandomState(8)
  n = LONG_ROW + 5
  m = (rng.rand(8, n) < 0.02).astype(np.float32)
  for r, c in ((3, LONG_ROW - 1), (4, LONG_ROW), (5, LONG_ROW + 1)):
    m[r, :] = 0
    m[r, rng.permutation(n)[:c]] = 1
  m[6, :] = 0
  return m


def _oriented(name):
  m = sp.csr_matrix(_hand_matrix() if name.startswith("hand") else _long_matrix())
  su, si = lg.scales(m)
  if name.endswith("T"):
    return lg.transpose(m), si, su
  m.sort_indices()
  return m, su, si


KEY = dict(seed=11, step=3, view=1, layer=2, side=0)


def _propagate_gpu(csr, rs, cs, F, ld_pad, eps=EPS, out=True, acc=None, acc_scale=1.0, row_lo=0, row_hi=None,
                   lgcn=False, **key):
  """(Out, Acc) as numpy after one rk_als_gcl_propagate (``lgcn``: rk_als_lgcn_propagate); the padding columns
  must stay 7."""
  from recoder_amd import lightgcn, simgcl
  h = F.shape[1]
  Ffull, Fv = _padded(F, h + ld_pad)
  rows = csr.shape[0]
  Ofull, Ov = _padded(np.full((rows, h), 7.0), h + ld_pad) if out else (None, None)
  Afull, Av = _padded(acc, h + ld_pad) if acc is not None else (None, None)
  if lgcn:
    lightgcn.propagate(csr, _t(rs), _t(cs), Fv, Ov, Av, acc_scale, row_lo, row_hi)
  else:
    simgcl.propagate(csr, _t(rs), _t(cs), Fv, Ov, Av, acc_scale, eps, row_lo=row_lo, row_hi=row_hi, **dict(KEY, **key))
  for full in (Ofull, Afull):
    assert full is None or bool((full[:, h:] == 7.0).all()), "a padding column was written"
  return (Ov.cpu().numpy() if out else None), (Av.cpu().numpy() if acc is not None else None)


@pytest.mark.parametrize("h", [1, 4, 64, 65, 200, 300])      # (300: two float4s, or five floats, per lane)
def test_noisy_propagate_against_float64(h):
  worst, ambiguous, elements = 0.0, 0, 0
  for name in ("hand", "handT", "long", "longT"):
    m, rs, cs = _oriented(name)
    csr = _csr(m)
    rng = np.random.RandomState(h + len(name))
    F = rng.randn(m.shape[1], h).astype(np.float32)
    acc0 = rng.randn(m.shape[0], h).astype(np.float32)
    empty = np.diff(m.indptr) == 0
    assert empty.any() or name == "longT"
    key = sg.noise_key(**KEY)
    outs = []
    for ld_pad in (0, 3):
      out, _ = _propagate_gpu(csr, rs, cs, F, ld_pad)
      ratio, amb = sg.noisy_errors(out, m, rs, cs, F, EPS, key)
      worst, ambiguous, elements = max(worst, ratio.max()), ambiguous + int(amb.sum()), elements + amb.size
      assert ratio.max() <= 1, (name, ld_pad)
      assert not out[empty].any() and not np.signbit(out[empty]).any()
      # the noise has length eps on every row that holds an entry (those without a zero element)
      clean, _ = _propagate_gpu(csr, rs, cs, F, ld_pad, lgcn=True)
      full = ~empty & (clean != 0).all(1)
      d = out.astype(np.float64) - clean
      assert np.all((np.sign(d[full]) == np.sign(clean[full])) | (d[full] == 0))       # (0: lost in out's rounding)
      # (out - clean carries out's rounding, 2^-24 |out| an element; eps / |u| and the products, four roundings)
      lim = U24 * np.sqrt((out[full].astype(np.float64) ** 2).sum(1)) + 4 * U24 * EPS
      assert np.all(np.abs(np.sqrt((d[full] ** 2).sum(1)) - EPS) <= lim)
      zero, _ = _propagate_gpu(csr, rs, cs, F, ld_pad, eps=0.0)
      assert np.array_equal(zero, clean) and np.array_equal(np.signbit(zero), np.signbit(clean)), \
          "eps = 0 is not rk_als_lgcn_propagate"
      again, _ = _propagate_gpu(csr, rs, cs, F, ld_pad)
      assert np.array_equal(out, again), "not bitwise repeatable"
      outs.append(out)
      for scale, with_out in ((1.0, True), (0.25, True), (0.25, False)):
        o2, acc = _propagate_gpu(csr, rs, cs, F, ld_pad, out=with_out, acc=acc0, acc_scale=scale)
        assert o2 is None or np.array_equal(o2, out)
        # the accumulate is two more f32 operations on the rounded, perturbed Out, exactly
        assert np.array_equal(acc, (acc0 + out) * np.float32(scale))
      zacc = _propagate_gpu(csr, rs, cs, F, ld_pad, eps=0.0, out=False, acc=acc0, acc_scale=0.25)[1]
      assert np.array_equal(zacc, _propagate_gpu(csr, rs, cs, F, ld_pad, out=False, acc=acc0, acc_scale=0.25, lgcn=True)[1])
      lo, hi = 3, min(11, m.shape[0])
      part, _ = _propagate_gpu(csr, rs, cs, F, ld_pad, row_lo=lo, row_hi=hi)
      assert np.array_equal(part[lo:hi], out[lo:hi]) and np.all(part[:lo] == 7.0) and np.all(part[hi:] == 7.0)
    assert np.array_equal(outs[0], outs[1]), "the leading dimension (16-byte accesses or not) changed the bits"
    nz = ~empty
    for other in (dict(view=2), dict(layer=1), dict(step=4), dict(seed=12), dict(side=1)):
      o, _ = _propagate_gpu(csr, rs, cs, F, 0, **other)
      assert h == 1 or np.all((o[nz] != outs[0][nz]).any(1)), other           # (h = 1: u / |u| = 1 whatever the key)
  print("h %d: largest err / (2 x bound) %.3f, ambiguous signs %d of %d" % (h, worst, ambiguous, elements))
  assert ambiguous <= 0.01 * elements


def test_a_long_row_and_a_short_row_of_one_key_take_the_same_noise():
  """Rows 4 and 5 of the long matrix are the long kernel's (a workgroup, the waves' sums meeting in LDS), the others
  the short one's (a group of lanes).  |u[r]| is an integer sum and every later operation is one correctly rounded
  f32 operation on known operands, so both kernels must give the bits of the restatement's float32 form on the
  kernel's own unperturbed row."""
  m, rs, cs = _oriented("long")
  for h in (4, 65, 300):
    F = np.ones((m.shape[1], h), np.float32)
    out, _ = _propagate_gpu(_csr(m), rs, cs, F, 0)
    clean, _ = _propagate_gpu(_csr(m), rs, cs, F, 0, lgcn=True)
    want = sg.perturb(clean, EPS, sg.noise_key(**KEY), np.float32)
    assert np.array_equal(out, want), h


# ----------------------------------------------------------------- contrast
def _contrast_gpu(keys, V1, V2, tau=TAU, w=W, ld_pad=3, G0=None):
  """(loss, m, G1, G2) after one rk_als_gcl_contrast; V1 and G1 with a padded leading dimension."""
  from recoder_amd import simgcl
  T, (n, h) = len(keys), V1.shape
  V1full, V1v = _padded(V1, h + ld_pad)
  G1full, G1v = _padded(np.zeros((n, h)) if G0 is None else G0, h + ld_pad)
  G2 = _t(np.zeros((n, h)) if G0 is None else G0)
  raw = torch.empty(simgcl.contrast_workspace_bytes(T, h), dtype=torch.uint8, device=DEV)
  loss, count = torch.full((1,), 7.0, device=DEV), torch.full((1,), 7, dtype=torch.int32, device=DEV)
  simgcl.contrast(_t(keys, np.int32), V1v, _t(V2), tau, w, G1v, G2, raw, loss, count)
  assert bool((V1full[:, h:] == 7.0).all()) and bool((G1full[:, h:] == 7.0).all()), "a padding column was written"
  return float(loss.item()), int(count.item()), G1v.cpu().numpy(), G2.cpu().numpy()


def _contrast_case(T, h):
  """Sorted keys from a 40-row table (duplicates from T = 65 on), about a tenth of the slots invalid (the sentinel
  40, and one -1), and row ``zero`` of view 1 all zeros although its key is active."""
  rng = np.random.RandomState(T * 1000 + h)
  V1, V2 = rng.randn(40, h).astype(np.float32), rng.randn(40, h).astype(np.float32)
  if T <= 2:
    keys = np.array([3, 9][:T], np.int32)
  else:
    keys = rng.randint(0, 40, T).astype(np.int32)
    keys[rng.rand(T) < 0.1] = 40
    keys[0] = -1
    keys[1] = 40
  keys = np.sort(keys)
  zero = int(keys[keys >= 0][-1 if T <= 2 else 0]) if T > 1 else None
  if zero is not None:
    V1[zero] = 0
  return keys, V1, V2, zero


def _contrast_bounds(keys, V1, V2, tau, w):
  """First-order bounds (loss, G1, G2) of the f32 contrast against float64, u = 2^-24, every chain at its
  length: z = v / |v| carries (h + 3) u (h products under the root, the root, the division, the product); a score
  sums h products of |z| <= 1 factors, so eS = (3 h + 7) u / tau; expf and logf are good to 1 ulp (HIP's table
  of device functions); a row's lse takes both S and its maximum, T terms and the logarithm:
  e_lse = 3 eS + (T + 2 / tau + 4 + |lse|) u; P = exp(S - lse) then carries eP = eS + e_lse + (|S - lse| + 2) u
  relatively.  dz = (sum_s P z - z) c with sum_s P_rs = 1 across a row and the column sums down a column; the
  normalisation's backward adds a dot of h products.  The whole is doubled for the terms of second order."""
  T, h = len(keys), V1.shape[1]
  u = U24
  sk, act = sg.active(keys, V1.shape[0])
  idx = sk[act]
  m = len(idx)
  B1, B2 = np.zeros(V1.shape), np.zeros(V2.shape)
  if m == 0:
    return 0.0, B1, B2
  z, inv = [], []
  for V in (V1, V2):
    v = V[idx].astype(np.float64)
    n = np.sqrt((v * v).sum(1))
    i = np.where(n > 0, 1 / np.where(n > 0, n, 1), 0)
    inv.append(i[:, None])
    z.append(v * i[:, None])
  S = z[0] @ z[1].T / tau
  lse = np.log(np.exp(S - S.max(1)[:, None]).sum(1)) + S.max(1)
  P = np.exp(S - lse[:, None])
  eS = (3 * h + 7) * u / tau
  e_lse = 3 * eS + (T + 2 / tau + 4 + np.abs(lse).max()) * u
  term = lse - np.diag(S)
  e_loss = e_lse + eS + (T + 3) * u * np.abs(term).max()
  eP = eS + e_lse + (np.abs(S - lse[:, None]).max() + 2) * u
  c = 1 / (tau * m)
  for B, zz, other, Pm, i in ((B1, z[0], z[1], P, inv[0]), (B2, z[1], z[0], P.T, inv[1])):
    dz = (Pm @ other - other) * c
    mass = Pm.sum(1)[:, None]                                  # (1 across a row of P, the column sum down a column)
    e_dz = (mass * (eP + (h + 3 + T) * u) + (h + 5) * u) * c + 3 * u * np.abs(dz)
    dot = (zz * dz).sum(1)[:, None]
    e_dot = (np.abs(zz) * e_dz).sum(1)[:, None] + (2 * h + 3) * u * (np.abs(zz) * np.abs(dz)).sum(1)[:, None]
    dv = (dz - zz * dot) * i
    e_dv = i * (e_dz + np.abs(zz) * e_dot + (h + 5) * u * (np.abs(dz) + np.abs(zz * dot))) + (h + 6) * u * np.abs(dv)
    B[idx] = w * e_dv
  return 2 * e_loss, 2 * B1, 2 * B2


@pytest.mark.parametrize("h", [1, 4, 65, 200])
@pytest.mark.parametrize("T", [1, 2, 65, 300])
def test_contrast_against_float64(T, h):
  keys, V1, V2, zero = _contrast_case(T, h)
  _, act = sg.active(keys, 40)
  if T >= 65:
    assert (keys == 40).any() and (keys == -1).any() and act.sum() < (keys < 40).sum() - 1      # invalid, duplicates
  wl, wm, wG1, wG2 = sg.contrast(keys, V1, V2, TAU)
  loss, m, G1, G2 = _contrast_gpu(keys, V1, V2)
  bl, B1, B2 = _contrast_bounds(keys, V1, V2, TAU, W)
  assert m == wm == act.sum()
  ratios = [abs(loss - wl) / max(bl, 1e-300)] + [(np.abs(G - W * wG) / np.maximum(B, 1e-300)).max()
                                                for G, wG, B in ((G1, wG1, B1), (G2, wG2, B2))]
  print("T %d h %d: m %d, loss %.6g (float64 %.6g), err / bound: loss %.3f, G1 %.3f, G2 %.3f" % (T, h, m, loss, wl, *ratios))
  assert abs(loss - wl) <= bl and np.all(np.abs(G1 - W * wG1) <= B1) and np.all(np.abs(G2 - W * wG2) <= B2)
  inactive = np.setdiff1d(np.arange(40), keys[act])
  assert not G1[inactive].any() and not G2[inactive].any()
  if T == 1:
    assert loss == 0 and not G1.any() and not G2.any()
  else:
    assert loss > 0 and not G1[zero].any()                                     # |v1| = 0: z1 = 0, its gradient 0
    if h > 1:                                                                  # (h = 1: z = +-1, no gradient passes)
      assert G2[zero].any() and G1[np.setdiff1d(keys[act], [zero])].any(1).all()
  again = _contrast_gpu(keys, V1, V2)
  assert again[:2] == (loss, m) and np.array_equal(again[2], G1) and np.array_equal(again[3], G2), "not repeatable"


def test_contrast_adds_to_the_tables_and_takes_one_table_for_both_views():
  from recoder_amd import simgcl
  keys, V1, V2, _ = _contrast_case(65, 24)
  G0 = np.random.RandomState(0).randn(40, 24).astype(np.float32)
  _, _, G1, G2 = _contrast_gpu(keys, V1, V2, ld_pad=0)
  _, _, A1, A2 = _contrast_gpu(keys, V1, V2, ld_pad=0, G0=G0)
  assert np.array_equal(A1, G0 + G1) and np.array_equal(A2, G0 + G2)
  G = _t(G0)
  raw = torch.empty(simgcl.contrast_workspace_bytes(65, 24), dtype=torch.uint8, device=DEV)
  loss, count = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
  simgcl.contrast(_t(keys, np.int32), _t(V1), _t(V2), TAU, W, G, G, raw, loss, count)
  assert np.array_equal(G.cpu().numpy(), (G0 + G1) + G2)                       # (view 1, then view 2)
  allbad = np.array([-1, 40, 40], np.int32)
  l, m, B1, B2 = _contrast_gpu(allbad, V1, V2)
  assert l == 0 and m == 0 and not B1.any() and not B2.any()


# ---------------------------------------------------------------- one step
def _graph(tr):
  from recoder_amd import als, lightgcn
  return lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))


def _clean_bound(tr, Eu, Ei, K):
  """tests/test_lightgcn.py's ``_final_bound`` for the mean over the layers 1..K: K chains of at most Lmax products
  with three more roundings each, the K - 1 roundings of the layer sum and the rounding of 1 / K and of its product."""
  Lmax = max(np.diff(tr.indptr).max(), np.diff(lg.transpose(tr).indptr).max())
  aP, aQ = sg.forward(tr, np.abs(Eu), np.abs(Ei), K)
  f = (K * (Lmax + 3) + K + 1) * U24
  return f * aP, f * aQ


@pytest.mark.parametrize("w", [W, 0.0])
def test_one_full_step_against_the_restatement_on_the_same_triples(w):
  from recoder_amd import simgcl
  tr, _ = bpr_util.planted()
  h, K, T = 24, 2, 256
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = _graph(tr)
  state = simgcl.new_state(X, Y, K)
  ws = simgcl.Workspace(200, 120, T, h, DEV, contrast=w > 0)
  simgcl.step(X, Y, graph, state, ws, 11, 3, LR, REG, w, EPS, TAU)
  users, pos, neg = (v.cpu().numpy() for v in (ws.bpr.users, ws.bpr.pos, ws.bpr.neg))
  wu, wp, wn = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and np.array_equal(neg, wn)
  assert state["step"] == 1
  # X, Y hold the clean tables of the start of the step
  for name, got, want, bound in zip("PQ", (X, Y), sg.forward(tr, Eu, Ei, K), _clean_bound(tr, Eu, Ei, K)):
    err = np.abs(got.cpu().numpy() - want)
    print("clean %s: max err / (2 x bound) %.3f" % (name, (err / np.maximum(2 * bound, 1e-300)).max()))
    assert np.all(err <= 2 * bound), name
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  _, _, cl64 = sg.step(tr, s64, K, users, pos, neg, LR, REG, w, EPS, TAU, 11, 3)
  _, _, cl32 = sg.step(tr, s32, K, users, pos, neg, LR, REG, w, EPS, TAU, 11, 3, np.float32)
  cl = float(ws.cl_loss.sum().item())
  ok = neg >= 0
  print("cl_weight %g: NCE users + items: kernels %.6f, f32 restatement %.6f, float64 %.6f" % (w, cl, cl32, cl64))
  if w > 0:
    assert ws.cl_count.cpu().tolist() == [len(set(users[ok])), len(set(pos[ok]))] and cl64 > 0 and cl > 0
  else:
    assert cl == 0 and not hasattr(ws, "views")
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      dist = np.abs(s32[key][side] - s64[key][side]).max()
      err = np.abs(state[key][side].cpu().numpy() - s64[key][side]).max()
      print("step %s[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (key, side, dist, err))
      assert dist > 0 and err <= 4 * dist, (key, side)


# -------------------------------------------------------------- end to end
def _recoder(h=16):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _tables(rec):
  m = rec.model
  return tuple(p.detach().cpu().numpy().copy() for p in
               (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


def _train(tr, seed, start, epochs=(5,)):
  """train_simgcl on the planted matrix from the base tables ``start`` (set after an empty fit has built the
  model); more than one entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder()
  ds = RecommendationDataset(tr)
  kw = dict(num_layers=2, batch_size=256, lr=LR, reg=REG, cl_weight=W, cl_eps=EPS, cl_temperature=TAU, seed=seed)
  assert rec.train_simgcl(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  hist = []
  for k, n in enumerate(epochs):
    hist += rec.train_simgcl(ds, num_epochs=n, resume=k > 0, **kw)
  return rec, hist, _tables(rec)


@pytest.fixture(scope="module")
def planted_fit():
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)[:2]
  rec, hist, tables = _train(tr, 0, start)
  return tr, ho, start, rec, hist, tables


def test_train_simgcl_lowers_both_losses_repeats_and_resumes_bit_for_bit(planted_fit):
  tr, _, start, rec, hist, tables = planted_fit
  assert len(hist) == 5 and rec.simgcl_history == hist and np.all(np.isfinite(hist))
  assert all(b < hist[0][0] and c < hist[0][1] for b, c in hist[1:]), hist
  st = rec.simgcl_state
  assert st["num_layers"] == 2 and st["step"] == 5 * -(-tr.nnz // 256) and st["E0"][0].is_cuda
  assert rec.lightgcn_state is None and rec.lightgcn_history == []
  _, hist2, again = _train(tr, 0, start)
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist
  _, _, other = _train(tr, 1, start)
  assert not np.array_equal(tables[0], other[0]) and not np.array_equal(tables[1], other[1])
  rec3, hist3, resumed = _train(tr, 0, start, epochs=(2, 3))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist
  from recoder_amd.data import RecommendationDataset
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 3\\)"):
    rec3.train_simgcl(RecommendationDataset(tr), num_layers=3, num_epochs=1, resume=True)
  assert all(np.array_equal(a, b) for a, b in zip(resumed, _tables(rec3)))


def test_held_out_auc_beside_the_float64_restatement(planted_fit):
  """The yardstick is the float64 restatement trained on the same triples and the same noise (same start, 2
  layers, lr 0.05, reg 1e-3, cl_weight 0.5, eps 0.1, temperature 0.2, batch 256, 5 epochs, seed 0).  Measured on
  the CPU, the f32-numpy restatement beside the float64 one over the seeds 0, 1, 2 (start and draws): AUC 0.914135
  / 0.914135, 0.890692 / 0.890692, 0.952296 / 0.952296 -- gaps 0, 0, 0 (the final tables differ by 5e-7 at most
  and no pair of scores changes order; the untrained starts are at 0.823, 0.815, 0.813).  Ten times the largest
  gap measured is therefore 0, the margin of tests/test_lightgcn.py: the held-out AUC has to equal the
  restatement's."""
  tr, ho, start, _, hist, tables = planted_fit
  P64, Q64, _, hist64 = sg.fit(tr, *start, 2, 5, 256, LR, REG, W, EPS, TAU, seed=0)
  zero = np.zeros(120)
  want, got = bpr_util.auc(P64, Q64, zero, tr, ho), bpr_util.auc(tables[0], tables[1], tables[2], tr, ho)
  print("held-out AUC: kernels %.6f, float64 restatement %.6f; max table difference %.3g; history %s beside %s"
        % (got, want, np.abs(tables[0] - P64).max(), hist, hist64))
  assert want > 0.7
  assert abs(got - want) <= 10 * 0.0


def test_the_fitted_tables_plug_into_the_rest(planted_fit, tmp_path):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.metrics import Recall
  tr, ho, _, rec, _, tables = planted_fit
  assert not tables[2].any()                                                   # (the bias is all zeros)
  users = np.arange(50)
  inp = UsersInteractions(users, tr[users])
  lists = rec.recommend(inp, 10)
  assert len(lists) == 50 and all(len(l) == 10 for l in lists)
  seen = tr[users].toarray() > 0
  assert not any(seen[u, l].any() for u, l in enumerate(lists)) and all(len(set(l)) == 10 for l in lists)
  res = rec.evaluate(RecommendationDataset(tr, ho), num_recommendations=20, metrics=[Recall(k=20, normalize=True)],
                     batch_size=100)
  assert np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)) > 20.0 / 120       # (better than chance)
  f = rec.save_state(str(tmp_path / "simgcl"))
  rec2 = _recoder()
  rec2.init_from_model_file(f)
  assert all(np.array_equal(a, b) for a, b in zip(tables, _tables(rec2)))
  assert np.array_equal(rec.recommend_array(inp, 10), rec2.recommend_array(inp, 10))
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
  rec.train(RecommendationDataset(tr), batch_size=100, lr=1e-3, num_epochs=1, negative_sampling=True)
  assert np.all(np.isfinite(rec.last_epoch_losses)) and len(rec.last_epoch_losses) == 2
  bpr_hist = rec.train_bpr(RecommendationDataset(tr), num_epochs=1)                       # (a warm start)
  assert len(bpr_hist) == 1 and np.isfinite(bpr_hist[0])
  als_hist = rec.train_als(RecommendationDataset(tr), num_iterations=1, reg=1.0)
  assert len(als_hist) == 1 and np.isfinite(als_hist[0])
