"""GPU: the LightGCN kernels (rk_als_lgcn_* of librecoder_als.so) and recoder_amd/lightgcn.py against the
restatement of tests/lightgcn_util.py -- the propagation against float64 within the rounding of its own f32 chain,
its adjointness, the scatter and the Adam pass, one whole step, and Recoder.train_lightgcn end to end with what
the fitted tables plug into."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util, lightgcn_util as lg

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
LR, REG = float(np.float32(0.05)), float(np.float32(1e-3))     # (f32 values: the kernels take floats)


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


def _prop_bound(m, rs, cs, F, acc=None, acc_scale=1.0):
  """(L + 3) 2^-24 (rs sum |cs F| (+ |acc|)) |acc_scale| per element: an fmaf chain over the row's L products,
  then three more roundings."""
  mag, _ = lg.propagate(m, rs, cs, np.abs(F))
  if acc is not None:
    mag = mag + np.abs(np.asarray(acc, np.float64))
  return (np.diff(m.indptr)[:, None] + 3) * U24 * mag * abs(acc_scale)


def _propagate_gpu(csr, rs, cs, F, ld_pad, out=True, acc=None, acc_scale=1.0, row_lo=0, row_hi=None):
  """(Out, Acc) as numpy (with their padding columns, which must stay 7) after one call."""
  from recoder_amd import lightgcn
  h = F.shape[1]
  Ffull, Fv = _padded(F, h + ld_pad)
  rows = csr.shape[0]
  Ofull, Ov = _padded(np.full((rows, h), 7.0), h + ld_pad) if out else (None, None)
  Afull, Av = _padded(acc, h + ld_pad) if acc is not None else (None, None)
  lightgcn.propagate(csr, _t(rs), _t(cs), Fv, Ov, Av, acc_scale, row_lo, row_hi)
  for full in (Ofull, Afull):
    assert full is None or bool((full[:, h:] == 7.0).all()), "a padding column was written"
  return (Ov.cpu().numpy() if out else None), (Av.cpu().numpy() if acc is not None else None)


@pytest.mark.parametrize("h", [1, 4, 64, 65, 200, 300])      # (300: two float4s, or five floats, per lane)
def test_propagate_against_float64(h):
  worst = 0.0
  for name in ("hand", "handT", "long", "longT"):
    m, rs, cs = _oriented(name)
    csr = _csr(m)
    rng = np.random.RandomState(h + len(name))
    F = rng.randn(m.shape[1], h).astype(np.float32)
    acc0 = rng.randn(m.shape[0], h).astype(np.float32)
    want, _ = lg.propagate(m, rs, cs, F)
    empty = np.diff(m.indptr) == 0
    assert empty.any() or name == "longT"
    outs = []
    for ld_pad in (0, 3):
      out, _ = _propagate_gpu(csr, rs, cs, F, ld_pad)
      bound = _prop_bound(m, rs, cs, F)
      err = np.abs(out - want)
      worst = max(worst, (err / np.maximum(2 * bound, 1e-300)).max())
      assert np.all(err <= 2 * bound), (name, ld_pad)
      assert not out[empty].any() and not np.signbit(out[empty]).any()
      again, _ = _propagate_gpu(csr, rs, cs, F, ld_pad)
      assert np.array_equal(out, again), "not bitwise repeatable"
      outs.append(out)
      for scale, with_out in ((1.0, True), (0.25, True), (0.25, False)):
        o2, acc = _propagate_gpu(csr, rs, cs, F, ld_pad, out=with_out, acc=acc0, acc_scale=scale)
        assert o2 is None or np.array_equal(o2, out)
        wacc = (acc0.astype(np.float64) + want) * scale
        bacc = _prop_bound(m, rs, cs, F, acc0, scale)
        worst = max(worst, (np.abs(acc - wacc) / np.maximum(2 * bacc, 1e-300)).max())
        assert np.all(np.abs(acc - wacc) <= 2 * bacc), (name, ld_pad, scale, with_out)
        # the accumulate is two more f32 operations on the rounded Out, exactly
        assert np.array_equal(acc, (acc0 + out) * np.float32(scale))
      lo, hi = 3, min(11, m.shape[0])
      part, _ = _propagate_gpu(csr, rs, cs, F, ld_pad, row_lo=lo, row_hi=hi)
      assert np.array_equal(part[lo:hi], out[lo:hi]) and np.all(part[:lo] == 7.0) and np.all(part[hi:] == 7.0)
    assert np.array_equal(outs[0], outs[1]), "the leading dimension (16-byte accesses or not) changed the bits"
  print("h %d: largest err / (2 x bound) %.3f" % (h, worst))


def test_the_two_orientations_are_adjoint():
  h = 64
  m, su, si = _oriented("hand")
  mt = lg.transpose(m)
  rng = np.random.RandomState(5)
  x, y = rng.randn(23, h).astype(np.float32), rng.randn(37, h).astype(np.float32)
  Ax, _ = _propagate_gpu(_csr(m), su, si, x, 0)
  Aty, _ = _propagate_gpu(_csr(mt), si, su, y, 0)
  lhs = float((Ax.astype(np.float64) * y).sum())
  rhs = float((x.astype(np.float64) * Aty).sum())
  bound = float((_prop_bound(m, su, si, x) * np.abs(y)).sum() + (_prop_bound(mt, si, su, y) * np.abs(x)).sum())
  print("<Ax, y> %.9g, <x, A^T y> %.9g, difference / (2 x bound) %.3f" % (lhs, rhs, abs(lhs - rhs) / (2 * bound)))
  assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 2 * bound


# ------------------------------------------------------------------ scatter
def _triples(n_users, n_items, T):
  if T == 7:
    return (np.array([0, 1, 0, 2, 0, 1, 0], np.int32), np.array([0, 1, 2, 3, 1, 4, 0], np.int32),
            np.array([1, 0, -1, 4, 2, 3, 3], np.int32))
  rng = np.random.RandomState(T)
  users = rng.randint(0, n_users // 2, T).astype(np.int32)          # (the upper half of the users: not in the batch)
  users[10:100] = 3                                                  # one user in 90 triples
  pos = rng.randint(0, n_items - 10, T).astype(np.int32)
  neg = ((pos + 1 + rng.randint(0, n_items - 11, T)) % (n_items - 10)).astype(np.int32)
  neg[rng.rand(T) < 0.1] = -1
  return users, pos, neg


@pytest.mark.parametrize("h", [1, 65, 300])
@pytest.mark.parametrize("shape", [(3, 5, 7), (200, 120, 256)])
def test_scatter_against_float64(shape, h):
  from recoder_amd import bpr, lightgcn
  n_users, n_items, T = shape
  users, pos, neg = _triples(*shape)
  ok = neg >= 0
  assert (~ok).any() and set(pos[ok]) & set(neg[ok]) and (T == 7 or np.bincount(users[ok]).max() >= 64)
  rng = np.random.RandomState(h)
  g = rng.rand(T).astype(np.float32)
  D, P = rng.randn(T, h).astype(np.float32), rng.randn(T, h).astype(np.float32)
  scale = float(np.float32(1.0 / T))
  (uk, uo), (ik, io) = bpr.sorted_keys(_t(users, np.int32), _t(pos, np.int32), _t(neg, np.int32), n_users, n_items)

  def run():
    Gu, Gi = torch.zeros((n_users, h), device=DEV), torch.zeros((n_items, h), device=DEV)
    cu, ci = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (n_users, n_items))
    lightgcn.scatter(uk, uo, 1, _t(g), _t(D), scale, Gu, cu)
    lightgcn.scatter(ik, io, 2, _t(g), _t(P), scale, Gi, ci)
    return [v.cpu().numpy() for v in (Gu, Gi, cu, ci)]
  Gu, Gi, cu, ci = run()
  wGu, wGi, wcu, wci = (np.asarray(a) for a in lg.scatter(users, pos, neg, g, D, P, n_users, n_items))
  wGu, wGi = wGu * T * np.float64(scale), wGi * T * np.float64(scale)           # (the f32 scale the kernel was given)
  assert np.array_equal(cu, wcu) and np.array_equal(ci, wci) and cu.dtype == np.int32
  # c 2^-24 sum |g V| scale, doubled
  mu, mi, _, _ = lg.scatter(users, pos, np.where(ok, neg, -1), g, -np.abs(D), -np.abs(P), n_users, n_items)
  mi = np.zeros_like(mi)
  np.add.at(mi, pos[ok], g[ok, None].astype(np.float64) * np.abs(P[ok]) / T)
  np.add.at(mi, neg[ok], g[ok, None].astype(np.float64) * np.abs(P[ok]) / T)
  for name, got, want, c, mag in (("users", Gu, wGu, wcu, mu), ("items", Gi, wGi, wci, mi)):
    bound = 2 * c[:, None] * U24 * mag
    err = np.abs(got - want)
    print("%s h %d %s: max err / bound %.3f" % (shape, h, name, (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), name
    assert not got[c == 0].any() and got[c > 0].any()
  assert T == 7 or ((wcu == 0).any() and (wci == 0).any())
  assert all(np.array_equal(a, b) for a, b in zip((Gu, Gi, cu, ci), run())), "not bitwise repeatable"


# --------------------------------------------------------------------- adam
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_against_the_restatement(t):
  from recoder_amd import lightgcn
  rows, h, ld = 50, 65, 68
  rng = np.random.RandomState(t)
  E, H = (0.3 * rng.randn(rows, h)).astype(np.float32), (0.01 * rng.randn(rows, h)).astype(np.float32)
  count = rng.randint(0, 41, rows).astype(np.int32)
  count[:5] = 0
  count[7] = 40
  H[:3] = 0                                                    # rows 0..2: a zero gradient and a zero count
  first = t == 1
  M = np.zeros((rows, h), np.float32) if first else (0.01 * rng.randn(rows, h)).astype(np.float32)
  V = np.zeros((rows, h), np.float32) if first else (1e-4 * rng.rand(rows, h)).astype(np.float32)
  rs = float(np.float32(REG / 256))
  want = lg.adam(E, H, count, rs, M, V, LR, t)
  f32 = lg.adam(E, H, count, rs, M, V, LR, t, np.float32)
  Efull, Ev = _padded(E, ld)
  Hfull, Hv = _padded(H, ld)
  Mt, Vt = _t(M), _t(V)
  lightgcn.adam(Ev, Hv, _t(count, np.int32), rs, Mt, Vt, LR, t)
  assert bool((Efull[:, h:] == 7.0).all()) and bool((Hfull[:, h:] == 7.0).all()) and np.array_equal(Hv.cpu().numpy(), H)
  for name, got, w, r in zip(("E0", "M", "V"), (Ev, Mt, Vt), want, f32):
    tol = 4 * np.abs(r - w).max()
    err = np.abs(got.cpu().numpy() - w).max()
    print("t %d %s: f32 restatement - float64 %.3g, kernel - float64 %.3g" % (t, name, tol / 4, err))
    assert tol > 0 and err <= tol, name
  if first:
    assert np.array_equal(Ev[:3].cpu().numpy(), E[:3])
  else:                                                        # a zero gradient still decays the moments
    assert np.array_equal(Mt[:3].cpu().numpy(), np.float32(0.9) * M[:3])


# ---------------------------------------------------------------- one step
def _graph(tr):
  from recoder_amd import als, lightgcn
  return lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))


def _final_bound(tr, Eu, Ei, K):
  """The bound of the propagate test composed over K layers: every term of an element's expansion passes at
  most K chains of at most Lmax products with three more roundings each, then the K + 1 roundings of the layer
  sum and the rounding of 1 / (K + 1); the operator is non-negative, so the final tables of |E0| bound the sum
  of the terms' magnitudes."""
  Lmax = max(np.diff(tr.indptr).max(), np.diff(lg.transpose(tr).indptr).max())
  aP, aQ = lg.forward(tr, np.abs(Eu), np.abs(Ei), K)
  f = (K * (Lmax + 3) + K + 2) * U24
  return f * aP, f * aQ


def test_one_full_step_against_the_restatement_on_the_same_triples():
  from recoder_amd import lightgcn
  tr, _ = bpr_util.planted()
  h, K, T = 24, 2, 256
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = _graph(tr)
  state = lightgcn.new_state(X, Y, K)
  ws = lightgcn.Workspace(200, 120, T, h, DEV)
  lightgcn.step(X, Y, graph, state, ws, 11, 3, LR, REG)
  users, pos, neg = (v.cpu().numpy() for v in (ws.bpr.users, ws.bpr.pos, ws.bpr.neg))
  wu, wp, wn = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and np.array_equal(neg, wn)
  assert state["step"] == 1
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  lg.step(tr, s64, K, users, pos, neg, LR, REG)
  lg.step(tr, s32, K, users, pos, neg, LR, REG, np.float32)
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      dist = np.abs(s32[key][side] - s64[key][side]).max()
      err = np.abs(state[key][side].cpu().numpy() - s64[key][side]).max()
      print("step %s[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (key, side, dist, err))
      assert dist > 0 and err <= 4 * dist, (key, side)
  # X, Y hold the final tables of the START of the step; those of the new base tables:
  lightgcn.forward(graph, state["E0"], K, ws.layers, (X, Y))
  nu, ni = (e.cpu().numpy() for e in state["E0"])
  wP, wQ = lg.forward(tr, nu, ni, K)
  for name, got, want, bound in zip("PQ", (X, Y), (wP, wQ), _final_bound(tr, nu, ni, K)):
    err = np.abs(got.cpu().numpy() - want)
    print("final %s: max err / (2 x bound) %.3f" % (name, (err / np.maximum(2 * bound, 1e-300)).max()))
    assert np.all(err <= 2 * bound), name


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
  """train_lightgcn on the planted matrix from the base tables ``start`` (set after an empty fit has built the
  model); more than one entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder()
  ds = RecommendationDataset(tr)
  kw = dict(num_layers=2, batch_size=256, lr=LR, reg=REG, seed=seed)
  assert rec.train_lightgcn(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  hist = []
  for k, n in enumerate(epochs):
    hist += rec.train_lightgcn(ds, num_epochs=n, resume=k > 0, **kw)
  return rec, hist, _tables(rec)


@pytest.fixture(scope="module")
def planted_fit():
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)[:2]
  rec, hist, tables = _train(tr, 0, start)
  return tr, ho, start, rec, hist, tables


def test_train_lightgcn_lowers_the_loss_repeats_and_resumes_bit_for_bit(planted_fit):
  tr, _, start, rec, hist, tables = planted_fit
  assert len(hist) == 5 and rec.lightgcn_history == hist and all(np.isfinite(hist))
  assert all(v < hist[0] for v in hist[1:]), hist
  st = rec.lightgcn_state
  assert st["num_layers"] == 2 and st["step"] == 5 * -(-tr.nnz // 256) and st["E0"][0].is_cuda
  _, hist2, again = _train(tr, 0, start)
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist
  _, _, other = _train(tr, 1, start)
  assert not np.array_equal(tables[0], other[0]) and not np.array_equal(tables[1], other[1])
  rec3, hist3, resumed = _train(tr, 0, start, epochs=(2, 3))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist
  from recoder_amd.data import RecommendationDataset
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 3\\)"):
    rec3.train_lightgcn(RecommendationDataset(tr), num_layers=3, num_epochs=1, resume=True)
  assert all(np.array_equal(a, b) for a, b in zip(resumed, _tables(rec3)))


def test_held_out_auc_beside_the_float64_restatement(planted_fit):
  """The yardstick is the float64 restatement trained on the same triples (same start, 2 layers, lr 0.05, reg
  1e-3, batch 256, 5 epochs, seed 0).  Measured on the CPU, the f32-numpy restatement beside the float64 one over
  the seeds 0, 1, 2 (start and draws): AUC 0.970267 / 0.970267, 0.973019 / 0.973019, 0.971588 / 0.971588 -- gaps
  0, 0, 0 (the final tables differ by 5e-6 at most and no pair of scores changes order; the untrained starts
  are at 0.542, 0.556, 0.517).  Ten times the largest gap measured is therefore 0: the held-out AUC has to
  equal the restatement's."""
  tr, ho, start, _, hist, tables = planted_fit
  P64, Q64, _, hist64 = lg.fit(tr, *start, 2, 5, 256, LR, REG, seed=0)
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
  S = tables[0][:50].astype(np.float64) @ tables[1].astype(np.float64).T
  seen = tr[users].toarray() > 0
  S[seen] = -np.inf
  assert not any(seen[u, l].any() for u, l in enumerate(lists)) and all(len(set(l)) == 10 for l in lists)
  assert np.mean([len(set(l) & set(np.argsort(-S[u])[:10])) for u, l in enumerate(lists)]) >= 8
  res = rec.evaluate(RecommendationDataset(tr, ho), num_recommendations=20, metrics=[Recall(k=20, normalize=True)],
                     batch_size=100)
  assert np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)) > 20.0 / 120       # (better than chance)
  f = rec.save_state(str(tmp_path / "lightgcn"))
  rec2 = _recoder()
  rec2.init_from_model_file(f)
  assert np.array_equal(rec.recommend_array(inp, 10), rec2.recommend_array(inp, 10))
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
  rec.train(RecommendationDataset(tr), batch_size=100, lr=1e-3, num_epochs=1, negative_sampling=True)
  assert np.all(np.isfinite(rec.last_epoch_losses)) and len(rec.last_epoch_losses) == 2
  als_hist = rec.train_als(RecommendationDataset(tr), num_iterations=1, reg=1.0)          # (a warm start)
  assert len(als_hist) == 1 and np.isfinite(als_hist[0])
