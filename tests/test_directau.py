"""GPU: rk_als_dau_grad of librecoder_als.so and recoder_amd/directau.py against the restatement of
tests/directau_util.py -- the loss and the gradient rows against float64 within a bound worked out from the
kernels' chains, one whole step, and Recoder.train_directau end to end with what the fitted tables plug into."""
import numpy as np
import pytest
import torch

from tests import bpr_util, directau_util as du, lightgcn_util as lg

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
f32 = lambda v: float(np.float32(v))                           # (f32 values: the kernels take floats)
LR, REG, GAMMA = f32(0.05), f32(1e-3), 1.0
N = 40                                                         # rows of either table in the kernel's cases


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, ld, fill=7.0):
  a = np.asarray(a, np.float32)
  full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  full[:, :a.shape[1]] = _t(a)
  return full, full[:, :a.shape[1]]


# ------------------------------------------------------------------ kernel
def _grad_gpu(users, items, X, Y, gamma=GAMMA, ld_pad=3):
  """((align, unif_users, unif_items), m, valid, DU, DI) after one rk_als_dau_grad; X with a padded leading
  dimension, every output filled with 7 first."""
  from recoder_amd import directau
  T, h = len(users), X.shape[1]
  Xfull, Xv = _padded(X, h + ld_pad)
  raw = torch.empty(directau.grad_workspace_bytes(T, h), dtype=torch.uint8, device=DEV)
  DU, DI = torch.full((T, h), 7.0, device=DEV), torch.full((T, h), 7.0, device=DEV)
  valid, loss = torch.full((T,), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
  count = torch.full((1,), 7, dtype=torch.int32, device=DEV)
  directau.grad(_t(users, np.int32), _t(items, np.int32), Xv, _t(Y), gamma, raw, DU, DI, valid, loss, count)
  assert bool((Xfull[:, h:] == 7.0).all()), "a padding column was written"
  return tuple(loss.cpu().tolist()), int(count.item()), valid.cpu().numpy(), DU.cpu().numpy(), DI.cpu().numpy()


def _case(T, h):
  """Slots over two 40-row tables.  From T = 65 on: slot 0 has the user -1 and slot 1 the item 40 (both invalid),
  users and items repeat (T > 40), and the user of slot 2 and the item of slot 3 have rows of norm 0."""
  rng = np.random.RandomState(T * 1000 + h)
  X, Y = rng.randn(N, h).astype(np.float32), rng.randn(N, h).astype(np.float32)
  if T <= 2:
    return np.array([3, 9][:T], np.int32), np.array([5, 11][:T], np.int32), X, Y, None, None
  users, items = rng.randint(0, N, T).astype(np.int32), rng.randint(0, N, T).astype(np.int32)
  users[0], items[1] = -1, N
  zu, zi = int(users[2]), int(items[3])
  X[zu], Y[zi] = 0, 0
  return users, items, X, Y, zu, zi


def _dau_bounds(users, items, X, Y, gamma):
  """First-order bounds ((align, unif_users, unif_items), BU, BI) of the f32 kernels against float64, u = 2^-24,
  every chain at its length.  z = v / |v| carries ez = (h + 3) u an element (h products under the root, the root,
  the division, the product).  A dot of two rows of |z| <= 1 carries es = (3 h + 7) u; the squared distance
  n_p + n_q - 2 s (n = 1 or 0 exactly; one fmaf, at most 4) carries ed = 2 es + 4 u; e = expf(-2 d) (the product by
  2 is exact, expf good to 1 ulp as HIP's table of device functions says) carries eE = 2 ed + 3 u relatively.
  A row sum r adds ceil(T / 64) terms a lane and six butterfly steps, all positive: er = eE + (ceil(T / 64) + 7) u;
  their sum S = 2 E adds ceil(T / 256) terms a thread and eight tree steps: eS = er + (ceil(T / 256) + 9) u;
  unif = logf(S / (m (m - 1))): eS + (3 + 2 |unif|) u absolutely.  An alignment term sums h squares of d = a - b
  (each 2 ez + 2 u off, |d| <= 2), their mean over the slots as S.  c1 = 4 gamma / S carries eS + 3 u, c2 = 2 / m
  one u.  The product sum_q e_pq z_q is a chain of T fmafs: sum_q e_pq (eE |z_q| + ez) + (T + 1) u sum_q e_pq |z_q|;
  minus r z and times c1, plus c2 (z - z'), each operation its own rounding; the normalisation's backward adds a
  dot of h products, as in tests/test_simgcl.py.  The whole is doubled for the terms of second order."""
  T, h, u = len(users), X.shape[1], U24
  ok = du.valid_slots(users, items, X.shape[0], Y.shape[0])
  m = int(ok.sum())
  BU, BI = np.zeros((T, h)), np.zeros((T, h))
  if m == 0:
    return (0.0, 0.0, 0.0), BU, BI
  (a, ia), (b, ib) = du.normalise(X[users[ok]].astype(np.float64)), du.normalise(Y[items[ok]].astype(np.float64))
  ez, es = (h + 3) * u, (3 * h + 7) * u
  eE = 2 * (2 * es + 4 * u) + 3 * u
  er = eE + (-(-T // 64) + 7) * u
  eS = er + (-(-T // 256) + 9) * u
  d = a - b
  term = (d * d).sum(1)
  e_term = 2 * np.abs(d).sum(1) * (2 * ez + 2 * u) + (-(-h // 64) + 8) * u * term
  e_align = e_term.sum() / m + (-(-T // 256) + 11) * u * term.sum() / m
  e_unif = []
  for z, B, inv, sign in ((a, BU, ia, 1.0), (b, BI, ib, -1.0)):
    if m >= 2:
      E = du.weights(z)
      r = E.sum(1)[:, None]
      S = r.sum()
      unif = np.log(S / (m * (m - 1.0)))
      c1 = 4 * gamma / S
      acc = E @ z
      e_acc = E @ (eE * np.abs(z) + ez) + (T + 1) * u * (E @ np.abs(z))
      un = acc - r * z
      e_un = e_acc + r * (er * np.abs(z) + ez) + u * np.abs(un)
      e_unif.append(eS + (3 + 2 * abs(unif)) * u)
    else:
      c1, un, e_un = 0.0, np.zeros_like(z), np.zeros_like(z)
      e_unif.append(0.0)
    c2 = 2.0 / m
    dz = c1 * un + sign * c2 * d
    e_dz = c1 * ((eS + 3 * u) * np.abs(un) + e_un) + c2 * (4 * u * np.abs(d) + 2 * ez) + u * np.abs(dz)
    dot = (z * dz).sum(1)[:, None]
    e_dot = (np.abs(z) * e_dz).sum(1)[:, None] + (2 * h + 3) * u * (np.abs(z) * np.abs(dz)).sum(1)[:, None]
    dv = (dz - z * dot) * inv
    B[ok] = 2 * (inv * (e_dz + np.abs(z) * e_dot + (h + 5) * u * (np.abs(dz) + np.abs(z * dot))) + (h + 6) * u * np.abs(dv))
  return (2 * e_align, 2 * e_unif[0], 2 * e_unif[1]), BU, BI


def _check(users, items, X, Y, gamma, label):
  want_l, want_m, want_valid, wDU, wDI = du.grad_rows(users, items, X, Y, gamma)
  got_l, m, valid, DU, DI = _grad_gpu(users, items, X, Y, gamma)
  bl, BU, BI = _dau_bounds(users, items, X, Y, gamma)
  ratios = [abs(g - w) / max(b, 1e-300) if (b > 0 or g != w) else 0.0 for g, w, b in zip(got_l, want_l, bl)] + \
      [(np.abs(G - W) / np.maximum(B, 1e-300))[(B > 0) | (G != W)].max(initial=0.0) for G, W, B in ((DU, wDU, BU), (DI, wDI, BI))]
  print("%s: m %d, losses %s (float64 %s), err / bound: align %.3f, unif users %.3f, unif items %.3f, DU %.3f, "
        "DI %.3f" % (label, m, np.round(got_l, 6), np.round(want_l, 6), *ratios))
  assert m == want_m and np.array_equal(valid, want_valid)
  assert all(abs(g - w) <= b for g, w, b in zip(got_l, want_l, bl))
  assert np.all(np.abs(DU - wDU) <= BU) and np.all(np.abs(DI - wDI) <= BI)
  assert not DU[valid == 0].any() and not DI[valid == 0].any()                 # (an invalid slot: zero rows)
  return got_l, m, valid, DU, DI


@pytest.mark.parametrize("h", [1, 4, 65, 200])
@pytest.mark.parametrize("T", [1, 2, 65, 300])
def test_grad_against_float64(T, h):
  users, items, X, Y, zu, zi = _case(T, h)
  ok = du.valid_slots(users, items, N, N)
  if T >= 65:
    assert not ok[0] and not ok[1] and ok.sum() == T - 2
    assert len(set(users[ok])) < ok.sum() and len(set(items[ok])) < ok.sum() and not X[zu].any() and not Y[zi].any()
  got = _check(users, items, X, Y, GAMMA, "T %d h %d" % (T, h))
  losses, m, valid, DU, DI = got
  if T == 1:                                                   # no pair: the alignment's gradient alone
    assert losses[1] == 0 and losses[2] == 0 and m == 1
    zero_gamma = _grad_gpu(users, items, X, Y, 0.0)
    assert np.array_equal(DU, zero_gamma[3]) and np.array_equal(DI, zero_gamma[4])
    assert h == 1 or (DU.any() and DI.any())
  else:
    assert losses[0] > 0 and losses[1] <= 0 and losses[2] <= 0
  if T >= 65:                                                  # |v| = 0: z = 0 and no gradient on its own side
    su, si = users == zu, items == zi
    assert not DU[su].any() and not DI[si].any()
    if h > 1:
      assert DI[su & ok & ~si].any(1).all() and DU[si & ok & ~su].any(1).all()
  again = _grad_gpu(users, items, X, Y)
  assert again[:2] == (losses, m) and all(np.array_equal(a, b) for a, b in zip(again[2:], got[2:])), "not repeatable"


@pytest.mark.parametrize("h", [4, 65])
def test_a_batch_of_one_pair_has_no_uniformity(h):
  rng = np.random.RandomState(h)
  X, Y = rng.randn(N, h).astype(np.float32), rng.randn(N, h).astype(np.float32)
  users, items = np.full(65, 3, np.int32), np.full(65, 5, np.int32)
  losses, m, _, DU, DI = _check(users, items, X, Y, 5.0, "one pair, h %d" % h)     # (float64: unif = 0 to 1e-15)
  assert m == 65
  # the uniformity's gradient vanishes: what is left is the alignment's, within the same bound
  _, BU, BI = _dau_bounds(users, items, X, Y, 5.0)
  _, _, _, AU, AI = _grad_gpu(users, items, X, Y, 0.0)
  assert np.all(np.abs(DU - AU) <= BU) and np.all(np.abs(DI - AI) <= BI)
  allbad = _grad_gpu(np.array([-1, N, 3], np.int32), np.array([2, 2, N], np.int32), X, Y)
  assert allbad[0] == (0.0, 0.0, 0.0) and allbad[1] == 0 and not allbad[2].any() and not allbad[3].any() \
      and not allbad[4].any()


# ---------------------------------------------------------------- one step
def _graph(tr):
  from recoder_amd import als, lightgcn
  return lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))


@pytest.mark.parametrize("K", [2, 0])
def test_one_full_step_against_the_restatement_on_the_same_draws(K):
  from recoder_amd import directau
  tr, _ = bpr_util.planted()
  h, T = 24, 256
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = _graph(tr)
  state = directau.new_state(X, Y, K)
  ws = directau.Workspace(200, 120, T, h, DEV)
  directau.step(X, Y, graph, state, ws, 11, 3, LR, REG, GAMMA)
  users, pos = ws.bpr.users.cpu().numpy(), ws.bpr.pos.cpu().numpy()
  wu, wp, _ = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and state["step"] == 1
  assert int(ws.valid_count.item()) == T and bool((ws.bpr.g == 1).all())
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  l64, _ = du.step(tr, s64, K, users, pos, LR, REG, GAMMA)
  l32, _ = du.step(tr, s32, K, users, pos, LR, REG, GAMMA, np.float32)
  print("K %d: losses: kernels %s, f32 restatement %s, float64 %s" % (K, ws.loss.cpu().tolist(), l32, l64))
  counts = [np.bincount(users, minlength=200), np.bincount(pos, minlength=120)]
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      dist = np.abs(s32[key][side] - s64[key][side]).max()
      err = np.abs(state[key][side].cpu().numpy() - s64[key][side]).max()
      print("step %s[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (key, side, dist, err))
      assert dist > 0 and err <= 4 * dist, (key, side)
  for side in (0, 1):
    assert np.array_equal(ws.count[side].cpu().numpy(), counts[side])


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
  """train_directau on the planted matrix from the base tables ``start`` (set after an empty fit has built the
  model); more than one entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder()
  ds = RecommendationDataset(tr)
  kw = dict(num_layers=2, batch_size=256, lr=LR, reg=REG, gamma=GAMMA, seed=seed)
  assert rec.train_directau(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  hist = []
  for k, n in enumerate(epochs):
    hist += rec.train_directau(ds, num_epochs=n, resume=k > 0, **kw)
  return rec, hist, _tables(rec)


@pytest.fixture(scope="module")
def planted_fit():
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)[:2]
  rec, hist, tables = _train(tr, 0, start)
  return tr, ho, start, rec, hist, tables


def test_train_directau_lowers_the_alignment_repeats_and_resumes_bit_for_bit(planted_fit):
  tr, _, start, rec, hist, tables = planted_fit
  assert len(hist) == 5 and rec.directau_history == hist and np.all(np.isfinite(hist))
  assert all(len(e) == 3 and e[0] < hist[0][0] for e in hist[1:]), hist
  st = rec.directau_state
  assert st["num_layers"] == 2 and st["step"] == 5 * -(-tr.nnz // 256) and st["E0"][0].is_cuda
  assert rec.lightgcn_state is None and rec.simgcl_state is None
  assert rec.lightgcn_history == [] and rec.simgcl_history == []
  _, hist2, again = _train(tr, 0, start)
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist
  _, _, other = _train(tr, 1, start)
  assert not np.array_equal(tables[0], other[0]) and not np.array_equal(tables[1], other[1])
  rec3, hist3, resumed = _train(tr, 0, start, epochs=(2, 3))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist
  from recoder_amd.data import RecommendationDataset
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 0\\)"):
    rec3.train_directau(RecommendationDataset(tr), num_layers=0, num_epochs=1, resume=True)
  assert all(np.array_equal(a, b) for a, b in zip(resumed, _tables(rec3)))


def test_held_out_auc_beside_the_float64_restatement(planted_fit):
  """The yardstick is the float64 restatement trained on the same draws (same start, 2 layers, lr 0.05, reg 1e-3,
  gamma 1, batch 256, 5 epochs, seed 0).  Measured on the CPU, the f32-numpy restatement beside the float64 one
  over the seeds 0, 1, 2 (start and draws): AUC 0.859906 / 0.859906, 0.849733 / 0.849733, 0.866006 / 0.866006 --
  gaps 0, 0, 0 (the final tables differ by 5.1e-7, 2.1e-6 and 1.1e-4 at most and no pair of scores changes order;
  the untrained starts are at 0.508, 0.521, 0.499; profiles/directau_quality.jsonl keeps the three records).  Ten
  times the largest gap measured is therefore 0, the margin of tests/test_lightgcn.py and tests/test_simgcl.py:
  the held-out AUC has to equal the restatement's."""
  tr, ho, start, _, hist, tables = planted_fit
  P64, Q64, _, hist64 = du.fit(tr, *start, 2, 5, 256, LR, REG, GAMMA, seed=0)
  zero = np.zeros(120)
  want, got = bpr_util.auc(P64, Q64, zero, tr, ho), bpr_util.auc(tables[0], tables[1], tables[2], tr, ho)
  untrained = bpr_util.auc(start[0], start[1], zero, tr, ho)
  print("held-out AUC: kernels %.6f, float64 restatement %.6f, untrained %.6f; max table difference %.3g; history "
        "%s beside %s" % (got, want, untrained, np.abs(tables[0] - P64).max(), hist, hist64))
  assert want > untrained
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
  f = rec.save_state(str(tmp_path / "directau"))
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
