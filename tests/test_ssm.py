"""GPU: rk_als_ssm_grad of librecoder_als.so and recoder_amd/ssm.py against the restatement of tests/ssm_util.py --
the losses and the gradient rows against float64 within a bound worked out from the kernels' chains, one whole step,
and Recoder.train_ssm end to end with what the fitted tables plug into."""
import numpy as np
import pytest
import torch

from tests import bpr_util, lightgcn_util as lg, ssm_util as su

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24
TINY = 2.0 ** -126                                             # (an f32 below it may be flushed to 0)
f32 = lambda v: float(np.float32(v))                           # (f32 values: the kernels take floats)
LR, REG, TAU = f32(0.05), f32(1e-3), f32(0.2)
N = 40                                                         # rows of either table in the kernel's cases
SEED, STEP = 5, 9


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, ld, fill=7.0):
  a = np.asarray(a, np.float32)
  full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  full[:, :a.shape[1]] = _t(a)
  return full, full[:, :a.shape[1]]


# ------------------------------------------------------------------ kernel
def _grad_gpu(users, items, S, X, Y, temperature=TAU, similarity="cosine", corr=None, ld_pad=3):
  """((loss, probability), m, valid, cvalid, cand, DU, DC) after one rk_als_ssm_grad; X with a padded leading
  dimension, every output filled with 7 first."""
  from recoder_amd import ssm
  T, h = len(users), X.shape[1]
  C = T + S
  Xfull, Xv = _padded(X, h + ld_pad)
  raw = torch.empty(ssm.grad_workspace_bytes(T, S, h), dtype=torch.uint8, device=DEV)
  DU, DC = torch.full((T, h), 7.0, device=DEV), torch.full((C, h), 7.0, device=DEV)
  valid, cvalid, loss = torch.full((T,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV)
  count, cand = torch.full((1,), 7, dtype=torch.int32, device=DEV), torch.full((C,), 7, dtype=torch.int32, device=DEV)
  ssm.grad(_t(users, np.int32), _t(items, np.int32), S, SEED, STEP, Xv, _t(Y), temperature, similarity,
           None if corr is None else _t(corr), raw, cand, DU, DC, valid, cvalid, loss, count)
  assert bool((Xfull[:, h:] == 7.0).all()), "a padding column was written"
  return (tuple(loss.cpu().tolist()), int(count.item()), valid.cpu().numpy(), cvalid.cpu().numpy(), cand.cpu().numpy(),
          DU.cpu().numpy(), DC.cpu().numpy())


def _case(T, h, scale=1.0):
  """Slots over two 40-row tables.  From T = 65 on: slot 0 has the user -1 and slot 1 the item 40 (both invalid),
  users and items repeat (T > 40: some column holds a row's positive once more), and the user of slot 2 and the
  item of slot 3 have rows of norm 0."""
  rng = np.random.RandomState(T * 1000 + h)
  X, Y = (scale * rng.randn(N, h)).astype(np.float32), (scale * rng.randn(N, h)).astype(np.float32)
  if T <= 2:
    return np.array([3, 9][:T], np.int32), np.array([5, 11][:T], np.int32), X, Y, None, None
  users, items = rng.randint(0, N, T).astype(np.int32), rng.randint(0, N, T).astype(np.int32)
  users[0], items[1] = -1, N
  zu, zi = int(users[2]), int(items[3])
  X[zu], Y[zi] = 0, 0
  return users, items, X, Y, zu, zi


def _ssm_bounds(users, items, cand, X, Y, temperature, cosine, corr):
  """First-order bounds ((loss, probability), BU, BC) of the f32 kernels against float64, u = 2^-24, every chain at
  its length; a dot of length k carries k u of the sum of its terms' magnitudes, in any order.  z = v / |v| carries
  ez = (h + 3) u of |z| an element (h products under the root, the root, the division, the product; 0 for the dot
  product, whose rows are the tables' own).  A score carries es = (2 ez + h u) sum_k |zu_k zc_k| / tau and the one
  rounding of its fmaf, u |s|.  e = expf(s - max) carries, relatively, es, the subtraction's u |s - max| and expf's
  2 u (1 ulp, as HIP's table of device functions says); the maximum cancels between e and its sum.  The sum adds
  ceil(C / 64) terms a lane and six butterfly steps, all positive, and carries the p-weighted mean R of its terms'
  errors; p = e / sum one more rounding; an f32 below 2^-126 may be flushed.  W = (p - [c == t]) / m adds two
  roundings.  lse = max + logf(sum): the weighted means of es and of the terms' errors, the sum's chain, logf's
  2 u |log sum| and the addition's u |lse|; the loss term adds es of the diagonal and its own rounding, the
  probability expf's; their means over the slots ceil(T / 256) terms a thread and eight tree steps, and the division.
  The products W Zc and W^T Zu are chains of C and T terms on the stored W; times 1 / tau one rounding; the
  normalisation's backward adds a dot of h products, as in tests/test_directau.py.  The whole is doubled for the terms
  of second order."""
  T, C, h, u = len(users), len(cand), X.shape[1], U24
  ok, cvalid, live = su.live_mask(users, items, cand, X.shape[0], Y.shape[0])
  m = int(ok.sum())
  BU, BC = np.zeros((T, h)), np.zeros((C, h))
  if m == 0:
    return (0.0, 0.0), BU, BC
  A, B = np.zeros((T, h)), np.zeros((C, h))
  A[ok], B[cvalid] = X[users[ok]], Y[cand[cvalid]]
  if cosine:
    (zu, iu), (zc, ic), ez = su.normalise(A), su.normalise(B), (h + 3) * u
  else:
    zu, zc, iu, ic, ez = A, B, np.ones((T, 1)), np.ones((C, 1)), 0.0
  it = su.inverse_temperature(temperature)
  cc = np.zeros(C)
  if corr is not None:
    cc[cvalid] = np.asarray(corr, np.float64)[cand[cvalid]]
  s = (zu @ zc.T) * it - cc[None, :]
  es = (2 * ez + h * u) * (np.abs(zu) @ np.abs(zc).T) * it + u * np.abs(s)
  rows = np.nonzero(ok)[0]
  sl = np.where(live, s, -np.inf)[rows]
  lv = live[rows]
  esl = np.where(lv, es[rows], 0.0)
  mx = sl.max(1, keepdims=True)
  d = np.where(lv, sl - mx, 0.0)
  e = np.where(lv, np.exp(sl - mx), 0.0)
  tot = e.sum(1, keepdims=True)
  p = e / tot
  chain = (-(-C // 64) + 6) * u
  r = np.where(lv, esl + u * np.abs(d) + 2 * u, 0.0)
  R = (p * r).sum(1, keepdims=True)
  ep = p * (r + R + chain + 2 * u) + TINY * lv
  diag = np.zeros_like(p)
  diag[np.arange(len(rows)), rows] = 1
  W, eW = np.zeros((T, C)), np.zeros((T, C))
  W[rows] = (p - diag) / m
  eW[rows] = (ep + u * np.abs(p - diag)) / m + u * np.abs(W[rows])
  lse = mx[:, 0] + np.log(tot[:, 0])
  e_lse = R[:, 0] + chain + 2 * u * np.abs(np.log(tot[:, 0])) + u * np.abs(lse)
  stt, estt = sl[np.arange(len(rows)), rows], esl[np.arange(len(rows)), rows]
  term, prob = lse - stt, np.exp(stt - lse)
  e_term = e_lse + estt + u * np.abs(term)
  e_prob = prob * (e_lse + estt + u * np.abs(term) + 2 * u) + TINY
  tree = (-(-T // 256) + 10) * u
  b_loss = e_term.sum() / m + tree * np.abs(term).sum() / m
  b_prob = e_prob.sum() / m + tree * prob.sum() / m
  for Wm, eWm, zo, z, inv, Bd, k in ((W, eW, zc, zu, iu, BU, C), (W.T, eW.T, zu, zc, ic, BC, T)):
    acc = Wm @ zo
    e_acc = eWm @ np.abs(zo) + (ez + k * u) * (np.abs(Wm) @ np.abs(zo))
    dz = acc * it
    e_dz = it * e_acc + u * np.abs(dz)
    if cosine:
      dot = (z * dz).sum(1)[:, None]
      e_dot = (np.abs(z) * e_dz).sum(1)[:, None] + (2 * h + 3) * u * (np.abs(z) * np.abs(dz)).sum(1)[:, None]
      dv = (dz - z * dot) * inv
      Bd[:] = 2 * (inv * (e_dz + np.abs(z) * e_dot + (h + 5) * u * (np.abs(dz) + np.abs(z * dot))) + (h + 6) * u * np.abs(dv))
    else:
      Bd[:] = 2 * e_dz
  return (2 * b_loss, 2 * b_prob), BU, BC


def _check(users, items, S, X, Y, temperature, similarity, corr, label):
  cosine = similarity == "cosine"
  cand = su.candidates(items, SEED, STEP, S, Y.shape[0])
  want_l, want_m, want_valid, want_cvalid, wDU, wDC = su.grad_rows(users, items, cand, X, Y, temperature, cosine, corr)
  got = _grad_gpu(users, items, S, X, Y, temperature, similarity, corr)
  got_l, m, valid, cvalid, gcand, DU, DC = got
  bl, BU, BC = _ssm_bounds(users, items, cand, X, Y, temperature, cosine, corr)
  ratios = [abs(g - w) / max(b, 1e-300) if (b > 0 or g != w) else 0.0 for g, w, b in zip(got_l, want_l, bl)] + \
      [(np.abs(G - Wt) / np.maximum(B, 1e-300))[(B > 0) | (G != Wt)].max(initial=0.0) for G, Wt, B in ((DU, wDU, BU), (DC, wDC, BC))]
  print("%s: m %d, losses %s (float64 %s), err / bound: loss %.3f, probability %.3f, DU %.3f, DC %.3f"
        % (label, m, np.round(got_l, 6), np.round(want_l, 6), *ratios))
  assert np.array_equal(gcand, cand), "the candidate columns are not the restatement's draws"
  assert m == want_m and np.array_equal(valid, want_valid) and np.array_equal(cvalid, want_cvalid)
  assert all(abs(g - w) <= b for g, w, b in zip(got_l, want_l, bl))
  assert np.all(np.abs(DU - wDU) <= BU) and np.all(np.abs(DC - wDC) <= BC)
  assert not DU[valid == 0].any() and not DC[cvalid == 0].any()                # (an invalid slot or column: zero rows)
  return got


@pytest.mark.parametrize("h", [1, 4, 65, 200])
@pytest.mark.parametrize("S", [0, 1, 70])
@pytest.mark.parametrize("T", [1, 2, 65, 300])
def test_grad_against_float64(T, S, h):
  users, items, X, Y, zu, zi = _case(T, h)
  ok, _, live = su.live_mask(users, items, su.candidates(items, SEED, STEP, S, N), N, N)
  if T >= 65:
    assert not ok[0] and not ok[1] and ok.sum() == T - 2
    assert len(set(users[ok])) < ok.sum() and not X[zu].any() and not Y[zi].any()
    assert (~live[ok][:, np.concatenate([ok, np.ones(S, bool)])]).any()        # (an excluded duplicate-item column)
  corr = su.correction(bpr_util.planted(N, N)[0], T, S, 1.0) if h == 4 else None   # (with the correction at one h)
  got = _check(users, items, S, X, Y, TAU, "cosine", corr, "T %d S %d h %d" % (T, S, h))
  losses, m, valid, cvalid, cand, DU, DC = got
  if (live.sum(1) <= 1).all():                                 # no row has a live column but its own
    assert T == 1 and losses == (0.0, 1.0) and m == 1 and not DU.any() and not DC.any()
  else:
    assert losses[0] > 0 and 0 < losses[1] < 1
  if T >= 65:                                                  # |v| = 0: z = 0 and no gradient on its own row
    assert not DU[users == zu].any() and not DC[cand == zi].any()
    if h > 1:
      assert DU[ok & (users != zu)].any(1).all() and DC[:T][ok & (items != zi)].any(1).all()
  again = _grad_gpu(users, items, S, X, Y, TAU, "cosine", corr)
  assert again[:2] == got[:2] and all(np.array_equal(a, b) for a, b in zip(again[2:], got[2:])), "not repeatable"


@pytest.mark.parametrize("T,S,h", [(2, 1, 4), (65, 70, 65), (300, 1, 200)])
def test_grad_of_the_dot_product_against_float64(T, S, h):
  """At (65, 70, 65) the tables are scaled so that the logits of a row span more than 100: exp of a logit without
  the row's maximum taken off would overflow f32."""
  users, items, X, Y, _, _ = _case(T, h, scale=2.0 if h == 65 else 1.0)
  temperature = 1.0 if h == 65 else f32(2.0)
  if h == 65:
    cand = su.candidates(items, SEED, STEP, S, N)
    ok, cvalid, live = su.live_mask(users, items, cand, N, N)
    s = X[users[ok]].astype(np.float64) @ Y[cand[cvalid]].astype(np.float64).T
    assert (np.where(live[ok][:, cvalid], s, -np.inf).max(1) - np.where(live[ok][:, cvalid], s, np.inf).min(1)).max() > 100
    assert s.max() > 89                                        # (expf(89) is past f32)
  corr = su.correction(bpr_util.planted(N, N)[0], T, S, 0.5)
  got = _check(users, items, S, X, Y, temperature, "dot", corr, "dot, T %d S %d h %d" % (T, S, h))
  assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[5])) and np.all(np.isfinite(got[6]))


def test_a_batch_of_invalid_slots_gives_zeros():
  rng = np.random.RandomState(0)
  X, Y = rng.randn(N, 8).astype(np.float32), rng.randn(N, 8).astype(np.float32)
  losses, m, valid, cvalid, cand, DU, DC = _grad_gpu(np.array([-1, N, 3], np.int32), np.array([2, 2, N], np.int32), 5, X, Y)
  assert losses == (0.0, 0.0) and m == 0 and not valid.any() and not DU.any() and not DC.any()
  assert cvalid.tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and np.array_equal(cand, su.candidates([2, 2, N], SEED, STEP, 5, N))


# ---------------------------------------------------------------- one step
def _graph(tr):
  from recoder_amd import als, lightgcn
  return lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))


@pytest.mark.parametrize("K", [2, 0])
def test_one_full_step_against_the_restatement_on_the_same_draws(K):
  from recoder_amd import ssm
  tr, _ = bpr_util.planted()
  h, T, S, w = 24, 256, 64, 1.0
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = _graph(tr)
  state = ssm.new_state(X, Y, K)
  ws = ssm.Workspace(200, 120, T, h, DEV, num_negatives=S)
  ssm.step(X, Y, graph, state, ws, 11, 3, LR, REG, TAU, S, "cosine", w)
  users, pos, cand = ws.bpr.users.cpu().numpy(), ws.bpr.pos.cpu().numpy(), ws.cand.cpu().numpy()
  wu, wp, _ = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and state["step"] == 1
  assert np.array_equal(cand, su.candidates(wp, 11, 3, S, 120))
  assert int(ws.valid_count.item()) == T and bool((ws.bpr.g == 1).all()) and bool((ws.cvalid == 1).all())
  corr = su.correction(tr, T, S, w)
  assert np.array_equal(ws.corr[w].cpu().numpy(), corr)
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  l64, _ = su.step(tr, s64, K, users, pos, cand, LR, REG, TAU, True, corr)
  l32, _ = su.step(tr, s32, K, users, pos, cand, LR, REG, TAU, True, corr, np.float32)
  print("K %d: losses: kernels %s, f32 restatement %s, float64 %s" % (K, ws.loss.cpu().tolist(), l32, l64))
  counts = [np.bincount(users, minlength=200), np.bincount(cand, minlength=120)]
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


def _train(tr, seed, start, epochs=(5,), **kw):
  """train_ssm at its defaults on the planted matrix from the base tables ``start`` (set after an empty fit has built
  the model); more than one entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder()
  ds = RecommendationDataset(tr)
  kw = dict(kw, seed=seed)
  assert rec.train_ssm(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  hist = []
  for k, n in enumerate(epochs):
    hist += rec.train_ssm(ds, num_epochs=n, resume=k > 0, **kw)
  return rec, hist, _tables(rec)


@pytest.fixture(scope="module")
def planted_fit():
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)[:2]
  rec, hist, tables = _train(tr, 0, start)
  return tr, ho, start, rec, hist, tables


def test_train_ssm_lowers_the_loss_repeats_and_resumes_bit_for_bit(planted_fit):
  tr, _, start, rec, hist, tables = planted_fit
  assert len(hist) == 5 and rec.ssm_history == hist and np.all(np.isfinite(hist))
  assert all(len(e) == 2 for e in hist) and hist[-1][0] < hist[0][0] and hist[-1][1] > hist[0][1], hist
  st = rec.ssm_state
  assert st["num_layers"] == 2 and st["step"] == 5 * -(-tr.nnz // 1024) and st["E0"][0].is_cuda
  assert rec.lightgcn_state is None and rec.directau_state is None and rec.directau_history == []
  _, hist2, again = _train(tr, 0, start)
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist
  _, _, other = _train(tr, 1, start)
  assert not np.array_equal(tables[0], other[0]) and not np.array_equal(tables[1], other[1])
  rec3, hist3, resumed = _train(tr, 0, start, epochs=(3, 2))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist
  from recoder_amd.data import RecommendationDataset
  with pytest.raises(ValueError, match="resume=True continues a fit with num_layers = 2 \\(got 0\\)"):
    rec3.train_ssm(RecommendationDataset(tr), num_layers=0, num_epochs=1, resume=True)
  assert all(np.array_equal(a, b) for a, b in zip(resumed, _tables(rec3)))


def test_recall_above_popularity_and_normalize_gives_unit_rows(planted_fit):
  """tests/test_ssm_host.py shows the float64 restatement of the same fit (the defaults, 10 epochs) above popularity."""
  tr, ho, start, rec, _, five = planted_fit
  _, hist, tables = _train(tr, 0, start, epochs=(10,))
  got, pop = su.recall_at(tables[0], tables[1], tr, ho), su.popularity_recall(tr, ho)
  print("planted: Recall@20 of train_ssm %.4f, popularity %.4f, untrained %.4f; history %s"
        % (got, pop, su.recall_at(*start, tr, ho), hist))
  assert got > pop and not tables[2].any()
  rec_n, _, unit = _train(tr, 0, start, normalize=True)
  for a, b in zip(unit[:2], five[:2]):
    norms = np.linalg.norm(a.astype(np.float64), axis=1)
    # (relatively: 16 squares under the root, the root, the division, and the norm as measured here)
    assert np.abs(norms - 1).max() <= (16 + 4) * U24 and np.abs(a - su.unit_rows(b)).max() <= (16 + 4) * U24
  for a, b in zip(rec_n.ssm_state["E0"], rec.ssm_state["E0"]):                  # (the base tables are not touched)
    assert torch.equal(a, b)
  _, _, dot = _train(tr, 0, start, similarity="dot", logq_weight=1.0, num_negatives=0, num_layers=0)
  assert np.all(np.isfinite(dot[0])) and not np.array_equal(dot[0], five[0])


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
  f = rec.save_state(str(tmp_path / "ssm"))
  rec2 = _recoder()
  rec2.init_from_model_file(f)
  assert all(np.array_equal(a, b) for a, b in zip(tables, _tables(rec2)))
  assert np.array_equal(rec.recommend_array(inp, 10), rec2.recommend_array(inp, 10))
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
  bpr_hist = rec.train_bpr(RecommendationDataset(tr), num_epochs=1)                       # (a warm start)
  assert len(bpr_hist) == 1 and np.isfinite(bpr_hist[0])
