"""GPU: rk_als_sx_forward and rk_als_sx_backward against the numpy restatement of their chains (tests/simplex_util.py)
bit for bit, one whole step at gamma = 0.5 against the float64 step, gamma = 1 against train_ccl, and
Recoder.train_simplex / simplex_encode end to end on the ML-20M slice."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util, simplex_util as su

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_ITEMS = 200
LS = (1, 4, 64)
# profiles/simplex_quality.jsonl: the "simplex_test_reference" records -> loss and recall20 of the float64 fit of
# SLICE_FIT itself (tools/simplex_bench.py --test-reference).  The gap allowed on Recall@20 is the one
# tests/test_ccl.py allows its fit (the restatement's spread over five seeds, profiles/ultragcn_quality.jsonl).  The
# loss terms are means over 118144 slots of an epoch; f32 against float64 moves a cosine by about 1e-7 and flips the
# liveness of the few negatives that close to the margin, so an epoch's mean is allowed 1e-3 of its value: four
# orders above the rounding of a term and far below the change from one epoch to the next.
SEED_SPREAD, LOSS_RTOL = 0.0036, 1e-3
REFERENCE_LOSS = ((0.7837321191789196, 0.20054960675386654), (0.7312804128856042, 0.12024618465467737))
REFERENCE_RECALL20 = 0.1277
SLICE_FIT = dict(gamma=0.5, max_history=256, batch_size=1024, lr=0.01, reg=1e-3, num_negatives=64,
                 negative_weight=16.0, margin=0.0)


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, ld, fill=7.0):
  a = np.asarray(a, np.float32)
  full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  full[:, :a.shape[1]] = _t(a)
  return full, full[:, :a.shape[1]]


def _matrix(lengths, rng):
  """One stored row per entry of ``lengths`` over N_ITEMS items, ascending ids; the last row ends in the last item."""
  indptr, indices = [0], []
  for r in lengths:
    row = np.sort(rng.choice(N_ITEMS, r, replace=False))
    indices.extend(row)
    indptr.append(len(indices))
  if lengths[-1]:
    indices[-1] = N_ITEMS - 1
  return sp.csr_matrix((np.ones(len(indices), np.float32), np.array(indices, np.int32), np.array(indptr)),
                       shape=(len(lengths), N_ITEMS))


def _case(T, h, L, short=False):
  """Rows of 1, L - 1, L, L + 1 and 3 L + 1 entries (``short``: none above L - 1, so that E < L), T slots that repeat
  users, among them the last user; from T = 255 on a slot with user -1 and one past the table."""
  rng = np.random.RandomState(1000 * T + 10 * h + L)
  lengths = [1, L - 1, max(L - 2, 0)] if short else [1, L - 1, L, L + 1, 3 * L + 1]
  m = _matrix(lengths, rng)
  n_users = m.shape[0]
  Q, P = rng.randn(N_ITEMS, h).astype(np.float32), rng.randn(n_users, h).astype(np.float32)
  W = (rng.randn(h, h) / np.sqrt(h)).astype(np.float32)
  users = rng.randint(0, n_users, T).astype(np.int32)
  users[-1] = n_users - 1
  if T >= 255:
    users[3], users[10] = -1, n_users
  return m, P, Q, W, users


def _forward_gpu(m, users, Q, P, W, gamma, L, E, compact, ld_pad=3):
  """(B, X, hkey, hcoef) of one rk_als_sx_forward: every table strided, every output filled with 7 first; X is the
  whole table (``compact``: the slots' rows)."""
  from recoder_amd import als, simplex
  T, h = len(users), Q.shape[1]
  ucsr = als.AlsCSR(m, DEV)
  Qf, Qv = _padded(Q, h + ld_pad)
  Wf, Wv = _padded(W, h + ld_pad + 1)
  Pv = None if P is None else _padded(P, h + 2)[1]
  Xf = torch.full((T if compact else m.shape[0], h + ld_pad + 2), 7.0, device=DEV)
  B = torch.full((T, h), 7.0, device=DEV)
  hkey = torch.full((T, E), 7, dtype=torch.int32, device=DEV)
  hcoef = torch.full((T, E), 7.0, device=DEV)
  simplex.forward(_t(users, np.int32), ucsr, Qv, Pv, Wv, gamma, L, Xf[:, :h], compact=compact, B=B, hkey=hkey,
                  hcoef=hcoef)
  assert bool((Xf[:, h:] == 7.0).all()) and bool((Qf[:, h:] == 7.0).all()) and bool((Wf[:, h:] == 7.0).all())
  return tuple(a.cpu().numpy() for a in (B, Xf[:, :h], hkey, hcoef))


def _backward_gpu(DU, valid, B, W, scale, ld_pad=5):
  from recoder_amd import simplex
  T, h = DU.shape
  dB, dW = torch.full((T, h), 7.0, device=DEV), torch.full((h, h), 7.0, device=DEV)
  part = torch.full((-(-T // simplex.CHUNK), h, h), 7.0, device=DEV)
  simplex.backward(_t(DU), _t(valid), _t(B), _padded(W, h + ld_pad)[1], scale, dB, part, dW)
  return dB.cpu().numpy(), dW.cpu().numpy()


def _same(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("h", [1, 7, 32, 33, 64, 200, 512])
@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_forward_and_backward_reproduce_the_restated_chains_bit_for_bit(T, h):
  gamma = 0.375
  for L, short in [(L, False) for L in LS] + [(64, True)]:
    m, P, Q, W, users = _case(T, h, L, short)
    n_users = m.shape[0]
    E = min(L, int(np.diff(m.indptr).max()))
    assert (E < L) == short and E >= 1
    ok = (users >= 0) & (users < n_users)
    wB, wX, wk, wc = su.forward_f32(m, users, Q, P, W, gamma, L, E)
    B, X, hkey, hcoef = _forward_gpu(m, users, Q, P, W, gamma, L, E, compact=False)
    label = (T, h, L, short)
    assert _same(B, wB) and np.array_equal(hkey, wk) and _same(hcoef, wc), label
    assert (hkey[~ok] == N_ITEMS).all() and not B[~ok].any()
    seen = np.zeros(n_users, bool)
    seen[users[ok]] = True
    assert _same(X[users[ok]], wX[ok]), label                  # (two slots of a user: the same bits to the same row)
    assert (X[~seen] == 7.0).all(), label                      # (no other row is touched)
    B64, X64 = su.rows64(m, users, P, Q, W, gamma, L)          # the float64 model, within the f32 forward bound
    terms = np.abs(gamma * P[users[ok]].astype(np.float64)) + (1 - gamma) * (
        np.abs(np.asarray(su.pool_matrix(m, users, L) @ np.abs(Q.astype(np.float64)))) @ np.abs(W.T.astype(np.float64)))[ok]
    assert (np.abs(X[users[ok]] - X64[ok]) <= (h + 2 + E) * 2.0 ** -24 * terms + 1e-300).all(), label
    # P = NULL into a compact table; an invalid slot's row is +0
    _, wX0, _, _ = su.forward_f32(m, users, Q, None, W, gamma, L, E)
    B0, X0, k0, c0 = _forward_gpu(m, users, Q, None, W, gamma, L, E, compact=True, ld_pad=0)
    assert _same(X0, wX0) and _same(B0, wB) and np.array_equal(k0, wk) and _same(c0, wc), label
    assert not X0[~ok].any()
    # two runs, and another grid: the first slots of the batch alone give the same rows
    again = _forward_gpu(m, users, Q, P, W, gamma, L, E, compact=False, ld_pad=17)
    assert all(_same(a, b) for a, b in zip((B, X, hkey, hcoef), again)), label
    n = max(1, T // 3)
    first = _forward_gpu(m, users[:n], Q, None, W, gamma, L, E, compact=True)
    assert _same(first[0], B[:n]) and _same(first[1], X0[:n]) and np.array_equal(first[2], hkey[:n]), label
    if L != 64 or short:
      continue
    # backward on the pooled rows, with invalid slots
    rng = np.random.RandomState(T + h)
    DU = rng.randn(T, h).astype(np.float32)
    valid = (rng.rand(T) > 0.2).astype(np.float32) if T > 1 else np.ones(1, np.float32)
    scale = (1.0 - gamma) / T
    wdB, wdW = su.backward_f32(DU, valid, B, W, scale)
    dB, dW = _backward_gpu(DU, valid, B, W, scale)
    assert _same(dB, wdB) and _same(dW, wdW), label
    assert not dB[valid == 0].any()
    D64 = np.where(valid[:, None] > 0, DU, 0).astype(np.float64)
    s = float(np.float32(scale))
    bound = (h + 2) * 2.0 ** -24 * s * (np.abs(D64) @ np.abs(W.astype(np.float64)))
    assert (np.abs(dB - s * (D64 @ W.astype(np.float64))) <= bound + 1e-300).all(), label
    bound = (T + 1) * 2.0 ** -24 * s * (np.abs(D64).T @ np.abs(B.astype(np.float64)))
    assert (np.abs(dW - s * (D64.T @ B.astype(np.float64))) <= bound + 1e-300).all(), label
    dB2, dW2 = _backward_gpu(DU, valid, B, W, scale, ld_pad=0)
    assert _same(dB, dB2) and _same(dW, dW2), label
    # another grid: invalid slots appended (T = 255, 256: one more chunk) leave dW's bits alone
    pad = 3
    dB3, dW3 = _backward_gpu(np.concatenate([DU, np.ones((pad, h), np.float32)]),
                             np.concatenate([valid, np.zeros(pad, np.float32)]),
                             np.concatenate([B, np.ones((pad, h), np.float32)]), W, scale)
    assert _same(dW3, dW) and _same(dB3[:T], dB) and not dB3[T:].any(), label


def test_the_history_list_feeds_the_entry_scatter():
  """rk_als_ccl_scatter on (hkey, hcoef, self = 0, dB, users = the slot index) sums dB / |H| per history item."""
  from recoder_amd import ccl
  T, h, L = 257, 33, 4
  m, P, Q, W, users = _case(T, h, L)
  E = 4
  B, X, hkey, hcoef = _forward_gpu(m, users, Q, P, W, 0.5, L, E, compact=False)
  dB = np.random.RandomState(3).randn(T, h).astype(np.float32)
  G = torch.zeros((N_ITEMS, h), device=DEV)
  count = torch.zeros(N_ITEMS, dtype=torch.int32, device=DEV)
  keys, order = torch.sort(_t(hkey, np.int32).view(-1), stable=True)
  ccl.scatter(keys, order, E, torch.arange(T, dtype=torch.int32, device=DEV), _t(hcoef), torch.zeros((T, E), device=DEV),
              _t(dB), _t(Q), 1.0, G, count)
  want = np.asarray(su.pool_matrix(m, users, L).T @ dB.astype(np.float64))
  # (a row sums at most T terms, each at most max |dB|: the forward bound of such a sum)
  assert np.abs(G.cpu().numpy() - want).max() <= (T + 2) * 2.0 ** -24 * T * np.abs(dB).max()
  assert np.abs(want).max() > 0


# ---------------------------------------------------------------- one step
def test_one_full_step_at_gamma_half_against_the_float64_step_on_the_same_draws():
  from recoder_amd import als, lightgcn, simplex
  tr, _ = bpr_util.planted()
  h, T, R, lr, reg = 24, 256, 64, float(np.float32(0.05)), float(np.float32(1e-3))
  margin, nw, gamma = float(np.float32(0.2)), 8.0, 0.5
  L = max(2, int(np.diff(tr.indptr).max()) // 2)               # (the longest rows are cut to L entries)
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))
  state = simplex.new_state(X, Y, (gamma, L))
  E = simplex.entry_width(np.diff(tr.indptr), L)
  ws = simplex.Workspace(200, 120, T, h, DEV, num_negatives=R, entries=E, pooled=True)
  simplex.step(X, Y, graph, state, ws, 11, 3, lr, reg, R, nw, margin)
  users, pos = ws.bpr.users.cpu().numpy(), ws.bpr.pos.cpu().numpy()
  wu, wp, _ = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and state["step"] == 1
  negs = su.draws(11, 3, T, R, 120)
  assert np.array_equal(ws.cand.cpu().numpy()[:, 1:], negs) and bool((ws.bpr.g == 1).all())
  s64, s32 = su.new_state(Eu, Ei), su.new_state(Eu, Ei, np.float32)
  l64, cnt, live64 = su.step(tr, s64, gamma, L, users, pos, negs, lr, reg, margin, nw)
  l32, _, live32 = su.step(tr, s32, gamma, L, users, pos, negs, lr, reg, margin, nw, np.float32)
  got = ws.loss.double().sum(0).cpu().numpy()
  live = int(ws.live.sum())
  print("losses: kernels %s, f32 restatement %s, float64 %s; live %d / %d / %d" % (got, l32, l64, live, live32, live64))
  assert cnt == T and 0 < live64 < T * R and live == live32 == live64
  # the yardstick of tests/test_ccl.py: the kernels stay within 4 x the distance of the f32 restatement from float64
  for k in range(2):
    dist, err = abs(l32[k] - l64[k]), abs(got[k] - l64[k])
    print("loss[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (k, dist, err))
    assert dist > 0 and err <= 4 * dist, k
  for key in ("E0", "M", "V"):
    for k in range(3):
      dist = np.abs(s32[key][k] - s64[key][k]).max()
      err = np.abs(state[key][k].cpu().numpy() - s64[key][k]).max()
      print("step %s[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (key, k, dist, err))
      assert np.isfinite(err) and dist > 0 and err <= 4 * dist, (key, k)
  assert np.abs(s64["E0"][2] - np.eye(h)).max() > 0            # (W moved)


# -------------------------------------------------------------- end to end
def _recoder(h=64):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _tables(rec):
  m = rec.model
  return tuple(p.detach().cpu().numpy().copy() for p in
               (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


def _train(tr, start, epochs=(2,), method="train_simplex", **kw):
  """``method`` at SLICE_FIT from the tables ``start`` (set after an empty fit has built the model); more than one
  entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder(start[0].shape[1])
  ds = RecommendationDataset(tr)
  kw = dict(SLICE_FIT, seed=0, **kw)
  if method == "train_ccl":
    kw = dict({k: v for k, v in kw.items() if k not in ("gamma", "max_history")}, num_layers=0)
  fit = getattr(rec, method)
  assert fit(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  hist, stats = [], []
  for k, n in enumerate(epochs):
    hist += fit(ds, num_epochs=n, resume=k > 0, **kw)
    stats += rec.simplex_stats if method == "train_simplex" else rec.ccl_stats
  return rec, hist, stats, _tables(rec)


@pytest.fixture(scope="module")
def slice_fit():
  tr, ho = bpr_util.load_slice()
  start = bpr_util.xavier_tables(tr.shape[0], tr.shape[1], 64, 0)[:2]
  rec, hist, stats, tables = _train(tr, start)
  return tr, ho, start, rec, hist, stats, tables


def test_gamma_one_is_train_ccl_without_layers_bit_for_bit(slice_fit):
  tr, _, start, _, _, _, _ = slice_fit
  rec, hist, stats, tables = _train(tr, start, gamma=1.0)
  ref, chist, cstats, ctables = _train(tr, start, method="train_ccl")
  assert all(np.array_equal(a, b) for a, b in zip(tables, ctables)) and hist == chist and stats == cstats
  s, c = rec.simplex_state, ref.ccl_state
  for key in ("E0", "M", "V"):
    for k in (0, 1):
      assert np.array_equal(s[key][k].cpu().numpy(), c[key][k].cpu().numpy()), (key, k)
  assert s["step"] == c["step"] and torch.equal(s["E0"][2], torch.eye(64, device=DEV)) and not bool(s["M"][2].any())


def test_train_simplex_beside_the_float64_restatement_repeats_and_resumes_bit_for_bit(slice_fit):
  """The same configuration, seed and start as tools/simplex_bench.py --test-reference; ranked by the dot product of
  the un-normalised tables on both sides."""
  tr, ho, start, rec, hist, stats, tables = slice_fit
  assert len(hist) == 2 and rec.simplex_history == hist and np.all(np.isfinite(hist))
  assert all(len(e) == 2 for e in hist) and sum(hist[1]) < sum(hist[0]), hist
  assert len(stats) == 2 and all(0 < s < 1 for s in stats), stats
  st = rec.simplex_state
  assert st["num_layers"] == 0 and st["step"] == 2 * -(-tr.nnz // 1024) and st["gamma"] == 0.5 and \
      st["max_history"] == 256 and tuple(st["E0"][2].shape) == (64, 64) and not tables[2].any()
  assert np.array_equal(tables[1], st["E0"][1].cpu().numpy())  # (Y = Q)
  r20, n100 = su.quality(tables[0], tables[1], tr, ho)
  print("slice: Recall@20 of train_simplex %.4f (NDCG@100 %.4f), float64 restatement %s; history %s (float64 %s), "
        "live %s" % (r20, n100, REFERENCE_RECALL20, hist, REFERENCE_LOSS, stats))
  assert REFERENCE_RECALL20 is not None and REFERENCE_LOSS is not None
  assert abs(r20 - REFERENCE_RECALL20) <= SEED_SPREAD
  assert np.allclose(np.asarray(hist), np.asarray(REFERENCE_LOSS), rtol=LOSS_RTOL, atol=0)
  _, hist2, stats2, again = _train(tr, start)                                    # a fixed seed repeats
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist and stats2 == stats
  rec3, hist3, stats3, resumed = _train(tr, start, epochs=(1, 1))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist and stats3 == stats
  assert torch.equal(rec3.simplex_state["E0"][2], st["E0"][2])


def test_restore_best_leaves_the_best_epochs_bits_and_step_count(slice_fit):
  from recoder_amd.data import RecommendationDataset
  tr, ho, start, _, _, _, _ = slice_fit
  val = RecommendationDataset(tr, ho)
  rec, hist, _, tables = _train(tr, start, epochs=(3,), lr=0.05, val_dataset=val, restore_best=True)
  v = rec.simplex_validation
  assert v is not None and len(v["values"]) == 3 and v["epochs"] == [1, 2, 3] and 1 <= v["best_epoch"] <= 3
  assert len(hist) == 3 and np.all(np.isfinite(v["values"]))
  _, _, _, best = _train(tr, start, epochs=(v["best_epoch"],), lr=0.05)
  assert all(np.array_equal(a, b) for a, b in zip(tables, best))
  assert rec.simplex_state["step"] == v["best_epoch"] * -(-tr.nnz // 1024)


def test_simplex_encode_gives_the_training_rows_at_gamma_zero_and_a_row_to_any_history(slice_fit):
  tr, _, start, rec, _, _, _ = slice_fit
  rng = np.random.RandomState(9)
  unseen = sp.csr_matrix((np.ones(30, np.float32), (np.repeat([0, 2], 15), rng.choice(tr.shape[1], 30, replace=False))),
                         shape=(3, tr.shape[1]))                                 # (row 1 is empty)
  rows = rec.simplex_encode(unseen)
  assert rows.is_cuda and tuple(rows.shape) == (3, 64)
  rows = rows.cpu().numpy()
  assert np.isfinite(rows).all() and rows[0].any() and rows[2].any() and not rows[1].any()
  rec0, _, _, tables = _train(tr, start, epochs=(1,), gamma=0.0)
  enc = rec0.simplex_encode(tr).cpu().numpy()
  assert np.array_equal(enc, tables[0]) and enc.any()
  with pytest.raises(ValueError, match="needs the state of an earlier train_simplex"):
    _recoder().simplex_encode(unseen)


def test_the_fitted_tables_plug_into_the_rest(slice_fit, tmp_path):
  from recoder_amd.data import UsersInteractions
  tr, _, _, rec, _, _, tables = slice_fit
  users = np.arange(50)
  inp = UsersInteractions(users, tr[users])
  lists = rec.recommend(inp, 10)
  assert len(lists) == 50 and all(len(l) == 10 for l in lists)
  f = rec.save_state(str(tmp_path / "simplex"))
  rec2 = _recoder()
  rec2.init_from_model_file(f)
  assert all(np.array_equal(a, b) for a, b in zip(tables, _tables(rec2)))
  assert np.array_equal(rec.recommend_array(inp, 10), rec2.recommend_array(inp, 10))
