"""GPU: rk_als_ccl_grad and rk_als_ccl_scatter against the float64 restatement (tests/ccl_util.py) within 4 x the
error of the f32 restatement that follows the header's chains, their sentinels, long keys and repeatability, one whole
step at 0 and 2 layers, and Recoder.train_ccl end to end on the ML-20M slice.

Measured on an MI355X over the cases of ``ccl_util.CASES`` (largest |f32 restatement - float64| / largest |kernels -
float64| per output): see DESIGN.md section 4, "rk_als_ccl_grad"."""
import numpy as np
import pytest
import torch

from tests import bpr_util, ccl_util as cu, lightgcn_util as lg, ultragcn_util as uu

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, SEED, STEP, MARGIN, NW = cu.N, cu.SEED, cu.STEP, cu.MARGIN, cu.NW
# profiles/ccl_quality.jsonl: the "ccl_test_reference" record -> recall20, the float64 fit of SLICE_FIT itself
# (tools/ccl_bench.py --test-reference); the gap allowed is the one tests/test_ultragcn.py allows its own fit: the
# UltraGCN restatement's Recall@20 spread over five seeds (profiles/ultragcn_quality.jsonl)
SEED_SPREAD, REFERENCE_RECALL20 = 0.0036, 0.0544
SLICE_FIT = dict(num_layers=0, batch_size=1024, lr=0.01, reg=1e-3, num_negatives=64, negative_weight=64.0, margin=0.4)


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _padded(a, ld, fill=7.0):
  a = np.asarray(a, np.float32)
  full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
  full[:, :a.shape[1]] = _t(a)
  return full, full[:, :a.shape[1]]


NAMES = ("cand", "key", "coef", "self", "DU", "valid", "loss", "live")


def _grad_gpu(users, items, R, X, Y, margin=MARGIN, nw=NW, ld_pad=3):
  """The outputs of one rk_als_ccl_grad as a dict; both tables with a padded leading dimension, every output filled
  with 7 first."""
  from recoder_amd import ccl
  T, h, E = len(users), X.shape[1], 1 + R
  Xfull, Xv = _padded(X, h + ld_pad)
  Yfull, Yv = _padded(Y, h + ld_pad + 2)
  i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=DEV)
  f32 = lambda *s: torch.full(s, 7.0, device=DEV)
  out = (i32(T, E), i32(T, E), f32(T, E), f32(T, E), f32(T, h), f32(T), f32(T, 2), i32(T))
  ccl.grad(_t(users, np.int32), _t(items, np.int32), R, SEED, STEP, Xv, Yv, margin, nw, *out)
  assert bool((Xfull[:, h:] == 7.0).all()) and bool((Yfull[:, h:] == 7.0).all()), "a padding column was written"
  return dict(zip(NAMES, (a.cpu().numpy() for a in out)))


def _scatter_gpu(key, coef, self_, users, X, Y, n_rows, ld_pad=3, row_pad=0):
  """(G [n_rows, h], count) after one stable sort of the keys and one rk_als_ccl_scatter at scale 1 / T; G padded in
  its leading dimension (and by ``row_pad`` rows behind the table), zeroed first as the contract asks."""
  from recoder_amd import ccl
  h = X.shape[1]
  full = torch.zeros((n_rows + row_pad, h + ld_pad), device=DEV)
  full[:, h:] = 7.0
  count = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
  keys, order = torch.sort(_t(key, np.int32).view(-1), stable=True)
  ccl.scatter(keys, order, key.shape[1], _t(users, np.int32), _t(coef).contiguous(), _t(self_).contiguous(),
              _padded(X, h + 1)[1], _padded(Y, h + 2)[1], 1.0 / len(users), full[:n_rows, :h], count)
  assert bool((full[:, h:] == 7.0).all()) and not bool(full[n_rows:, :h].any()), "written outside the rows' h columns"
  return full[:n_rows, :h].cpu().numpy(), count.cpu().numpy()


def _ugcn_draws_gpu(users, items, R, X, Y):
  """rk_als_ugcn_grad's cand at K = 0 for the same (seed, step)."""
  from recoder_amd import ultragcn
  T, h = len(users), X.shape[1]
  cand = torch.zeros((T, 1 + R), dtype=torch.int32, device=DEV)
  f32 = lambda *s: torch.zeros(s, device=DEV)
  ultragcn.grad(_t(users, np.int32), _t(items, np.int32), R, 0, SEED, STEP, _t(X), _t(Y), f32(N), f32(N), None, None,
                (1, 1, 1, 1), 1.0, 0.0, cand, f32(T, 1 + R), f32(T, h), f32(T), f32(T, 3))
  return cand.cpu().numpy()


def _within(got, r32, r64, keep, label):
  """max |got - float64| <= 4 max |f32 restatement - float64| over ``keep``; returns both."""
  if not keep.any():
    return 0.0, 0.0
  dist = float(np.abs(r32.astype(np.float64) - r64)[keep].max())
  err = float(np.abs(got.astype(np.float64) - r64)[keep].max())
  assert err <= 4 * dist, (label, err, dist)
  return dist, err


def _check(T, R, h, margin=MARGIN, nw=NW, worst=None):
  X, Y, users, items = cu.case(T, R, h)
  negs = cu.draws(SEED, STEP, T, R, N)
  r64 = cu.grad_rows(users, items, negs, X, Y, margin, nw)
  r32 = cu.grad_rows_f32(users, items, negs, X, Y, margin, nw)
  got = _grad_gpu(users, items, R, X, Y, margin, nw)
  label = (T, R, h)
  assert np.array_equal(got["cand"], r64["cand"]) and np.array_equal(got["cand"], _ugcn_draws_gpu(users, items, R, X, Y))
  assert np.array_equal(got["valid"], r64["valid"]), label
  near = cu.near_margin(r64, margin)
  assert near.sum() <= 0.01 * near.size, label
  far, far_slot = ~near, ~near.any(1)
  assert np.array_equal(got["key"][far], r64["key"][far]), label
  assert np.array_equal(got["live"][far_slot], r64["live"][far_slot]), label
  dead = got["key"] == N
  for name in ("coef", "self"):
    assert not got[name][dead].any() and not np.signbit(got[name][dead]).any(), (label, name)       # (+0)
  worst = {} if worst is None else worst
  for name, keep in (("coef", far), ("self", far), ("DU", far_slot[:, None] & np.ones((1, h), bool)),
                     ("loss", far_slot[:, None] & np.ones((1, 2), bool))):
    d, e = _within(got[name], r32[name], r64[name], keep, label + (name,))
    worst[name] = tuple(max(a, b) for a, b in zip(worst.get(name, (0.0, 0.0)), (d, e)))
  # the scatter, on the kernel's own entries; the rows a near entry could touch are left out
  G, count = _scatter_gpu(got["key"], got["coef"], got["self"], users, X, Y, N)
  G32, c32 = cu.scatter_rows(r32["key"], r32["coef"], r32["self"], users, X, Y, N, np.float32)
  G32 = (np.float32(1.0 / T) * G32).astype(np.float32)
  rows = np.ones(N, bool)
  rows[np.unique(r64["cand"][near])] = False
  d, e = _within(G, G32, r64["DI"] / T, rows[:, None] & np.ones((1, h), bool), label + ("G",))
  worst["G"] = tuple(max(a, b) for a, b in zip(worst.get("G", (0.0, 0.0)), (d, e)))
  assert np.array_equal(count[rows], r64["count"][rows]), label
  untouched = np.bincount(got["key"].ravel(), minlength=N + 1)[:N] == 0
  assert not G[untouched].any() and not np.signbit(G[untouched]).any(), label
  return worst


@pytest.mark.parametrize("h", [1, 3, 20, 64, 65, 200, 512])       # (20: the two-candidate lane groups of 32)
@pytest.mark.parametrize("T", [1, 2, 65, 257])
def test_grad_and_scatter_against_float64(T, h):
  assert (T, 5, h) in cu.CASES
  worst = _check(T, 5, h)
  print("T %d h %d: (f32 restatement, kernels) - float64 %s" % (T, h, {k: "%.3g / %.3g" % v for k, v in worst.items()}))


def test_grad_and_scatter_against_float64_at_64_negatives():
  assert (65, 64, 64) in cu.CASES
  worst = _check(65, 64, 64)
  print("R 64: (f32 restatement, kernels) - float64 %s" % {k: "%.3g / %.3g" % v for k, v in worst.items()})
  assert all(v[0] > 0 for v in worst.values())               # (the comparison is not vacuous)


# ------------------------------------------------- zero rows and dead slots
def test_zero_norm_rows_give_zero_gradient_rows_and_sentinel_keys():
  T, R, h = 65, 5, 20
  X, Y, users, items = cu.case(T, R, h)                        # user row 7 (slot 10) and item row 9 (slot 11) are 0
  got = _grad_gpu(users, items, R, X, Y, margin=-0.5)          # (margin < 0: a zero-norm negative is live, c = 0)
  assert (got["key"][10] == N).all() and not got["DU"][10].any() and got["valid"][10] == 1
  assert not got["coef"][10].any() and not got["self"][10].any() and got["loss"][10, 0] == 1.0
  at9 = got["cand"] == 9
  assert at9.sum() > 1 and (got["key"][at9] == N).all() and not got["coef"][at9].any()
  assert got["live"][10] == R and got["loss"][10, 1] == np.float32(np.float32(NW) / np.float32(R)) * np.float32(2.5)
  G, count = _scatter_gpu(got["key"], got["coef"], got["self"], users, X, Y, N)
  assert not G[9].any() and count[9] == 0
  ref = cu.grad_rows(users, items, cu.draws(SEED, STEP, T, R, N), X, Y, -0.5, NW)
  assert np.array_equal(got["key"], ref["key"]) and np.array_equal(got["live"], ref["live"])
  assert np.array_equal(count, ref["count"])


def test_a_margin_of_0999_leaves_the_positives_update_alone_and_gathers_nothing_for_the_dead():
  T, R, h = 65, 64, 64
  X, Y, users, items = cu.case(T, R, h)
  users[:] = np.where(users >= 0, users % 20, users)
  items[:] = np.where(items < N, items % 20, items)            # (items 20..39 occur only as negatives)
  got = _grad_gpu(users, items, R, X, Y, margin=0.999)
  ref = cu.grad_rows(users, items, cu.draws(SEED, STEP, T, R, N), X, Y, 0.999, NW)
  assert np.array_equal(got["key"], ref["key"]) and np.array_equal(got["live"], ref["live"])
  none = (got["live"] == 0) & (got["valid"] > 0)
  assert none.sum() >= T - 10 and (got["key"][none, 1:] == N).all() and not got["loss"][none, 1].any()
  r32 = cu.grad_rows_f32(users, items, cu.draws(SEED, STEP, T, R, N), X, Y, 0.999, NW)
  _within(got["DU"], r32["DU"], ref["DU"], np.ones_like(ref["DU"], bool), "DU")
  G, count = _scatter_gpu(got["key"], got["coef"], got["self"], users, X, Y, N)
  only_dead = np.bincount(got["key"].ravel(), minlength=N + 1)[:N] == 0
  assert only_dead[20:].sum() >= 15 and (np.bincount(got["cand"][got["cand"] < N], minlength=N)[only_dead] > 0).any()
  assert not G[only_dead].any() and not np.signbit(G[only_dead]).any() and not count[only_dead].any()   # exactly +0
  keys, order = torch.sort(_t(got["key"], np.int32).view(-1), stable=True)
  assert int((keys < N).sum()) < keys.numel() // 10


def test_a_batch_of_invalid_slots_gives_zeros_and_sentinels():
  X, Y, _, _ = cu.case(65, 5, 4)
  got = _grad_gpu(np.array([-1, N, 3], np.int32), np.array([2, 2, N], np.int32), 5, X, Y)
  assert (got["cand"] == N).all() and (got["key"] == N).all() and not got["live"].any()
  assert not any(got[k].any() for k in ("coef", "self", "DU", "valid", "loss"))
  G, count = _scatter_gpu(got["key"], got["coef"], got["self"], np.array([-1, N, 3], np.int32), X, Y, N, row_pad=2)
  assert not G.any() and not count.any()


# ---------------------------------------------------------------- long keys
@pytest.mark.parametrize("h", [33, 130, 512])
def test_scatter_hands_keys_of_1023_and_1024_and_more_than_4096_entries_to_the_right_path(h):
  """Sorted layout: key 0 holds exactly 1024 entries (long), key 1 holds 1023 (short, beginning on the multiple
  1024), key 2 holds 1024 (long, beginning at 2047), key 3 holds 4200 (long, several multiples inside: only the first
  workgroup takes it), the rest are sentinels or lie past the table.  One slot has user -1."""
  from recoder_amd import ccl
  assert ccl.LONG_KEY == cu.LONG_KEY == 1024
  T, E = 1500, 5
  rng = np.random.RandomState(h)
  lengths = [1024, 1023, 1024, 4200]
  flat = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(lengths)] +
                        [np.full(T * E - sum(lengths), N, np.int32)])
  flat[-7:] = N + 3                                            # (keys past the table)
  key = rng.permutation(flat).reshape(T, E)
  coef, self_ = rng.randn(T, E).astype(np.float32), rng.randn(T, E).astype(np.float32)
  X, Y = (rng.randn(N, h) * 0.5).astype(np.float32), (rng.randn(N, h) * 0.5).astype(np.float32)
  users = rng.randint(0, N, T).astype(np.int32)
  users[17] = -1
  G, count = _scatter_gpu(key, coef, self_, users, X, Y, N, row_pad=2)
  want, wc = cu.scatter_rows(key, coef, self_, users, X, Y, N)
  G32, c32 = cu.scatter_rows(key, coef, self_, users, X, Y, N, np.float32)
  G32 = (np.float32(1.0 / T) * G32).astype(np.float32)
  for k in range(4):
    dist, err = np.abs(G32[k] - want[k] / T).max(), np.abs(G[k] - want[k] / T).max()
    print("h %d key %d (%d entries): f32 restatement - float64 %.3g, kernel - float64 %.3g" % (h, k, lengths[k], dist, err))
    assert dist > 0 and err <= 4 * dist, k
  assert np.array_equal(count, wc) and np.array_equal(count, c32) and count[:4].min() > 0 and not G[4:].any()
  again, count2 = _scatter_gpu(key, coef, self_, users, X, Y, N, ld_pad=11)
  assert np.array_equal(G, again) and np.array_equal(count, count2)


def test_scatter_of_keys_past_the_table_writes_nothing():
  T, E, h = 70, 5, 9
  key = np.full((T, E), N, np.int32)
  ones = np.ones((T, E), np.float32)
  X = np.ones((N, h), np.float32)
  for n_rows in (N, 7):                                        # (a shorter table: still past it)
    G, count = _scatter_gpu(key, ones, ones, np.zeros(T, np.int32), X, X, n_rows, row_pad=2)
    assert not G.any() and not count.any()


# ------------------------------------------------------- leading dimensions
@pytest.mark.parametrize("h", [3, 20, 64, 200])
def test_the_same_call_gives_the_same_bits_whatever_the_leading_dimensions(h):
  T, R = 65, 65
  X, Y, users, items = cu.case(T, R, h)
  first = _grad_gpu(users, items, R, X, Y)
  for pad in (3, 0, 64):
    again = _grad_gpu(users, items, R, X, Y, ld_pad=pad)
    assert all(np.array_equal(first[k], again[k]) for k in NAMES), pad
  args = (first["key"], first["coef"], first["self"], users, X, Y)
  G, count = _scatter_gpu(*args, N)
  for pad, rows in ((3, 0), (0, 0), (17, 5)):
    G2, count2 = _scatter_gpu(*args, N, ld_pad=pad, row_pad=rows)
    assert np.array_equal(G, G2) and np.array_equal(count, count2), (pad, rows)
  # a row range: a table cut after row 20 receives the same rows 0..19 and ignores the keys behind them
  G3, count3 = _scatter_gpu(*args, 20, row_pad=3)
  assert np.array_equal(G3, G[:20]) and np.array_equal(count3, count[:20])
  # the draws of a slot do not depend on T: the first slots of a longer batch give the same rows
  short = _grad_gpu(users[:9], items[:9], R, X, Y)
  assert all(np.array_equal(first[k][:9], short[k]) for k in NAMES)


# ---------------------------------------------------------------- one step
@pytest.mark.parametrize("K", [0, 2])
def test_one_full_step_against_the_restatement_on_the_same_draws(K):
  from recoder_amd import als, ccl, lightgcn
  tr, _ = bpr_util.planted()
  h, T, R, lr, reg = 24, 256, 64, float(np.float32(0.05)), float(np.float32(1e-3))
  margin, nw = float(np.float32(0.2)), 8.0
  rng = np.random.RandomState(5)
  Eu, Ei = (0.3 * rng.randn(200, h)).astype(np.float32), (0.3 * rng.randn(120, h)).astype(np.float32)
  X, Y = _t(Eu), _t(Ei)
  graph = lightgcn.Graph(*als.csr_pair(tr, tr.shape[0], tr.shape[1], DEV))
  state = ccl.new_state(X, Y, K)
  ws = ccl.Workspace(200, 120, T, h, DEV, num_negatives=R)
  ccl.step(X, Y, graph, state, ws, 11, 3, lr, reg, R, nw, margin)
  users, pos = ws.bpr.users.cpu().numpy(), ws.bpr.pos.cpu().numpy()
  wu, wp, _ = bpr_util.sample(tr, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and state["step"] == 1 and state["num_layers"] == K
  negs = cu.draws(11, 3, T, R, 120)
  assert np.array_equal(ws.cand.cpu().numpy()[:, 1:], negs) and bool((ws.bpr.g == 1).all())
  s64, s32 = lg.new_state(Eu, Ei), lg.new_state(Eu, Ei, np.float32)
  l64, cnt, live64 = cu.step(tr, s64, K, users, pos, negs, lr, reg, margin, nw)
  l32, _, live32 = cu.step(tr, s32, K, users, pos, negs, lr, reg, margin, nw, np.float32)
  got = ws.loss.double().sum(0).cpu().numpy()
  live = int(ws.live.sum())
  print("losses: kernels %s, f32 restatement %s, float64 %s; live %d / %d / %d" % (got, l32, l64, live, live32, live64))
  assert cnt == T and 0 < live64 < T * R and live == live32 == live64
  # the yardstick of tests/test_lightgcn.py: the kernels stay within 4 x the distance of the f32 restatement (every
  # operation of the step in f32) from float64
  for k in range(2):
    dist, err = abs(l32[k] - l64[k]), abs(got[k] - l64[k])
    print("loss[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (k, dist, err))
    assert dist > 0 and err <= 4 * dist, k
  counts = [np.bincount(users, minlength=200), np.bincount(pos, minlength=120)]
  for side in (0, 1):
    assert np.array_equal(ws.count[side].cpu().numpy(), counts[side])
  for key in ("E0", "M", "V"):
    for side in (0, 1):
      dist = np.abs(s32[key][side] - s64[key][side]).max()
      err = np.abs(state[key][side].cpu().numpy() - s64[key][side]).max()
      print("step %s[%d]: f32 restatement - float64 %.3g, kernels - float64 %.3g" % (key, side, dist, err))
      assert dist > 0 and err <= 4 * dist, (key, side)


# -------------------------------------------------------------- end to end
def _recoder(h=64):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _tables(rec):
  m = rec.model
  return tuple(p.detach().cpu().numpy().copy() for p in
               (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


def _train(tr, start, epochs=(2,), validation=None, **kw):
  """train_ccl at SLICE_FIT from the tables ``start`` (set after an empty fit has built the model); more than one
  entry in ``epochs``: the later ones with resume=True."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder(start[0].shape[1])
  ds = RecommendationDataset(tr)
  kw = dict(SLICE_FIT, seed=0, **kw)
  assert rec.train_ccl(ds, num_epochs=0, **kw) == [] and rec.ccl_stats == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight), start):
    p.data.copy_(_t(a))
  rec.fit_validation = validation
  hist, stats = [], []
  for k, n in enumerate(epochs):
    hist += rec.train_ccl(ds, num_epochs=n, resume=k > 0, **kw)
    stats += rec.ccl_stats
  return rec, hist, stats, _tables(rec)


@pytest.fixture(scope="module")
def slice_fit():
  tr, ho = bpr_util.load_slice()
  start = bpr_util.xavier_tables(tr.shape[0], tr.shape[1], 64, 0)[:2]
  rec, hist, stats, tables = _train(tr, start)
  return tr, ho, start, rec, hist, stats, tables


def test_train_ccl_lowers_the_loss_repeats_and_resumes_bit_for_bit(slice_fit):
  tr, _, start, rec, hist, stats, tables = slice_fit
  assert len(hist) == 2 and rec.ccl_history == hist and np.all(np.isfinite(hist))
  assert all(len(e) == 2 for e in hist) and sum(hist[1]) < sum(hist[0]), hist
  assert len(stats) == 2 and all(0 < s < 1 for s in stats), stats
  st = rec.ccl_state
  assert st["num_layers"] == 0 and st["step"] == 2 * -(-tr.nnz // 1024) and st["E0"][0].is_cuda
  assert rec.ultragcn_state is None and rec.ssm_state is None and not tables[2].any()
  _, hist2, stats2, again = _train(tr, start)                                    # a fixed seed repeats
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist and stats2 == stats
  _, hist3, stats3, resumed = _train(tr, start, epochs=(1, 1))
  assert all(np.array_equal(a, b) for a, b in zip(tables, resumed)) and hist3 == hist and stats3 == stats


def test_normalize_leaves_unit_rows_and_the_state_untouched(slice_fit):
  tr, _, start, rec, _, _, tables = slice_fit
  rec2, _, _, unit = _train(tr, start, epochs=(1,), normalize=True)
  norms = np.linalg.norm(unit[1], axis=1)
  assert np.abs(norms[norms > 0] - 1).max() < 1e-5
  _, _, _, plain = _train(tr, start, epochs=(1,))
  assert np.array_equal(rec2.ccl_state["E0"][1].cpu().numpy(), plain[1])         # (num_layers 0: the base tables)


def test_recall_of_the_fit_beside_the_float64_restatement(slice_fit):
  """The same configuration, seed and start as tools/ccl_bench.py --test-reference; ranked by the dot product of the
  un-normalised tables on both sides."""
  tr, ho, _, _, hist, stats, tables = slice_fit
  assert REFERENCE_RECALL20 is not None
  r20, n100 = cu.quality(tables[0], tables[1], tr, ho)
  print("slice: Recall@20 of train_ccl %.4f (NDCG@100 %.4f), float64 restatement %.4f, margin %.4f; history %s, live %s"
        % (r20, n100, REFERENCE_RECALL20, SEED_SPREAD, hist, stats))
  assert abs(r20 - REFERENCE_RECALL20) <= SEED_SPREAD


def test_fit_validation_fills_ccl_validation_and_restore_best_leaves_the_best_epochs_bits(slice_fit):
  from recoder_amd.data import RecommendationDataset
  tr, ho, start, _, _, _, _ = slice_fit
  val = RecommendationDataset(tr, ho)
  rec, hist, _, tables = _train(tr, start, epochs=(3,), lr=0.05,
                                validation=dict(val_dataset=val, restore_best=True))
  v = rec.ccl_validation
  assert v is not None and len(v["values"]) == 3 and v["epochs"] == [1, 2, 3] and 1 <= v["best_epoch"] <= 3
  assert len(hist) == 3 and np.all(np.isfinite(v["values"]))
  _, _, _, best = _train(tr, start, epochs=(v["best_epoch"],), lr=0.05)
  assert all(np.array_equal(a, b) for a, b in zip(tables, best))
  assert rec.ccl_state["step"] == v["best_epoch"] * -(-tr.nnz // 1024)


def test_the_fitted_tables_plug_into_the_rest(slice_fit, tmp_path):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.metrics import Recall
  tr, ho, _, rec, _, _, tables = slice_fit
  users = np.arange(50)
  inp = UsersInteractions(users, tr[users])
  lists = rec.recommend(inp, 10)
  assert len(lists) == 50 and all(len(l) == 10 for l in lists)
  seen = tr[users].toarray() > 0
  assert not any(seen[u, l].any() for u, l in enumerate(lists)) and all(len(set(l)) == 10 for l in lists)
  sub = np.arange(1000)
  res = rec.evaluate(RecommendationDataset(tr[sub], ho[sub]), num_recommendations=20,
                     metrics=[Recall(k=20, normalize=True)], batch_size=500)
  assert np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)) > 20.0 / tr.shape[1]      # (above chance)
  f = rec.save_state(str(tmp_path / "ccl"))
  rec2 = _recoder()
  rec2.init_from_model_file(f)
  assert all(np.array_equal(a, b) for a, b in zip(tables, _tables(rec2)))
  assert np.array_equal(rec.recommend_array(inp, 10), rec2.recommend_array(inp, 10))
  index = ExactEmbeddingsIndex.from_recoder(rec)
  nn = index.get_nns_by_id(5, 10)
  assert len(nn) == 10 and nn[0] == 5
