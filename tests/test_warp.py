"""GPU: rk_als_rank_sample and rk_als_warp_grad (recoder_amd/warp.py) against the restatement of
tests/warp_util.py -- on exact tables (entries k/8: every score is exact in f32 in any order, so every decision
is an integer fact) bit for bit, on Gaussian tables the scores within the rounding of their chain and the
decisions exactly the sequential rule on the kernel's own scores -- then one whole WARP step, Recoder.train_warp
and train_bpr(num_candidates=...) end to end with what the fitted tables plug into."""
import functools

import numpy as np
import pytest
import torch

from tests import bpr_util, warp_util
from tests.test_bpr import LR, REG, U23, _apply_bounds, _csr, _t, _tables, _wide_matrix

pytestmark = pytest.mark.gpu

DEV = "cuda"
WARP, DNS = warp_util.WARP, warp_util.DNS
HIGH = (11, 20)                   # (users of edge_matrix whose positives cannot be violated at margin 0)


@functools.lru_cache(maxsize=None)
def _edge():
  m = bpr_util.edge_matrix()
  return m, warp_util.Sampler(m), _csr(m)


@functools.lru_cache(maxsize=None)
def _exact(h):
  m, _, _ = _edge()
  tables = warp_util.exact_tables(37, 53, h, 100 + h, high_bias_users=HIGH, csr=m)
  return tables, tuple(_t(a) for a in tables)


def _sample(csr, dev_tables, seed, step, T, mode, max_draws, M, margin):
  """rk_als_rank_sample into buffers filled with junk: every entry has to be written."""
  from recoder_amd import warp
  ints = [torch.full((T,), -7, dtype=torch.int32, device=DEV) for _ in range(4)]
  s_pos, s_neg = (torch.full((T,), 7.0, device=DEV) for _ in range(2))
  scores = torch.full((T, max_draws), 7.0, device=DEV)
  warp.sample(csr, seed, step, *dev_tables, mode, max_draws, M, margin, *ints, s_pos, s_neg, scores)
  return tuple(v.cpu().numpy() for v in ints + [s_pos, s_neg, scores])


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
  for name, a, w in zip(("users", "pos", "neg", "trials"), got[:4], want[:4]):
    assert a.dtype == np.int32 and np.array_equal(a, w), name
  for name, a, w in zip(("s_pos", "s_neg", "scores"), got[4:], want[4:]):
    assert np.array_equal(_bits(a), _bits(w)), name           # (bits: a -0 where +0 is due would show)


# ------------------------------------------------------- sampler, exact tables
@pytest.mark.parametrize("mode", [WARP, DNS])
@pytest.mark.parametrize("max_draws", [1, 32, 64, 65, 256])
@pytest.mark.parametrize("h", [1, 64, 65, 512])
def test_sampler_on_exact_tables_is_bitwise_the_restatement(h, max_draws, mode):
  """Seeds {0, -(2^40) - 3} x steps {0, 7} x margins {0, 1} (DNS, where the margin plays no part: x 3 and 11
  candidates, which end inside a group of rows in flight and past one) at T = 257."""
  m, sm, csr = _edge()
  (X, Y, b), dev = _exact(h)
  T = 257
  seen = dict(invalid=0, no_violator=0, later_violator=0, tie=0)
  for seed in (0, -(2 ** 40) - 3):
    for step in (0, 7):
      for margin, M in ((0.0, min(max_draws, 3)), (1.0, min(max_draws, 11))):
        got = _sample(csr, dev, seed, step, T, mode, max_draws, M, margin)
        want = sm.sample(seed, step, T, X, Y, b, mode, max_draws, M, margin)
        _same(got, want)
        users, _, neg, trials, _, _, scores = want
        assert (neg[users == 5] == -1).all() and (trials[users == 5] == 0).all()
        seen["invalid"] += int((users == 5).sum())
        if mode == WARP:
          seen["no_violator"] += int(((neg < 0) & np.isin(users, HIGH)).sum())
          seen["later_violator"] += int((trials > 1).sum())
        else:
          _, _, C, cand = sm.draws(seed, step, T, max_draws)
          taken = cand & (np.cumsum(cand, 1) <= M)
          at_top = taken & (scores == np.where(taken, scores, -np.inf).max(1, keepdims=True))
          tied, first = at_top.sum(1) > 1, at_top.argmax(1)
          # the winner of a tie is the earlier draw; a tie counts as seen when it is between different items
          assert np.array_equal(neg[tied], C[np.arange(T), first][tied].astype(np.int32))
          seen["tie"] += int((tied & (np.where(at_top, C, 2 ** 40).min(1) != np.where(at_top, C, -1).max(1))).sum())
  assert seen["invalid"] > 0
  if mode == WARP:
    assert seen["no_violator"] > 0
    assert max_draws == 1 or seen["later_violator"] > 0
  elif h == 1 and max_draws >= 32:
    assert seen["tie"] > 0


def test_dns_with_one_candidate_and_32_draws_is_bpr_sample_bitwise():
  from recoder_amd import bpr
  m, _, csr = _edge()
  T = 257
  dev = tuple(_t(a) for a in _tables(37, 53, 65, 3))
  for seed, step in ((0, 0), (-(2 ** 40) - 3, 7)):
    want = [torch.full((T,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    bpr.sample(csr, seed, step, *want)
    got = _sample(csr, dev, seed, step, T, DNS, 32, 1, 0.0)
    for a, w in zip(got[:3], want):
      assert np.array_equal(a, w.cpu().numpy())
    assert np.array_equal(got[3], (got[2] >= 0).astype(np.int32))


# ------------------------------------------------------------ Gaussian tables
@pytest.mark.parametrize("mode", [WARP, DNS])
@pytest.mark.parametrize("h", [1, 64, 65, 512])
def test_gaussian_tables_scores_within_the_chain_bound_and_decisions_exact(h, mode):
  """Every written score within (h + 4) 2^-23 (sum |p||q| + |b|) of float64 (test_bpr.py's bound for the same
  chain); neg / trials / s_neg exactly the sequential rule applied in float32 to the kernel's own scores and
  s_pos, for every slot; nothing written behind the stopping point."""
  m, sm, csr = _edge()
  X, Y, b = _tables(37, 53, h, h)
  T, D, M, margin = 257, 65, 11, 0.5
  got = _sample(csr, tuple(_t(a) for a in (X, Y, b)), 3, 2, T, mode, D, M, margin)
  users, pos, neg, trials, s_pos, s_neg, scores = got
  wu, wp, C, cand = sm.draws(3, 2, T, D)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp)
  X64, Y64, b64 = (a.astype(np.float64) for a in (X, Y, b))
  S64 = np.einsum("th,tdh->td", X64[wu], Y64[C]) + b64[C]
  bound = (h + 4) * U23 * (np.einsum("th,tdh->td", np.abs(X64[wu]), np.abs(Y64[C])) + np.abs(b64[C]))
  p64 = (X64[wu] * Y64[wp]).sum(1) + b64[wp]
  pb = (h + 4) * U23 * ((np.abs(X64[wu]) * np.abs(Y64[wp])).sum(1) + np.abs(b64[wp]))
  print("h %d: max |s_pos^ - s_pos| / bound %.3f" % (h, (np.abs(s_pos - p64) / pb).max()))
  assert np.all(np.abs(s_pos - p64) <= pb)
  wn, wt, wsn, written = warp_util.decide(C, cand, scores, s_pos, mode, M, margin)
  assert scores.dtype == np.float32 and s_pos.dtype == np.float32
  assert np.array_equal(neg, wn) and np.array_equal(trials, wt) and np.array_equal(_bits(s_neg), _bits(wsn))
  assert not _bits(scores)[~written].any()                      # (+0 where held or not reached)
  err = np.abs(scores - S64)[written]
  print("h %d mode %d: %d scores, max err / bound %.3f" % (h, mode, written.sum(), (err / bound[written]).max()))
  assert written.sum() > T and np.all(err <= bound[written])
  assert (trials > 1).any() and (neg < 0).any()


@pytest.mark.parametrize("mode", [WARP, DNS])
def test_a_slot_does_not_depend_on_the_launch(mode):
  m, _, csr = _edge()
  dev = tuple(_t(a) for a in _tables(37, 53, 65, 9))
  long, short = (_sample(csr, dev, 4, 1, T, mode, 65, 11, 0.5) for T in (257, 64))
  for a, w in zip(long[:4], short[:4]):
    assert np.array_equal(a[:64], w)
  for a, w in zip(long[4:], short[4:]):
    assert np.array_equal(_bits(a[:64]), _bits(w))


# --------------------------------------------------------------------- grad
@pytest.mark.parametrize("h", [1, 64, 65, 512])
def test_warp_grad_against_float64(h):
  """g is the table's entry; the loss g ((s_neg - s_pos) + margin) is within g times the two scores' chain bounds,
  plus one rounding (2^-24 relative) for each of the subtraction, the addition and the product."""
  from recoder_amd import warp
  m, sm, _ = _edge()
  X, Y, b = _tables(37, 53, h, h + 1)
  T, margin = 130, 0.5
  users, pos, neg, trials = sm.sample(3, 2, T, X, Y, b, WARP, 32, 1, margin)[:4]
  trials = trials.copy()
  last, zero, past = np.flatnonzero(neg >= 0)[:3]
  trials[last], trials[zero], trials[past] = 256, 0, 257     # (the table's last entry; two invalid counts)
  assert (neg < 0).any() and (neg >= 0).sum() > 60
  weight = warp.weight_table(100000, "harmonic")
  g, loss = (torch.full((T,), 7.0, device=DEV) for _ in range(2))
  D, P = (torch.full((T, h), 7.0, device=DEV) for _ in range(2))
  warp.grad(_t(users, np.int32), _t(pos, np.int32), _t(neg, np.int32), _t(trials, np.int32), _t(X), _t(Y), _t(b),
            margin, _t(weight), g, loss, D, P)
  g, loss, D, P = (v.cpu().numpy() for v in (g, loss, D, P))
  ok = (neg >= 0) & (trials >= 1) & (trials <= 256)
  assert not ok[zero] and not ok[past] and ok[last]
  wg = np.where(ok, weight[np.clip(trials, 0, 256)], np.float32(0))
  assert np.array_equal(_bits(g), _bits(wg)) and g[last] == weight[256]
  X64, Y64, b64 = (a.astype(np.float64) for a in (X, Y, b))
  u, i, j = users[ok], pos[ok], neg[ok]
  sp, sn = (X64[u] * Y64[i]).sum(1) + b64[i], (X64[u] * Y64[j]).sum(1) + b64[j]
  cb = (h + 4) * U23 * ((np.abs(X64[u]) * (np.abs(Y64[i]) + np.abs(Y64[j]))).sum(1) + np.abs(b64[i]) + np.abs(b64[j]))
  want = wg[ok].astype(np.float64) * ((sn - sp) + margin)
  lb = wg[ok] * (cb + U23 * (np.abs(sn) + np.abs(sp) + margin)) + U23 * np.abs(want)
  print("h %d: max loss err / bound %.3f" % (h, (np.abs(loss[ok] - want) / lb).max()))
  assert np.all(np.abs(loss[ok] - want) <= lb)
  wantD, wantP = np.zeros((T, h), np.float32), np.zeros((T, h), np.float32)
  wantD[ok], wantP[ok] = Y[i] - Y[j], X[u]
  assert np.array_equal(_bits(D), _bits(wantD)) and np.array_equal(_bits(P), _bits(wantP))
  assert not _bits(g)[~ok].any() and not _bits(loss)[~ok].any()


# ---------------------------------------------------------------- one step
def test_one_full_warp_step_against_the_restatement():
  from recoder_amd import warp
  m = _wide_matrix()
  h, T, margin = 24, 256, 1.0
  X, Y, b = warp_util.exact_tables(200, 120, h, 5)
  Xt, Yt, bt = _t(X), _t(Y), _t(b)
  ws = warp.Workspace(T, h, DEV)
  weight = warp.weight_table(120, "log")
  warp.step(Xt, Yt, bt, _csr(m), ws, _t(weight), 11, 3, LR, REG, margin, 32)
  users, pos, neg, trials, s_pos, s_neg = (v.cpu().numpy() for v in (ws.users, ws.pos, ws.neg, ws.trials, ws.s_pos, ws.s_neg))
  want = warp_util.Sampler(m).sample(11, 3, T, X, Y, b, WARP, 32, 1, margin)
  _same((users, pos, neg, trials, s_pos, s_neg), want[:6])
  assert (neg >= 0).sum() > 100 and (trials > 1).any()
  g, _, D64, P64 = warp_util.grad(users, pos, neg, trials, X, Y, b, margin, weight)
  assert np.array_equal(ws.g.cpu().numpy(), g.astype(np.float32))          # (g exact: the table's f32 entries)
  wantX, wantY, wantb = bpr_util.apply(users, pos, neg, g, D64, P64, X, Y, b, LR, REG)
  bounds = _apply_bounds(users, pos, neg, g.astype(np.float32), D64, P64, X, Y, b, LR, REG)
  for name, a, w, bd in zip("XYb", (Xt, Yt, bt), (wantX, wantY, wantb), bounds):
    err = np.abs(a.cpu().numpy() - w)
    print("step %s: max err / bound %.3f" % (name, (err / np.maximum(bd, 1e-300)).max()))
    assert np.all(err <= bd), name
  assert not np.array_equal(Xt.cpu().numpy(), X)
  assert np.array_equal(Xt[0].cpu().numpy(), X[0]) and np.array_equal(Xt[9].cpu().numpy(), X[9])


# -------------------------------------------------------------- end to end
CFG = dict(batch_size=256, lr=0.02, reg=0.01, margin=1.0, max_draws=32, rank_weight="log")
AUC_TOL = 0.006337


def _recoder(h=16):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _start(rec, ds, start, method, **kw):
  """An empty fit builds the model; then the tables are set to ``start``."""
  assert getattr(rec, method)(ds, num_epochs=0, **kw) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias), start):
    p.data.copy_(_t(a))


def _tables_of(rec):
  m = rec.model
  return tuple(p.detach().cpu().numpy() for p in (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


def _train_warp(tr, seed, start, epochs=5):
  from recoder_amd.data import RecommendationDataset
  rec, ds = _recoder(), RecommendationDataset(tr)
  _start(rec, ds, start, "train_warp", seed=seed, **CFG)
  assert rec.warp_stats == []
  hist = rec.train_warp(ds, num_epochs=epochs, seed=seed, **CFG)
  return rec, hist, _tables_of(rec)


@pytest.fixture(scope="module")
def planted_fit():
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)
  rec, hist, tables = _train_warp(tr, 0, start)
  return tr, ho, start, rec, hist, tables


def test_train_warp_repeats_bit_for_bit_and_finds_fewer_violators(planted_fit):
  tr, _, start, rec, hist, tables = planted_fit
  stats = rec.warp_stats
  assert len(hist) == 5 and rec.warp_history == hist and all(np.isfinite(hist)) and len(stats) == 5
  share, mean_trials = zip(*stats)
  print("loss %s, valid share %s, mean trials %s" % (hist, share, mean_trials))
  assert all(0 < s <= 1 for s in share) and all(t >= 1 for t in mean_trials)
  assert all(a < b for a, b in zip(mean_trials, mean_trials[1:])), mean_trials      # (rises over the epochs)
  assert share[-1] < share[0]
  rec2, hist2, again = _train_warp(tr, 0, start)
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist and rec2.warp_stats == stats
  _, _, other = _train_warp(tr, 1, start)
  assert not np.array_equal(tables[0], other[0]) and not np.array_equal(tables[1], other[1])


def test_held_out_auc_beside_the_float64_restatement(planted_fit):
  """The yardstick is the float64 restatement (same start, lr 0.02, reg 0.01, margin 1, 32 draws, log weights,
  batch 256, 5 epochs, seed 0).  A decision that rounding flips is another legitimate draw, so it cannot cost
  more than a change of seed.  Measured on the CPU over the seeds 0, 1, 2 (start and draws), the float32-numpy
  restatement beside the float64 one: AUC 0.955220 / 0.955220, 0.948884 / 0.948884, 0.950613 / 0.950613 -- gaps
  0, 0, 0 (the tables differ by 4.5e-7 at most; the untrained start is at 0.508) -- and the float64 restatement's
  own spread over those seeds is 0.006336.  The tolerance is the larger of ten times the largest gap (0) and that
  spread: 0.006337."""
  tr, ho, start, rec, hist, tables = planted_fit
  X64, Y64, b64, hist64, stats64 = warp_util.fit(tr, *start, 5, seed=0, **CFG)
  base = bpr_util.auc(*start, tr, ho)
  want, got = bpr_util.auc(X64, Y64, b64, tr, ho), bpr_util.auc(*tables, tr, ho)
  print("held-out AUC: kernels %.6f, float64 restatement %.6f, start %.6f; max table difference %.3g; history %s "
        "beside %s; stats %s beside %s" % (got, want, base, np.abs(tables[0] - X64).max(), hist, hist64,
                                           rec.warp_stats, stats64))
  assert want > 0.9
  assert abs(got - want) <= AUC_TOL
  assert got - base >= 0.5 * (want - base)


def test_train_bpr_with_four_candidates(planted_fit):
  from recoder_amd import bpr, warp
  from recoder_amd.data import RecommendationDataset
  tr, _, start, _, _, _ = planted_fit
  ds = RecommendationDataset(tr)
  kw = dict(batch_size=256, lr=0.05, reg=0.01, seed=0)

  def run(**extra):
    rec = _recoder()
    _start(rec, ds, start, "train_bpr", **kw, **extra)
    hist = rec.train_bpr(ds, num_epochs=2, **kw, **extra)
    return hist, _tables_of(rec)
  hist4, t4 = run(num_candidates=4)
  again_hist, again = run(num_candidates=4)
  assert hist4 == again_hist and all(np.array_equal(a, b) for a, b in zip(t4, again))
  hist1, t1 = run()
  assert hist1 == run(num_candidates=1)[0] and not np.array_equal(t1[1], t4[1])
  # the first step's triples, on exact tables (the arg-max is then an integer fact): the DNS restatement's
  X, Y, b = warp_util.exact_tables(200, 120, 16, 8)
  ws = warp.Workspace(256, 16, DEV)
  bpr.step(_t(X), _t(Y), _t(b), _csr(tr), ws, 0, 0, 0.05, 0.01, num_candidates=4)
  want = warp_util.Sampler(tr).sample(0, 0, 256, X, Y, b, DNS, 32, 4)
  for a, w in zip((ws.users, ws.pos, ws.neg), want[:3]):
    assert np.array_equal(a.cpu().numpy(), w)
  ws1 = bpr.Workspace(256, 16, DEV)
  bpr.sample(_csr(tr), 0, 0, ws1.users, ws1.pos, ws1.neg)
  assert torch.equal(ws1.users, ws.users) and torch.equal(ws1.pos, ws.pos) and not torch.equal(ws1.neg, ws.neg)
  # (the hardest of four is never easier than the first: exact scores, so this holds slot by slot)
  u, j4, j1 = want[0], want[2], ws1.neg.cpu().numpy()
  ok = j1 >= 0
  score = lambda j: (X[u[ok]] * Y[j[ok]]).sum(1) + b[j[ok]]
  assert (j4[ok] >= 0).all() and (score(j4) >= score(j1)).all() and (score(j4) > score(j1)).any()


def test_the_fitted_tables_plug_into_the_rest(planted_fit, tmp_path):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.metrics import Recall
  tr, ho, _, rec, _, tables = planted_fit
  users = np.arange(50)
  inp = UsersInteractions(users, tr[users])
  lists = rec.recommend(inp, 10)
  assert len(lists) == 50 and all(len(l) == 10 for l in lists)
  S = tables[0][:50].astype(np.float64) @ tables[1].astype(np.float64).T + tables[2]
  seen = tr[users].toarray() > 0
  S[seen] = -np.inf
  assert not any(seen[u, l].any() for u, l in enumerate(lists)) and all(len(set(l)) == 10 for l in lists)
  assert np.mean([len(set(l) & set(np.argsort(-S[u])[:10])) for u, l in enumerate(lists)]) >= 8
  res = rec.evaluate(RecommendationDataset(tr, ho), num_recommendations=20, metrics=[Recall(k=20, normalize=True)],
                     batch_size=100)
  assert np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)) > 20.0 / 120       # (better than chance)
  f = rec.save_state(str(tmp_path / "warp"))
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


def test_train_warp_refusals(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, MatrixFactorization
  ds = RecommendationDataset(bpr_util.edge_matrix())
  with pytest.raises(ValueError, match="train_warp trains a MatrixFactorization, not DynamicAutoencoder"):
    Recoder(model=DynamicAutoencoder(hidden_layers=[8])).train_warp(ds)
  with pytest.raises(ValueError, match="train_warp needs activation_type='none'"):
    Recoder(model=MatrixFactorization(8, activation_type="tanh")).train_warp(ds)
  with pytest.raises(ValueError, match="train_warp needs dropout_prob == 0"):
    Recoder(model=MatrixFactorization(8, dropout_prob=0.5)).train_warp(ds)
  with pytest.raises(ValueError, match="train_warp supports embedding sizes 1..512 \\(got 513\\)"):
    Recoder(model=MatrixFactorization(513)).train_warp(ds)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError, match="train_warp runs on one GPU"):
    Recoder(model=MatrixFactorization(8)).train_warp(ds)
