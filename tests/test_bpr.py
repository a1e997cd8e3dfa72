"""GPU: the BPR step (recoder_amd/bpr.py, the rk_als_bpr_* kernels of librecoder_als.so) against the
restatement of tests/bpr_util.py -- the sampler bit for bit, grad and apply against float64 within the
rounding of their own f32 chains, one whole step, and Recoder.train_bpr end to end with what the fitted
tables plug into."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import bpr_util

pytestmark = pytest.mark.gpu

DEV = "cuda"
U23 = 2.0 ** -23
LR, REG = float(np.float32(0.05)), float(np.float32(0.02))     # (f32 values: the kernels take floats)


def _t(a, dtype=np.float32):
  return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _csr(m):
  from recoder_amd import bpr
  return bpr.user_csr(m, m.shape[0], m.shape[1], DEV)


def _wide_matrix():
  """200 users x 120 items at density 0.1, users 0 and 9 empty."""
  rng = np.random.RandomState(4)
  m = (rng.rand(200, 120) < 0.1).astype(np.float32)
  m[0, :] = 0
  m[9, :] = 0
  m = sp.csr_matrix(m)
  m.sort_indices()
  return m


def _tables(n_users, n_items, h, seed, scale=0.5):
  rng = np.random.RandomState(seed)
  return ((scale * rng.randn(n_users, h)).astype(np.float32), (scale * rng.randn(n_items, h)).astype(np.float32),
          (scale * rng.randn(n_items)).astype(np.float32))


# ------------------------------------------------------------------ sampler
@pytest.mark.parametrize("seed", [0, -(2 ** 40) - 3])
@pytest.mark.parametrize("step", [0, 7])
def test_sampler_is_bitwise_the_restatement(seed, step):
  from recoder_amd import bpr
  m = bpr_util.edge_matrix()
  T = 257
  users, pos, neg = (torch.full((T,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
  bpr.sample(_csr(m), seed, step, users, pos, neg)
  wu, wp, wn = bpr_util.sample(m, seed, step, T)
  assert (wn[wu == 5] == -1).all() and (wu == 5).any() and (wu == 3).any() and not (wu == 7).any()
  assert np.array_equal(users.cpu().numpy(), wu)
  assert np.array_equal(pos.cpu().numpy(), wp)
  assert np.array_equal(neg.cpu().numpy(), wn)


# --------------------------------------------------------------------- grad
def _grad_bounds(users, pos, neg, X, Y, b):
  """The float64 x, g, loss and the bound on |x_hat - x| for the f32 inputs."""
  h = X.shape[1]
  x, g, loss, D, P = bpr_util.grad(users, pos, neg, X, Y, b)
  ok = neg >= 0
  mag = np.zeros(len(users))
  b64 = b.astype(np.float64)
  mag[ok] = (np.abs(P[ok]) * np.abs(D[ok])).sum(1) + np.abs(b64[pos[ok]]) + np.abs(b64[neg[ok]])
  return x, g, loss, (h + 4) * U23 * mag


@pytest.mark.parametrize("h", [1, 64, 65, 512])
def test_grad_against_float64(h):
  from recoder_amd import bpr
  m = bpr_util.edge_matrix()
  T = 130
  users, pos, neg = bpr_util.sample(m, 3, 2, T)
  assert (neg < 0).any() and (neg >= 0).sum() > 60
  X, Y, b = _tables(37, 53, h, h)
  g, loss, xs = (torch.full((T,), 7.0, device=DEV) for _ in range(3))
  D, P = (torch.full((T, h), 7.0, device=DEV) for _ in range(2))
  bpr.grad(_t(users, np.int32), _t(pos, np.int32), _t(neg, np.int32), _t(X), _t(Y), _t(b), g, loss, D, P, x=xs)
  g, loss, xs, D, P = (v.cpu().numpy() for v in (g, loss, xs, D, P))
  ok = neg >= 0
  x64, g64, loss64, xb = _grad_bounds(users, pos, neg, X, Y, b)
  ex, eg = np.abs(xs - x64), np.abs(g - g64)
  print("h %d: max |x^ - x| / bound %.3f, max |g^ - g| / bound %.3f"
        % (h, (ex[ok] / xb[ok]).max(), (eg[ok] / (xb[ok] / 4 + 4 * 2.0 ** -24)).max()))
  assert np.all(ex <= xb)
  assert np.all(eg <= xb / 4 + 4 * 2.0 ** -24)
  # |softplus'| <= 1; max(-x, 0) is exact, log1p(e) <= ln 2 and the sum round within a few ulps of the loss
  assert np.all(np.abs(loss - loss64) <= xb + 4 * 2.0 ** -24 * np.maximum(1.0, loss64))
  wantD, wantP = np.zeros((T, h), np.float32), np.zeros((T, h), np.float32)
  wantD[ok], wantP[ok] = Y[pos[ok]] - Y[neg[ok]], X[users[ok]]
  assert np.array_equal(D, wantD) and np.array_equal(P, wantP)
  for v in (g, loss, xs):
    assert np.all(v[~ok] == 0) and not np.signbit(v[~ok]).any()


# -------------------------------------------------------------------- apply
def _apply_gpu(users, pos, neg, g, D, P, X, Y, b, lr, reg):
  from recoder_amd import bpr
  Xt, Yt, bt = _t(X), _t(Y), _t(b)
  (uk, uo), (ik, io) = bpr.sorted_keys(_t(users, np.int32), _t(pos, np.int32), _t(neg, np.int32), X.shape[0], Y.shape[0])
  gt = _t(g)
  bpr.apply(uk, uo, 1, gt, _t(D), lr, reg, Xt)
  bpr.apply(ik, io, 2, gt, _t(P), lr, reg, Yt, bt)
  return Xt.cpu().numpy(), Yt.cpu().numpy(), bt.cpu().numpy()


def _apply_bounds(users, pos, neg, g, D, P, X, Y, b, lr, reg, extra=None):
  """Per element (c + 4) 2^-23 (|old| + lr sum |g_t d_tk| + lr reg c |old|) for the three outputs; ``extra``
  [T]: a bound on |g_hat - g| whose effect lr sum extra_t |d_tk| is added (the composed step)."""
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  g64, D64, P64 = np.abs(g.astype(np.float64))[ok], np.abs(D.astype(np.float64))[ok], np.abs(P.astype(np.float64))[ok]
  e64 = np.zeros_like(g64) if extra is None else extra[ok]
  out = []
  for old, rows, vecs in ((X, (u,), D64), (Y, (i, j), P64), (b, (i, j), None)):
    old = np.abs(old.astype(np.float64))
    s, se, c = np.zeros_like(old), np.zeros_like(old), np.zeros(len(old))
    for r in rows:
      np.add.at(s, r, g64[:, None] * vecs if vecs is not None else g64)
      np.add.at(se, r, e64[:, None] * vecs if vecs is not None else e64)
      c += np.bincount(r, minlength=len(old))
    cc = c[:, None] if old.ndim == 2 else c
    out.append((cc + 4) * U23 * (old + lr * s + lr * reg * cc * old) + lr * se)
  return out


def _colliding_triples(n_users, n_items, T, seed):
  """Triples drawn freely (not from a matrix): every row collides, items appear in both roles, some slots invalid."""
  rng = np.random.RandomState(seed)
  users = rng.randint(0, n_users, T).astype(np.int32)
  pos = rng.randint(0, n_items, T).astype(np.int32)
  neg = ((pos + 1 + rng.randint(0, n_items - 1, T)) % n_items).astype(np.int32)
  neg[rng.rand(T) < 0.1] = -1
  return users, pos, neg


@pytest.mark.parametrize("shape", [(3, 5, 64, 7), (200, 120, 256, 65), (200, 120, 256, 300)])
def test_apply_alone_against_float64(shape):
  n_users, n_items, T, h = shape
  users, pos, neg = _colliding_triples(n_users, n_items, T, T + h)
  if n_users == 3:
    assert set(pos[neg >= 0]) & set(neg[neg >= 0]) and np.bincount(users).min() > 8
  rng = np.random.RandomState(h)
  X, Y, b = _tables(n_users, n_items, h, 1)
  g = rng.rand(T).astype(np.float32)
  D, P = rng.randn(T, h).astype(np.float32), rng.randn(T, h).astype(np.float32)
  got = _apply_gpu(users, pos, neg, g, D, P, X, Y, b, LR, REG)
  again = _apply_gpu(users, pos, neg, g, D, P, X, Y, b, LR, REG)
  want = bpr_util.apply(users, pos, neg, g, D, P, X, Y, b, LR, REG)
  bounds = _apply_bounds(users, pos, neg, g, D, P, X, Y, b, LR, REG)
  ok = neg >= 0
  touched = (np.isin(np.arange(n_users), users[ok]), np.isin(np.arange(n_items), np.r_[pos[ok], neg[ok]]),
             np.isin(np.arange(n_items), np.r_[pos[ok], neg[ok]]))
  for name, a, a2, w, bd, old, tch in zip("XYb", got, again, want, bounds, (X, Y, b), touched):
    err = np.abs(a - w)
    print("%s %s: max err / bound %.3f" % (shape, name, (err / np.maximum(bd, 1e-300)).max()))
    assert np.all(err <= bd), name
    assert np.array_equal(a, a2), "not bitwise repeatable: " + name
    assert np.array_equal(a[~tch], old[~tch]), "an untouched row changed: " + name
    assert not np.array_equal(a[tch], old[tch])
  if n_users == 200:
    assert (~touched[0]).any()


# ---------------------------------------------------------------- one step
def test_one_full_step_against_the_restatement_on_the_same_triples():
  from recoder_amd import bpr
  m = _wide_matrix()
  h, T = 24, 256
  X, Y, b = _tables(200, 120, h, 5, scale=0.3)
  Xt, Yt, bt = _t(X), _t(Y), _t(b)
  ws = bpr.Workspace(T, h, DEV)
  bpr.step(Xt, Yt, bt, _csr(m), ws, 11, 3, LR, REG)
  users, pos, neg = (v.cpu().numpy() for v in (ws.users, ws.pos, ws.neg))
  wu, wp, wn = bpr_util.sample(m, 11, 3, T)
  assert np.array_equal(users, wu) and np.array_equal(pos, wp) and np.array_equal(neg, wn)
  _, g64, _, D64, P64 = bpr_util.grad(users, pos, neg, X, Y, b)
  want = bpr_util.apply(users, pos, neg, g64, D64, P64, X, Y, b, LR, REG)
  # composed: the apply's own chain on the kernel's g, plus what the bound on |g_hat - g| lets through
  _, _, _, xb = _grad_bounds(users, pos, neg, X, Y, b)
  gb = xb / 4 + 4 * 2.0 ** -24
  bounds = _apply_bounds(users, pos, neg, (g64 + gb).astype(np.float32), D64, P64, X, Y, b, LR, REG, extra=gb)
  for name, a, w, bd in zip("XYb", (Xt, Yt, bt), want, bounds):
    err = np.abs(a.cpu().numpy() - w)
    print("step %s: max err / bound %.3f" % (name, (err / np.maximum(bd, 1e-300)).max()))
    assert np.all(err <= bd), name
  assert np.array_equal(Xt[0].cpu().numpy(), X[0]) and np.array_equal(Xt[9].cpu().numpy(), X[9])


# -------------------------------------------------------------- end to end
def _recoder(h=16):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  return Recoder(model=MatrixFactorization(h), loss="mse", optimizer_type="adam")


def _train(tr, seed, start, epochs=5):
  """train_bpr on the planted matrix from the tables ``start`` (set after an empty fit has built the model)."""
  from recoder_amd.data import RecommendationDataset
  rec = _recoder()
  ds = RecommendationDataset(tr)
  assert rec.train_bpr(ds, num_epochs=0, batch_size=256, lr=0.05, reg=0.01, seed=seed) == []
  m = rec.model
  for p, a in zip((m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias), start):
    p.data.copy_(_t(a))
  hist = rec.train_bpr(ds, num_epochs=epochs, batch_size=256, lr=0.05, reg=0.01, seed=seed)
  return rec, hist, tuple(p.detach().cpu().numpy() for p in
                          (m.user_embedding_layer.weight, m.item_embedding_layer.weight, m.bias))


@pytest.fixture(scope="module")
def planted_fit():
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, 0)
  rec, hist, tables = _train(tr, 0, start)
  return tr, ho, start, rec, hist, tables


def test_train_bpr_lowers_the_loss_and_repeats_bit_for_bit(planted_fit):
  tr, _, start, rec, hist, tables = planted_fit
  assert len(hist) == 5 and rec.bpr_history == hist and all(np.isfinite(hist))
  assert all(v < hist[0] for v in hist[1:]), hist
  _, hist2, again = _train(tr, 0, start)
  assert all(np.array_equal(a, b) for a, b in zip(tables, again)) and hist2 == hist
  _, _, other = _train(tr, 1, start)
  assert not np.array_equal(tables[0], other[0]) and not np.array_equal(tables[1], other[1])


def test_held_out_auc_beside_the_float64_restatement(planted_fit):
  """The yardstick is the float64 restatement trained on the same triples (same start, lr 0.05, reg 0.01,
  batch 256, 5 epochs, seed 0).  Measured on the CPU, the f32-numpy restatement beside the float64 one
  over the seeds 0, 1, 2 (start and draws): AUC 0.784434 / 0.784434, 0.784387 / 0.784387, 0.780582 /
  0.780582 -- gaps 0, 0, 0 (the tables differ by 1.4e-7 at most and no pair of scores changes order; the
  untrained start is at 0.508).  Ten times the largest gap measured is therefore 0: the held-out AUC has
  to equal the restatement's."""
  tr, ho, start, _, hist, tables = planted_fit
  X64, Y64, b64, hist64 = bpr_util.fit(tr, *start, 5, 256, 0.05, 0.01, seed=0)
  want, got = bpr_util.auc(X64, Y64, b64, tr, ho), bpr_util.auc(*tables, tr, ho)
  print("held-out AUC: kernels %.6f, float64 restatement %.6f, start %.6f; max table difference %.3g; "
        "history %s beside %s" % (got, want, bpr_util.auc(*start, tr, ho), np.abs(tables[0] - X64).max(), hist, hist64))
  assert want > 0.7
  assert abs(got - want) <= 10 * 0.0


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
  # the lists are the top of the tables' scores (the serving path may round the scores: not item for item)
  assert np.mean([len(set(l) & set(np.argsort(-S[u])[:10])) for u, l in enumerate(lists)]) >= 8
  res = rec.evaluate(RecommendationDataset(tr, ho), num_recommendations=20, metrics=[Recall(k=20, normalize=True)],
                     batch_size=100)
  assert np.nanmean(np.asarray(list(res.values())[0], dtype=np.float64)) > 20.0 / 120       # (better than chance)
  f = rec.save_state(str(tmp_path / "bpr"))
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


# ------------------------------------------------------------------ refusals
def test_train_bpr_refusals(monkeypatch):
  import torch.distributed as dist
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, MatrixFactorization
  ds = RecommendationDataset(bpr_util.edge_matrix())
  with pytest.raises(ValueError, match="train_bpr trains a MatrixFactorization, not DynamicAutoencoder"):
    Recoder(model=DynamicAutoencoder(hidden_layers=[8])).train_bpr(ds)
  with pytest.raises(ValueError, match="train_bpr needs activation_type='none'"):
    Recoder(model=MatrixFactorization(8, activation_type="tanh")).train_bpr(ds)
  with pytest.raises(ValueError, match="train_bpr supports embedding sizes 1..512 \\(got 513\\)"):
    Recoder(model=MatrixFactorization(513)).train_bpr(ds)
  monkeypatch.setattr(dist, "is_available", lambda: True)
  monkeypatch.setattr(dist, "is_initialized", lambda: True)
  monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
  with pytest.raises(NotImplementedError, match="train_bpr runs on one GPU"):
    Recoder(model=MatrixFactorization(8)).train_bpr(ds)
