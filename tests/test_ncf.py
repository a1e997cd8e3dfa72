"""GPU: the rk_als_ncf_* kernels, ncf.fit and the serving of a NeuralMatrixFactorization against the float64 restatement
of tests/ncf_util.py.  Every comparison is max |got - f64| <= bound * max |f64| with bound = 4 x the float32
restatement's own error on the same inputs (``ncf_util.bound``; tests/test_ncf_host.py pins the size of those errors).
37 users x 53 items throughout: neither is a multiple of the 32-row tile."""
import numpy as np
import pytest
import torch

from tests import bpr_util, ncf_util as nu

pytestmark = pytest.mark.gpu
NU, NI = 37, 53
DEV = "cuda"


def _dev(p):
  """(Pg, Qg, Pm, Qm, theta, A-less sizes) of the restatement's parameters on the device."""
  t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
  return t(p["Pg"]), t(p["Qg"]), t(p["Pm"]), t(p["Qm"]), t(nu.theta(p).astype(np.float32))


def _scores(p, sizes, users, lo, hi, ld=None):
  from recoder_amd import ncf
  Pg, Qg, Pm, Qm, th = _dev(p)
  A = ncf.item_part(Qm, th, sizes)
  ld = hi - lo if ld is None else ld
  out = torch.full((len(users), ld), -7.0, dtype=torch.float32, device=DEV)
  ncf.scores(torch.tensor(users, dtype=torch.int32, device=DEV), lo, hi, Pg, Qg, Pm, A, th, sizes, out, ld)
  return out.cpu().numpy(), A.cpu().numpy()


@pytest.mark.parametrize("sizes", [nu.SMALL, nu.MID, nu.WIDE, nu.LARGEST_L3],
                         ids=["small", "mid", "wide", "largest_equal_l3_at_128"])
def test_scores_and_item_part_match_float64(sizes):
  p = nu.params(sizes, NU, NI, 1)
  p64 = nu.cast(p, np.float64)
  everyone = list(range(NU))
  everyone[5] = everyone[20] = 3                               # (repeated ids)
  for users in ([9], everyone):
    for lo, hi, ld in ((0, NI, None), (5, 38, None), (17, 18, None), (5, 38, 40)):
      got, A = _scores(p, sizes, users, lo, hi, ld)
      want, f32 = nu.scores(p64, users, lo, hi), nu.scores(p, users, lo, hi)
      b = nu.bound(f32, want)
      print("scores %r B=%d [%d, %d): %.3g (bound %.3g)" % (sizes, len(users), lo, hi, nu.rel(got[:, :hi - lo], want), b))
      assert nu.rel(got[:, :hi - lo], want) <= b
      assert (got[:, hi - lo:] == -7.0).all()                  # (the padding is not written)
  dm = sizes[1]
  wantA = p64["Qm"] @ p64["W"][0][:, dm:].T
  assert nu.rel(A, wantA) <= nu.bound(p["Qm"] @ p["W"][0][:, dm:].T, wantA)


def test_scores_with_every_first_layer_unit_dead():
  """c_1 far below zero: phi_1 = 0 and the MLP term is w[dg:] . relu(c_2 ...), the same for every pair."""
  p = nu.params(nu.MID, NU, NI, 2)
  p["c"][0] = np.full_like(p["c"][0], -100.0)
  got, _ = _scores(p, nu.MID, list(range(NU)), 0, NI)
  p64 = nu.cast(p, np.float64)
  want = nu.scores(p64, list(range(NU)), 0, NI)
  assert nu.rel(got, want) <= nu.bound(nu.scores(p, list(range(NU)), 0, NI), want)
  tail = np.maximum(p64["W"][2] @ np.maximum(p64["c"][1], 0) + p64["c"][2], 0) @ p64["w"][20:] + p64["b0"]
  gmf = (p64["Pg"] * p64["w"][:20]) @ p64["Qg"].T
  assert np.abs(want - (gmf + tail)).max() <= 1e-12


def test_the_models_cache_is_refreshed_after_a_parameter_write():
  from recoder_amd.nn import NeuralMatrixFactorization
  m = NeuralMatrixFactorization(*nu.MID)
  m.init_model(NI, NU)
  m = m.to(DEV)
  users = torch.arange(NU, device=DEV)
  before = m.user_scores(users, 0, NI).clone()
  assert torch.equal(before, m.user_scores(users, 0, NI))
  m.mlp_weights[0].data.mul_(3.0)
  m._weights_written()
  after = m.user_scores(users, 0, NI)
  assert not torch.equal(before, after)
  p = nu.model_params(m)
  want = nu.scores(nu.cast(p, np.float64), np.arange(NU), 0, NI)
  assert nu.rel(after.cpu().numpy(), want) <= nu.bound(nu.scores(p, np.arange(NU), 0, NI), want)


def _run_step(p, sizes, users, pos, R, seed, step_index):
  from recoder_amd import ncf
  Pg, Qg, Pm, Qm, th = _dev(p)
  ws = ncf.Workspace(NU, NI, len(users), R, sizes, DEV)
  ws.slabs.fill_(float("nan")), ws.GU.fill_(float("nan")), ws.GI.fill_(float("nan"))
  ncf.step_kernel(torch.tensor(users, device=DEV), torch.tensor(pos, device=DEV), R, seed, step_index, Pg, Qg, Pm, Qm,
                  th, sizes, ws.ukey, ws.ikey, ws.GU, ws.GI, ws.slabs)
  return ws, th


@pytest.mark.parametrize("sizes", [nu.SMALL, nu.MID], ids=["small", "mid"])
@pytest.mark.parametrize("T,R", [(5, 3), (64, 1), (65, 4)])
def test_step_matches_float64_and_repeats_its_bits(sizes, T, R):
  p = nu.params(sizes, NU, NI, 3)
  rng = np.random.RandomState(T)
  users, pos = rng.randint(0, NU, T).astype(np.int32), rng.randint(0, NI, T).astype(np.int32)
  users[T // 2:] = users[:T - T // 2]                          # (users and items repeat inside a tile and across tiles)
  pos[-1] = pos[0]
  negs = nu.draws(11, 4, T, R, NI)
  ws, th = _run_step(p, sizes, users, pos, R, 11, 4)
  r64, r32 = nu.step_grads(nu.cast(p, np.float64), users, pos, negs), nu.step_grads(p, users, pos, negs)
  assert np.array_equal(ws.ukey.cpu().numpy(), r64["u"]) and np.array_equal(ws.ikey.cpu().numpy(), r64["i"])
  slabs = ws.slabs.cpu().numpy().astype(np.float64)
  assert np.isfinite(slabs).all()
  got = {"loss": slabs[:, -1].sum(), "dtheta": slabs[:, :-1].sum(0), "GU": ws.GU.cpu().numpy(),
         "GI": ws.GI.cpu().numpy()}
  for k in ("loss", "GU", "GI", "dtheta"):
    b = nu.bound(r32[k], r64[k])
    print("step %r T=%d R=%d %s: %.3g (bound %.3g)" % (sizes, T, R, k, nu.rel(got[k], r64[k]), b))
    assert nu.rel(got[k], r64[k]) <= b, k
  again, _ = _run_step(p, sizes, users, pos, R, 11, 4)
  for a, b in ((ws.slabs, again.slabs), (ws.GU, again.GU), (ws.GI, again.GI)):
    assert torch.equal(a, b)


def test_dense_adam_two_steps_match_float64_and_decay_weights_only():
  from recoder_amd import ncf
  sizes, E = nu.MID, 325
  n, tiles = ncf.layout(sizes)[3], -(-E // ncf.TILE)
  rng = np.random.RandomState(5)
  th0 = nu.theta(nu.params(sizes, 3, 3, 1)).astype(np.float32)
  mask = nu.weight_mask(sizes)
  th = torch.tensor(th0, device=DEV)
  M, V, loss = torch.zeros_like(th), torch.zeros_like(th), torch.zeros(1, device=DEV)
  s64 = [th0.astype(np.float64), np.zeros(n), np.zeros(n)]
  s32 = [th0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)]
  for t in (1, 2):
    slabs = rng.randn(tiles, n + 1).astype(np.float32)
    ncf.dense_adam(th, M, V, torch.tensor(slabs, device=DEV), E, sizes, 0.01, 0.5, t, loss)
    d64 = slabs.astype(np.float64).sum(0)
    s64 = list(nu.dense_adam(s64[0], d64[:-1], E, mask, s64[1], s64[2], 0.01, 0.5, t))
    s32 = list(nu.dense_adam(s32[0], slabs.sum(0, dtype=np.float32)[:-1], E, mask, s32[1], s32[2], 0.01, 0.5, t))
    assert nu.rel(loss.cpu().numpy(), d64[-1:]) <= 4 * max(nu.rel(slabs.sum(0, dtype=np.float32)[-1:], d64[-1:]), 2.0 ** -24)
  for got, a32, a64 in zip((th, M, V), s32, s64):
    assert nu.rel(got.cpu().numpy(), a64) <= nu.bound(a32, a64)
  # a zero gradient moves the weights (the decay) and leaves the biases alone
  th = torch.tensor(th0, device=DEV)
  M, V = torch.zeros_like(th), torch.zeros_like(th)
  ncf.dense_adam(th, M, V, torch.zeros(tiles, n + 1, device=DEV), E, sizes, 0.01, 0.5, 1, loss)
  moved = (th.cpu().numpy() != th0)
  assert not moved[~mask].any() and moved[mask & (th0 != 0)].all()


# ------------------------------------------------------------------ the fit
FIT = dict(num_epochs=3, batch_size=16, lr=0.01, reg=0.01, num_negatives=2, seed=7)


def _dataset(m):
  from recoder_amd.data import RecommendationDataset
  ds = RecommendationDataset.__new__(RecommendationDataset)
  ds.interactions_matrix, ds.users, ds.items = m, np.arange(m.shape[0]), np.arange(m.shape[1])
  return ds


def _recoder():
  from recoder_amd.model import Recoder
  from recoder_amd.nn import NeuralMatrixFactorization
  return Recoder(NeuralMatrixFactorization(*nu.MID), use_cuda=True, user_based=True, num_users=NU, num_items=NI)


@pytest.fixture(scope="module")
def fitted():
  m = nu.matrix()
  rec = _recoder()
  hist = rec.train_ncf(_dataset(m), **FIT)
  return m, rec, hist


_model_params = nu.model_params


def test_a_fit_matches_float64_repeats_its_bits_and_resumes(fitted):
  from recoder_amd.nn import NeuralMatrixFactorization
  m, rec, hist = fitted
  p0 = nu.start_params(nu.MID, NU, NI, FIT["seed"])
  kw = {k: v for k, v in FIT.items() if k != "num_epochs"}
  s64, h64 = nu.fit(m, p0, nu.MID, 3, **kw)
  s32, h32 = nu.fit(m, p0, nu.MID, 3, dtype=np.float32, **kw)
  assert hist == rec.ncf_history and len(hist) == 3
  assert nu.rel(hist, h64) <= nu.bound(h32, h64)
  got = rec.ncf_state
  for k, name in enumerate(("U", "I", "theta")):
    b = nu.bound(s32["E0"][k], s64["E0"][k])
    print("fit %s: %.3g (bound %.3g)" % (name, nu.rel(got[name].cpu().numpy(), s64["E0"][k]), b))
    assert nu.rel(got[name].cpu().numpy(), s64["E0"][k]) <= b
  assert nu.rel(nu.theta(_model_params(rec.model)), got["theta"].cpu().numpy()) == 0
  again = _recoder()
  assert again.train_ncf(_dataset(m), **FIT) == hist
  split = _recoder()
  h2 = split.train_ncf(_dataset(m), **dict(FIT, num_epochs=2))
  h1 = split.train_ncf(_dataset(m), **dict(FIT, num_epochs=1), resume=True)
  assert h2 + h1 == hist
  for other in (again, split):
    for name in ("U", "I", "theta"):
      assert torch.equal(other.ncf_state[name], got[name])
    assert other.ncf_state["step"] == got["step"] == 3 * -(-m.nnz // 16)


def test_serving_after_the_fit(fitted, tmp_path):
  """predict, recommend (held items out, the float64 top-k in order wherever the float64 gaps through rank k + 1 exceed
  twice the score bound: 0.95 of the 37 users at seed 7, at least 0.9 asked), a forced strip width, an id out of range
  and a checkpoint round trip."""
  from recoder_amd.data import UsersInteractions
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import NeuralMatrixFactorization
  m, rec, _ = fitted
  users = np.arange(NU)
  ui = UsersInteractions(users=users, interactions_matrix=m)
  scores = rec.predict(ui)[0].cpu().numpy()
  direct = rec.model.user_scores(torch.tensor(users, device=DEV), 0, NI).cpu().numpy()
  assert np.array_equal(scores, direct)
  p64 = nu.cast(_model_params(rec.model), np.float64)
  want = nu.scores(p64, users, 0, NI)
  b = nu.bound(nu.scores(nu.cast(p64, np.float32), users, 0, NI), want) * np.abs(want).max()
  assert np.abs(scores - want).max() <= b
  k = 5
  ids = rec.recommend_array(ui, k)
  dense = np.asarray(m.todense()) > 0
  assert not dense[np.arange(NU)[:, None], ids].any()          # (held items are excluded)
  masked = np.where(dense, -np.inf, want)
  order = np.argsort(-masked, axis=1, kind="stable")
  top = np.take_along_axis(masked, order, 1)
  clear = (top[:, :k] - top[:, 1:k + 1]).min(1) > 2 * b
  print("users with clear float64 gaps through rank %d: %.2f" % (k, clear.mean()))
  assert clear.mean() >= 0.9
  assert np.array_equal(ids[clear], order[clear, :k])
  rec.eval_strip_items = 16
  try:
    assert np.array_equal(rec.recommend_array(ui, k), ids)
  finally:
    del rec.eval_strip_items
  with pytest.raises(ValueError, match="user ids must lie in"):
    rec.recommend_array(UsersInteractions(users=np.array([NU]), interactions_matrix=m[:1]), k)
  path = rec.save_state(str(tmp_path / "ncf"))
  fresh = Recoder(NeuralMatrixFactorization(), use_cuda=True, user_based=True)
  fresh.init_from_model_file(path)
  assert fresh.model.sizes() == nu.MID and np.array_equal(fresh.recommend_array(ui, k), ids)


def _held_out(m, seed=3):
  """A target matrix: three items a user that the user does not hold."""
  rng = np.random.RandomState(seed)
  dense = np.asarray(m.todense()) > 0
  t = np.zeros(dense.shape, np.float32)
  for u in range(dense.shape[0]):
    t[u, rng.choice(np.flatnonzero(~dense[u]), 3, replace=False)] = 1.0
  import scipy.sparse as sp
  return sp.csr_matrix(t)


def test_evaluate_on_the_device_equals_the_host_metrics(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  m, rec, _ = fitted
  ds = RecommendationDataset(m, _held_out(m))
  metrics = [Recall(k=5, normalize=True), NDCG(k=10)]
  torch.manual_seed(5)                                       # (the evaluator walks a random order drawn from torch's
  host = rec.evaluate(ds, num_recommendations=10, metrics=metrics, batch_size=16)
  torch.manual_seed(5)                                       #  global generator: the same order for both)
  dev = rec.evaluate(ds, num_recommendations=10, metrics=metrics, batch_size=16, on_device=True)
  assert len(host) == len(dev) == 2
  for a, b in zip(host.values(), dev.values()):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and len(a) and np.abs(a - b).max() <= 1e-12 and a.max() > 0


def test_a_validated_fit_records_a_metric_per_epoch_and_can_stop_early(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import Recall
  m, rec, hist = fitted
  val = RecommendationDataset(m, _held_out(m))
  kw = dict(val_dataset=val, eval_metric=Recall(k=5, normalize=True), eval_batch_size=16)
  watched = _recoder()
  h = watched.train_ncf(_dataset(m), **FIT, restore_best=False, **kw)
  v = watched.ncf_validation
  assert h == hist                                             # (validation touches neither draws nor arithmetic)
  assert v["epochs"] == [1, 2, 3] and len(v["values"]) == 3 and all(np.isfinite(v["values"]))
  assert v["metric"] == "Recall@5" or "Recall" in v["metric"]
  for name in ("U", "I", "theta"):
    assert torch.equal(watched.ncf_state[name], rec.ncf_state[name])
  # the last value is the metric of the model the fit leaves
  res = watched.evaluate(val, num_recommendations=5, metrics=[Recall(k=5, normalize=True)], batch_size=16,
                         on_device=True)
  assert abs(float(np.nanmean(list(res.values())[0])) - v["values"][-1]) <= 1e-12
  # patience 1 on a metric that cannot improve (no target is ever hit: an empty target matrix gives nan, never a best;
  # so a constant target of held items, which recommend never returns, gives 0 every epoch): stops after two evaluations
  stop = _recoder()
  never = RecommendationDataset(m, m)
  h = stop.train_ncf(_dataset(m), **dict(FIT, num_epochs=6), val_dataset=never, eval_metric=Recall(k=5, normalize=True),
                     eval_batch_size=16, patience=1, restore_best=True)
  v = stop.ncf_validation
  assert v["values"] == [0.0, 0.0] and v["stopped_epoch"] == 2 and len(h) == 2 and v["best_epoch"] == 1
  # restore_best put the first epoch's state back: a fit of one epoch, bit for bit, step count included
  one = _recoder()
  one.train_ncf(_dataset(m), **dict(FIT, num_epochs=1))
  for name in ("U", "I", "theta"):
    assert torch.equal(stop.ncf_state[name], one.ncf_state[name])
  assert stop.ncf_state["step"] == one.ncf_state["step"]
  assert torch.equal(stop.model.user_scores(torch.arange(NU, device=DEV), 0, NI),
                     one.model.user_scores(torch.arange(NU, device=DEV), 0, NI))
