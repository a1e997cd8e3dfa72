"""NeuMF restated in numpy (recoder_amd/ncf.py, csrc/als/ncf.h): the score, the step (forward, loss, every gradient),
Adam for rows and dense parameters, the sampler's draws (tests/bpr_util.py, tests/ultragcn_util.py) and a whole fit, in
float64 -- and the same in float32 (every array and operation in that type), used only to size bounds.

The rule of tests/ials_util.py: a GPU quantity is compared with float64 as max |got - f64| <= bound * max |f64| with
bound = 4 x the float32 restatement's own such error on the same inputs (``bound``), and never below 4 x 2^-24, one
rounding of the result to f32, which a quantity that float32 happens to compute exactly still owes."""
import numpy as np
import scipy.sparse as sp

from tests import bpr_util
from tests.lightgcn_util import BETA1, BETA2, EPS, F32, F64
from tests.ultragcn_util import draws  # noqa: F401  (the negatives are UltraGCN's draws)

SMALL, MID, WIDE = (4, 4, (4,)), (20, 12, (24, 12, 4)), (128, 128, (128,))
# the largest three-layer configuration that fits the LDS among those with dg = dm = 128 and three equal widths
LARGEST_L3 = (128, 128, (76, 76, 76))


def params(sizes, n_users, n_items, seed=0, scale=0.5):
  """Random parameters (f32 values): tables N(0, scale), Xavier-uniform weights, small non-zero biases."""
  dg, dm, layers = sizes
  rng = np.random.RandomState(seed)
  p = {k: (scale * rng.randn(n, d)).astype(F32) for k, n, d in
       (("Pg", n_users, dg), ("Qg", n_items, dg), ("Pm", n_users, dm), ("Qm", n_items, dm))}
  prev, p["W"], p["c"] = 2 * dm, [], []
  for d in layers:
    b = np.sqrt(6.0 / (d + prev))
    p["W"].append(rng.uniform(-b, b, (d, prev)).astype(F32))
    p["c"].append((0.1 * rng.randn(d)).astype(F32))
    prev = d
  p["w"] = rng.uniform(-1, 1, dg + prev).astype(F32)
  p["b0"] = F32(0.05)
  return p


def cast(p, dtype):
  return {k: ([np.asarray(a, dtype) for a in v] if isinstance(v, list) else np.asarray(v, dtype)) for k, v in p.items()}


def theta(p):
  """The dense parameters in the kernels' order [W_1, c_1, ..., w, b0]."""
  parts = []
  for W, c in zip(p["W"], p["c"]):
    parts += [W.reshape(-1), c]
  return np.concatenate(parts + [p["w"], np.reshape(p["b0"], 1)])


def forward(p, u, i):
  """(z, [phi_0 .. phi_L]) of the entries (u[e], i[e]) in the dtype of ``p``."""
  dg = p["Pg"].shape[1]
  phi = [np.concatenate([p["Pm"][u], p["Qm"][i]], axis=1)]
  for W, c in zip(p["W"], p["c"]):
    phi.append(np.maximum(phi[-1] @ W.T + c, 0))
  z = (p["Pg"][u] * p["Qg"][i]) @ p["w"][:dg] + phi[-1] @ p["w"][dg:] + p["b0"]
  return z, phi


def scores(p, users, lo, hi):
  """[B, hi - lo] scores of ``users`` against the items lo .. hi - 1."""
  items = np.arange(lo, hi)
  u = np.repeat(np.asarray(users, np.int64), len(items))
  return forward(p, u, np.tile(items, len(users)))[0].reshape(len(users), len(items))


def scores_blocked(p, users, block=50):
  """``scores`` over the whole catalogue with layer 1 as a sum of a user half and an item half, ``block`` users at a
  time: what a quality run on thousands of users can afford."""
  dg, dm = p["Pg"].shape[1], p["Pm"].shape[1]
  W1 = p["W"][0]
  A = p["Qm"] @ W1[:, dm:].T
  out = []
  for b0 in range(0, len(users), block):
    u = np.asarray(users[b0:b0 + block], np.int64)
    x = np.maximum((p["Pm"][u] @ W1[:, :dm].T + p["c"][0])[:, None, :] + A[None, :, :], 0)
    for W, c in zip(p["W"][1:], p["c"][1:]):
      x = np.maximum(x @ W.T + c, 0)
    out.append((p["Pg"][u] * p["w"][:dg]) @ p["Qg"].T + x @ p["w"][dg:] + p["b0"])
  return np.concatenate(out)


def model_params(model):
  """The restatement's parameters (numpy, the model's dtype) of a ``NeuralMatrixFactorization``."""
  g = lambda t: t.detach().cpu().numpy()
  return {"Pg": g(model.Pg), "Qg": g(model.Qg), "Pm": g(model.Pm), "Qm": g(model.Qm),
          "W": [g(W) for W in model.mlp_weights], "c": [g(c) for c in model.mlp_biases], "w": g(model.w),
          "b0": g(model.b0)[0]}


def start_params(sizes, n_users, n_items, seed):
  """The parameters ``train_ncf`` starts a fresh model of ``sizes`` from under ``seed``."""
  from recoder_amd.nn import NeuralMatrixFactorization
  m = NeuralMatrixFactorization(*sizes)
  m.init_seed = seed
  m.init_model(n_items, n_users)
  return model_params(m)


def entries(users, pos, negs):
  """(u, i, y) of the E = T (1 + R) entries, e = t (1 + R) + c."""
  R = negs.shape[1]
  u = np.repeat(np.asarray(users, np.int64), 1 + R)
  i = np.concatenate([np.asarray(pos, np.int64)[:, None], np.asarray(negs, np.int64)], axis=1).reshape(-1)
  y = np.tile(np.r_[1.0, np.zeros(R)], len(users))
  return u, i, y


def step_grads(p, users, pos, negs):
  """The step's sums, nothing divided by E: {"loss", "GU", "GI" [E, dg + dm], "dtheta" (theta's layout)}."""
  dt = p["w"].dtype
  dg, dm = p["Pg"].shape[1], p["Pm"].shape[1]
  u, i, y = entries(users, pos, negs)
  y = y.astype(dt)
  z, phi = forward(p, u, i)
  e = np.exp(-np.abs(z))
  loss = np.maximum(z, 0) + np.log1p(e) - y * z
  g = (np.where(z >= 0, 1 / (1 + e), e / (1 + e)) - y).astype(dt)
  pq = p["Pg"][u] * p["Qg"][i]
  dw = np.concatenate([(g[:, None] * pq).sum(0), (g[:, None] * phi[-1]).sum(0)])
  dphi = g[:, None] * p["w"][dg:]
  dense = []
  for l in range(len(p["W"]), 0, -1):
    dz = dphi * (phi[l] > 0)
    dense = [(dz.T @ phi[l - 1]).reshape(-1), dz.sum(0)] + dense
    dphi = dz @ p["W"][l - 1]
  GU = np.concatenate([g[:, None] * p["w"][:dg] * p["Qg"][i], dphi[:, :dm]], axis=1)
  GI = np.concatenate([g[:, None] * p["w"][:dg] * p["Pg"][u], dphi[:, dm:]], axis=1)
  return {"loss": loss.sum(), "GU": GU.astype(dt), "GI": GI.astype(dt),
          "dtheta": np.concatenate(dense + [dw, np.reshape(g.sum(), 1)]).astype(dt), "u": u, "i": i}


def loss_only(p, users, pos, negs):
  u, i, y = entries(users, pos, negs)
  z = forward(p, u, i)[0]
  return (np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - y * z).sum()


def weight_mask(sizes):
  """True where theta holds a weight (W_l, w): what the decay reaches."""
  dg, dm, layers = sizes
  prev, parts = 2 * dm, []
  for d in layers:
    parts += [np.ones(d * prev, bool), np.zeros(d, bool)]
    prev = d
  return np.concatenate(parts + [np.ones(dg + prev, bool), np.zeros(1, bool)])


def adam(e, grad, m, v, lr, t):
  """(e, m, v) after Adam step t >= 1 in the dtype of ``e`` (the corrections in float64, as the kernels take them)."""
  dt = e.dtype
  b1, b2 = dt.type(BETA1), dt.type(BETA2)
  step = dt.type(F64(dt.type(lr)) / (1.0 - F64(b1) ** t))
  isb2 = dt.type(1.0 / np.sqrt(1.0 - F64(b2) ** t))
  m = b1 * m + (1 - b1) * grad
  v = b2 * v + ((1 - b2) * grad) * grad
  return e - step * (m / (np.sqrt(v) * isb2 + dt.type(EPS))), m, v


def dense_adam(th, dtheta, E, mask, m, v, lr, reg, t):
  dt = th.dtype
  grad = dtheta * (dt.type(1) / dt.type(E)) + np.where(mask, dt.type(reg) * th, 0).astype(dt)
  return adam(th, grad.astype(dt), m, v, lr, t)


def unpack(p, th):
  """``p`` with its dense parameters taken from ``th``."""
  off, q = 0, dict(p)
  q["W"], q["c"] = [], []
  for W, c in zip(p["W"], p["c"]):
    q["W"].append(th[off:off + W.size].reshape(W.shape)), q["c"].append(th[off + W.size:off + W.size + c.size])
    off += W.size + c.size
  q["w"], q["b0"] = th[off:off + p["w"].size], th[-1]
  return q


def new_state(p, dtype):
  p = cast(p, dtype)
  U, I = np.concatenate([p["Pg"], p["Pm"]], 1), np.concatenate([p["Qg"], p["Qm"]], 1)
  E0 = [U, I, theta(p)]
  return {"E0": E0, "M": [np.zeros_like(e) for e in E0], "V": [np.zeros_like(e) for e in E0], "step": 0, "p": p}


def state_params(state):
  dg = state["p"]["Pg"].shape[1]
  U, I, th = state["E0"]
  q = unpack(state["p"], th)
  q["Pg"], q["Pm"], q["Qg"], q["Qm"] = U[:, :dg], U[:, dg:], I[:, :dg], I[:, dg:]
  return q


def step(state, sizes, users, pos, negs, lr, reg):
  """One step on ``state`` in place; returns the step's loss sum."""
  p = state_params(state)
  dt = p["w"].dtype
  r = step_grads(p, users, pos, negs)
  E = len(r["u"])
  state["step"] += 1
  t = state["step"]
  for side, (key, rows) in enumerate(((r["u"], r["GU"]), (r["i"], r["GI"]))):
    tab = state["E0"][side]
    G, count = np.zeros_like(tab), np.bincount(key, minlength=len(tab)).astype(dt)
    np.add.at(G, key, rows)
    grad = G * (dt.type(1) / dt.type(E)) + (dt.type(reg / E) * count)[:, None] * tab
    state["E0"][side], state["M"][side], state["V"][side] = adam(tab, grad.astype(dt), state["M"][side],
                                                                 state["V"][side], lr, t)
  state["E0"][2], state["M"][2], state["V"][2] = dense_adam(state["E0"][2], r["dtheta"], E, weight_mask(sizes),
                                                             state["M"][2], state["V"][2], lr, reg, t)
  return r["loss"]


def fit(m, p, sizes, num_epochs, batch_size, lr, reg, num_negatives, seed=0, dtype=F64, state=None):
  """(state, the mean loss per entry of each epoch) of ``ncf.fit`` on the CSR ``m`` from the parameters ``p``."""
  m = sp.csr_matrix(m)
  state = new_state(p, dtype) if state is None else state
  sampler = bpr_util.Sampler(m)
  steps = -(-m.nnz // batch_size)
  hist = []
  for _ in range(num_epochs):
    total = 0.0
    for _ in range(steps):
      s = state["step"]
      users, pos, _ = sampler.sample(seed, s, batch_size)
      total += float(step(state, sizes, users, pos, draws(seed, s, batch_size, num_negatives, m.shape[1]), lr, reg))
    hist.append(total / (steps * batch_size * (1 + num_negatives)))
  return state, hist


def rel(got, want):
  want = np.asarray(want, F64)
  return float(np.abs(np.asarray(got, F64) - want).max() / max(np.abs(want).max(), 1e-300))


def bound(f32_value, f64_value):
  """4 x the float32 restatement's error against float64, at least 4 x 2^-24."""
  return 4 * max(rel(f32_value, f64_value), 2.0 ** -24)


def matrix(n_users=37, n_items=53, density=0.15, seed=1):
  rng = np.random.RandomState(seed)
  m = sp.csr_matrix((rng.rand(n_users, n_items) < density).astype(F32))
  m.sort_indices()
  return m
