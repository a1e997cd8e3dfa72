"""tests/linear_util.py held to torch.autograd in float64, and its case generators held to what they are named
for.  No GPU."""
import numpy as np
import pytest
import torch

from tests import linear_util as lu
from tests.encoder_util import ACT_ELU, ACT_NONE, ACT_RELU, ACT_SELU, ACT_SIGMOID, ACT_TANH, ACTS, U

TORCH_ACT = {ACT_NONE: lambda x: x, ACT_TANH: torch.tanh, ACT_SIGMOID: torch.sigmoid, ACT_RELU: torch.relu,
             ACT_SELU: torch.selu, ACT_ELU: torch.nn.functional.elu}


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("act", ACTS)
def test_restatement_is_autograd_in_float64(act, wt, acc):
  B, N, K = 7, 5, 9
  rng = np.random.RandomState(act * 4 + wt * 2 + acc)
  X, Wn, b, dY, dW0n, Xpre = (rng.randn(*s) for s in ((B, K), (N, K), (N,), (B, N), (N, K), (B, K)))
  W, dW0 = (Wn.T.copy(), dW0n.T.copy()) if wt else (Wn, dW0n)
  # the layer's input is itself an activation's output: X = act(Xpre), so that dX * act'(X) has an autograd twin
  Xp = torch.tensor(Xpre, requires_grad=True)
  Xt = TORCH_ACT[act](Xp)
  Wt, bt = torch.tensor(Wn, requires_grad=True), torch.tensor(b, requires_grad=True)
  Xl = Xt.detach().clone().requires_grad_(True)
  out = TORCH_ACT[act](Xl @ Wt.t() + bt)
  out.backward(torch.tensor(dY))
  X = Xl.detach().numpy()

  pre, Y, S = lu.linear_fwd64(X, W, b, wt, act)
  assert np.allclose(Y, out.detach().numpy(), rtol=1e-13, atol=1e-13)
  assert np.allclose(pre, X @ Wn.T + b, rtol=1e-13, atol=1e-13) and np.all(S >= np.abs(pre) - 1e-12)

  dYpre, dX, dW, db, SX, SW, Sb = lu.linear_bwd64(dY, Y, X, W, wt, act, dW0 if acc else None)
  want_dW = Wt.grad.numpy() + (dW0n if acc else 0.0)
  assert np.allclose(dX, Xl.grad.numpy(), rtol=1e-11, atol=1e-12)
  assert np.allclose(dW.T if wt else dW, want_dW, rtol=1e-11, atol=1e-12)
  assert np.allclose(db, bt.grad.numpy(), rtol=1e-11, atol=1e-12)
  assert np.all(SX >= np.abs(dX) - 1e-12) and np.all(Sb >= np.abs(db) - 1e-12) and np.all(SW >= np.abs(dW) - 1e-12)
  # rk_linear_bwd_pre's form (dY already is dYpre) and rk_linear_bwd_dact's factor on dX
  _, dX2, dW2, db2, _, _, _ = lu.linear_bwd64(dYpre, None, X, W, wt, act, dW0 if acc else None, dx_act_y=X)
  Xt.backward(torch.tensor(dX))
  assert np.allclose(dX2, Xp.grad.numpy(), rtol=1e-11, atol=1e-12)
  assert np.array_equal(dW2, dW) and np.array_equal(db2, db)


@pytest.mark.parametrize("act", ACTS)
def test_act_dy_of_the_output_is_autograds_derivative(act):
  rng = np.random.RandomState(act)
  x = np.concatenate([rng.randn(200) * 3, [1e-3, -1e-3, 5.0, -5.0, 12.0, -12.0]])
  xt = torch.tensor(x, requires_grad=True)
  TORCH_ACT[act](xt).sum().backward()
  got = lu.act_dy64(lu.act64(x, act), act)
  assert np.allclose(got, xt.grad.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("act", ACTS)
def test_act_dy_err_covers_the_fp32_formulas(act):
  """rk_act_dy's operations restated in numpy float32 stay inside the counted bound, at random outputs and at the edges."""
  rng = np.random.RandomState(act + 10)
  y = np.concatenate([lu.outputs_of(act, rng, (4000,)), lu.bwd_specials(act)]).astype(np.float32)
  one, s, a = np.float32(1), np.float32(lu.SELU_S), np.float32(lu.SELU_A)
  d32 = {ACT_NONE: lambda: np.ones_like(y), ACT_TANH: lambda: one - y * y, ACT_SIGMOID: lambda: (one - y) * y,
         ACT_RELU: lambda: np.where(y > 0, one, np.float32(0)), ACT_ELU: lambda: np.where(y > 0, one, y + one),
         ACT_SELU: lambda: np.where(y > 0, s, y + s * a)}[act]()
  assert d32.dtype == np.float32
  err = np.abs(d32.astype(np.float64) - lu.act_dy64(y, act))
  assert np.all(err <= lu.act_dy_err(y, act))
  dY = lu.log_uniform(rng, y.shape)
  err = np.abs((dY * d32).astype(np.float64) - dY.astype(np.float64) * lu.act_dy64(y, act))
  assert np.all(err <= lu.dypre_bound(dY, y, act))


def test_small_fits_and_route_at_the_limits():
  assert lu.small_fits(1, 1024, 4096) and not lu.small_fits(1, 1025, 1) and not lu.small_fits(1, 1, 4097)
  assert lu.small_fits(4096, 1024, 4) and not lu.small_fits(4097, 1024, 4) and not lu.small_fits(0, 1, 1)
  assert lu.route(500, 200, 200, 0) == {"fwd": ("small", 0, 0), "dx": ("small", 0, 1), "dw": ("small", 1, 1)}
  assert lu.route(500, 200, 200, 1) == {"fwd": ("small", 0, 1), "dx": ("small", 0, 0), "dw": ("small", 1, 1)}
  # the backward permutes the roles: K is dX's N, N its reduction; B is dW's reduction
  assert lu.route(33, 1100, 40, 0)["fwd"][0] == "gemm" and lu.route(33, 1100, 40, 0)["dx"][0] == "small"
  assert lu.route(33, 40, 1100, 1)["fwd"][0] == "small" and lu.route(33, 40, 1100, 1)["dw"][0] == "gemm"
  assert lu.route(5000, 8, 8, 0)["fwd"][0] == "small" and lu.route(5000, 8, 8, 0)["dx"][0] == "gemm"


def test_generators_reach_what_they_are_named_for():
  cov = lu.covering_cases()
  assert len(cov) == 3 * len(lu.REDUCTIONS) + 8
  assert len(lu.seam_cases()) == 10
  assert len(lu.fallback_cases()) == 27
  assert len(lu.real_cases()) == 12
  lu.check_reduction_cases()


def test_integer_cases_stay_exact_in_fp32():
  """The largest sum of absolute products over every integer case, taken on the operands themselves where that is
  cheap and by its analytic bound everywhere, is below 2^24: every partial sum is an integer fp32 holds."""
  worst = 0
  for B, N, K, _ in lu.covering_cases():
    for wt in (0, 1):
      o = lu.int_operands(B, N, K, wt, seed=B * 7 + N * 3 + K)
      _, _, S = lu.linear_fwd64(o["X"], o["W"], o["b"], wt, ACT_NONE)
      _, _, _, _, SX, SW, Sb = lu.linear_bwd64(o["dY"], o["Y"], o["X"], o["W"], wt, ACT_NONE, o["dW0"])
      m = max(S.max(), SX.max(), SW.max(), Sb.max())
      assert m <= lu.int_sum_bound(B, N, K)
      worst = max(worst, m)
  for _, _, B, N, K, top in lu.seam_cases():
    worst = max(worst, lu.int_sum_bound(B, N, K, top))
  for _, B, N, K, _ in lu.fallback_cases():
    worst = max(worst, lu.int_sum_bound(B, N, K))
  for rows in lu.AGC_ROWS + lu.SGC_ROWS + lu.CS_ROWS:
    worst = max(worst, rows * 8)
  assert worst < 2 ** 24, worst


def test_real_operands_hold_no_subnormals_and_legal_outputs():
  for act in ACTS:
    o = lu.real_operands(40, 30, 20, 0, act, seed=act)
    for k, v in o.items():
      assert v.dtype == np.float32 and np.all(np.abs(v) >= 2.0 ** -20), k
    y = o["Y"].astype(np.float64)
    lo, hi = {ACT_TANH: (-1, 1), ACT_SIGMOID: (0, 1), ACT_SELU: (-lu.SELU_S * lu.SELU_A, np.inf),
              ACT_ELU: (-1, np.inf)}.get(act, (-np.inf, np.inf))
    assert np.all(y > lo) and np.all(y < hi)
    assert np.all(np.abs(lu.act_dy64(y, act)) >= 2.0 ** -30) or act == ACT_RELU      # no subnormal dYpre either
  assert lu.gamma(8) > 8 * U
