"""The optimiser arithmetic of csrc/optim.hip restated in float64 with a counted rounding bound beside every value:
adam1 (every dense-Adam path: rk_adam_multi, the lazy sweeps) as adam64, sadam1 (rk_adam_rows, the SparseAdam jobs
of rk_adam_multi) as sadam64, the per-step constants of make_consts as consts32, and the fixed-order fp32 sum of
the partial gradients as sum_parts32.  Nothing here is measured: the bounds follow from fp32's unit roundoff and
from the 1-ulp contract the comment above adam1 states for the hardware square root and reciprocal."""
import math

import numpy as np

from tests.encoder_util import U

TINY = 2.0 ** -150                 # half the spacing of fp32's subnormals: the rounding of a result below 2^-126
SQRT_FLUSH = 1.1e-19               # > sqrt(2^-126): what a square root that flushes a subnormal operand loses


class E:
  """A float64 value with a running bound of the distance of the kernel's fp32 value from it: every fp32
  operation adds u times the magnitude of its result to what its operands carry."""

  def __init__(self, v, e=None):
    self.v = np.asarray(v, dtype=np.float64)
    self.e = np.zeros_like(self.v) if e is None else e

  def _rnd(self, v, e):
    return E(v, e + U * (np.abs(v) + e))

  def __add__(self, o):
    return self._rnd(self.v + o.v, self.e + o.e)

  def __sub__(self, o):
    return self._rnd(self.v - o.v, self.e + o.e)

  def __mul__(self, o):
    return self._rnd(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

  def __truediv__(self, o):
    q = self.v / o.v
    return self._rnd(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))

  def sqrt(self):
    return self._rnd(np.sqrt(self.v), np.sqrt(self.v + self.e) - np.sqrt(np.maximum(self.v - self.e, 0.0)))

  # ---- the operations adam1 spells out
  @staticmethod
  def fma(a, b, c):
    """fmaf(a, b, c): the exact a * b + c, ONE rounding.  (adam1's operands reach into the subnormals -- a
    subnormal moment, (1 - beta2) g g of a tiny gradient: below 2^-126 the rounding is absolute, TINY.)"""
    v = a.v * b.v + c.v
    e = np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e
    return E(v, e + U * (np.abs(v) + e) + TINY)

  @staticmethod
  def prod(a, b):
    """a * b where the product may be subnormal: fma(a, b, 0)."""
    return E.fma(a, b, E(np.zeros_like(a.v * b.v)))

  def sqrt_hw(self):
    """The hardware square root, within 1 ulp: E.sqrt's bound and one further ulp (2 u relative), and
    SQRT_FLUSH for an operand in the subnormals that the instruction takes for zero."""
    s = self.sqrt()
    return E(s.v, s.e + 2 * U * (np.abs(s.v) + s.e) + SQRT_FLUSH)

  def rcp_hw(self):
    """The hardware reciprocal, within 1 ulp of the exact quotient: what the operand carries, and 1 ulp."""
    q = 1.0 / self.v
    e = np.abs(q) * self.e / (np.abs(self.v) - self.e)
    return E(q, e + 2 * U * (np.abs(q) + e))


def _const(x, conv_err):
  """A host constant: formed in double, then ONE conversion to fp32.  conv_err: the conversion's error as the
  bound's seed -- the distance of an optimiser that keeps the double (torch.optim.Adam in float64)."""
  c = np.float32(x)
  return E(c, np.asarray(abs(float(c) - float(x))) if conv_err else None)


def consts32(lr, b1, b2, eps, wd, step):
  """The eight floats of make_consts (csrc/optim.hip), in AdamC's order: one_m_b1, b2, one_m_b2, eps, wd,
  inv_bc2_sqrt, neg_step, neg_step_sp -- as doubles, before the conversion."""
  bc1 = 1.0 - b1 ** step
  bc2 = 1.0 - b2 ** step
  return (1.0 - b1, b2, 1.0 - b2, eps, wd, 1.0 / math.sqrt(bc2), -(lr / bc1), -(lr * math.sqrt(bc2) / bc1))


def _as_e(x):
  return x if isinstance(x, E) else E(x)


def adam64(p, m, v, g, lr, b1, b2, eps, wd, step, conv_err=False):
  """adam1 of csrc/optim.hip, operation by operation, in float64 with the bound beside it.  p / m / v: fp32
  arrays (exact) or the E values of the step before (a trajectory carries its bound along); g: the summed
  gradient, exact (sum_parts32).  Returns (p, m, v) as E."""
  one_m_b1, cb2, one_m_b2, ceps, cwd, inv_bc2_sqrt, neg_step, _ = \
      (_const(x, conv_err) for x in consts32(lr, b1, b2, eps, wd, step))
  p, m, v, g = _as_e(p), _as_e(m), _as_e(v), _as_e(g)
  if float(cwd.v) != 0.0:
    g = E.fma(cwd, p, g)
  m = E.fma(one_m_b1, g - m, m)
  v = E.fma(E.prod(one_m_b2, g), g, E.prod(v, cb2))
  denom = E.fma(v.sqrt_hw(), inv_bc2_sqrt, ceps)
  p = E.fma(E.prod(neg_step, m), denom.rcp_hw(), p)
  return p, m, v


def sum_parts32(parts):
  """The gradient of a job with g_parts partial arrays: fp32 adds in strictly ascending part order (the
  kernel's grouped loads do not change the order of its adds), so the sum is the kernel's input bit for bit."""
  parts = [np.asarray(x, dtype=np.float32) for x in parts]
  g = parts[0].copy()
  for x in parts[1:]:
    g = (g + x).astype(np.float32)
  return g


def sadam64(p, m, v, g, lr, b1, b2, eps, step):
  """sadam1 of csrc/optim.hip in float64 with the bound beside it.  The constants as the host forms them:
  doubles, then one conversion to fp32.  A contracted g * g - v (or any other product folded into the add
  behind it) rounds once where this count rounds twice: inside the bound either way."""
  bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
  c1, c2 = E(np.float32(1.0 - b1)), E(np.float32(1.0 - b2))
  ceps, cstep = E(np.float32(eps)), E(np.float32(-(lr * math.sqrt(bc2) / bc1)))
  p, m, v, g = E(p), E(m), E(v), E(g)
  um = (g - m) * c1
  uv = (g * g - v) * c2
  numer = um + m
  dsq = uv + v
  return p + (numer / (dsq.sqrt() + ceps)) * cstep, m + um, v + uv


# ------------------------------------------------------------------ the 25-step trajectory both test modules walk
TRAJ_STEPS, TRAJ_ROWS, TRAJ_H = 25, 64, 64
TRAJ_SCALES = (1e-1, 1e-3, 1e-5)
TRAJ_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def trajectory_inputs(scale, seed=11):
  """p0 ~ 0.3 N(0, 1) as fp32 [TRAJ_ROWS, TRAJ_H] and, per step, (rows, g): the half of the table's rows that carry
  a gradient this step (scrambled: the compact order of a pos map) and their gradient rows g ~ scale N(0, 1); the
  other half takes g = 0.  Moments start at zero."""
  rng = np.random.RandomState(seed)
  p0 = (0.3 * rng.randn(TRAJ_ROWS, TRAJ_H)).astype(np.float32)
  steps = []
  for _ in range(TRAJ_STEPS):
    rows = rng.permutation(TRAJ_ROWS)[:TRAJ_ROWS // 2]
    steps.append((rows, (scale * rng.randn(len(rows), TRAJ_H)).astype(np.float32)))
  return p0, steps


def dense_gradient(rows, g, n_rows=TRAJ_ROWS):
  """The [n_rows, h] gradient that is g[k] in row rows[k] and zero elsewhere."""
  d = np.zeros((n_rows, g.shape[1]), np.float32)
  d[rows] = g
  return d


def trajectory64(scale, wd, conv_err=False):
  """adam64 over the trajectory's steps from fresh moments: the final (p, m, v) as E, the bound carried along."""
  p0, steps = trajectory_inputs(scale)
  p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
  for t, (rows, g) in enumerate(steps):
    p, m, v = adam64(p, m, v, dense_gradient(rows, g), wd=wd, step=t + 1, conv_err=conv_err, **TRAJ_HYPER)
  return p, m, v
