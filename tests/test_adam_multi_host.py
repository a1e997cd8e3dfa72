"""CPU: what stands behind tests/test_adam_multi.py without a GPU.

* tests/adam_util.adam64 -- the float64 restatement of adam1 (csrc/optim.hip) the GPU tests hold rk_adam_multi
  to -- against torch.optim.Adam in float64: the two differ by the constants' one conversion to fp32 and by
  nothing else, and the bound adam64 carries covers that when the conversion error seeds it.
* that bound stays below the project's own parameter tolerance (tight_stats of tests/test_hip_parity.py), element
  by element: a GPU test that asserts |kernel - adam64| <= bound asserts something.
* rk_adam_consts (a host function) returns the restatement's eight floats bit for bit.
* the argument checks of rk_adam_multi / rk_adam_lazy_flush that return before any launch.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import adam_util as au

LR, B1, B2, EPS = (au.TRAJ_HYPER[k] for k in ("lr", "b1", "b2", "eps"))


@pytest.fixture(scope="module")
def lib():
  from recoder_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    from recoder_amd.build import build_library
    build_library(verbose=False)
  return _lib.load()


# ------------------------------------------------------------------ the restatement against torch.optim.Adam
@pytest.mark.parametrize("wd", [0.0, 2e-5])
@pytest.mark.parametrize("scale", au.TRAJ_SCALES)
def test_adam64_is_torch_adam_up_to_the_fp32_constants(scale, wd):
  p0, steps = au.trajectory_inputs(scale)
  w = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
  opt = torch.optim.Adam([w], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
  p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
  for t, (rows, g) in enumerate(steps):
    gd = au.dense_gradient(rows, g)
    w.grad = torch.from_numpy(gd.astype(np.float64))
    opt.step()
    p, m, v = au.adam64(p, m, v, gd, wd=wd, step=t + 1, conv_err=True, **au.TRAJ_HYPER)
    # every step: torch's parameter inside the bound carried so far
    err = np.abs(w.detach().numpy() - p.v)
    assert np.all(err <= p.e), (t, float((err - p.e).max()))
  st = opt.state[w]
  for name, r, x in (("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
    err = np.abs(x.numpy() - r.v)
    assert np.all(err <= r.e), (name, float((err - r.e).max()))
  # the restatement moved: the comparison is not between two copies of p0
  assert np.abs(p.v - p0).max() > 1e-3
  # The bound is not vacuous: below the project's parameter tolerance (tight_stats: 2e-7 + 1e-5 |p|) for EVERY
  # element, with the constants' conversion error in it and, a fortiori, without (what the GPU tests assert)
  lim = 2e-7 + 1e-5 * np.abs(p.v)
  assert np.all(p.e < lim), float((p.e / lim).max())
  assert float(p.e.max()) <= 1.9e-6
  pk, mk, vk = au.trajectory64(scale, wd)
  for a, b in ((pk, p), (mk, m), (vk, v)):
    assert np.array_equal(a.v, b.v) and np.all(a.e <= b.e)
  print("adam64 vs torch, scale %g wd %g: largest bound on p %.3e, largest bound / (2e-7 + 1e-5 |p|) %.3f"
        % (scale, wd, float(p.e.max()), float((p.e / lim).max())))


def test_sum_parts32_adds_in_ascending_order():
  parts = [np.array([1.0, 1e8], np.float32), np.array([1e8, 1.0], np.float32), np.array([-1e8, -1e8], np.float32),
           np.array([3.0, 3.0], np.float32)]
  # ((a + b) + c) + d in fp32: the 1.0 is lost under 1e8 in either column, whatever float64 would keep
  assert np.array_equal(au.sum_parts32(parts), np.array([3.0, 3.0], np.float32))
  # (the reverse order is another number: only the ascending one is the kernel's)
  assert np.array_equal(au.sum_parts32(parts[::-1]), np.array([1.0, 0.0], np.float32))
  assert au.sum_parts32(parts[:1])[1] == np.float32(1e8)


# ------------------------------------------------------------------ rk_adam_consts
def _consts_bits(lr, wd, step):
  return np.array(au.consts32(lr, B1, B2, EPS, wd, step), dtype=np.float64).astype(np.float32).view(np.int32)


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
@pytest.mark.parametrize("wd", [0.0, 2e-5])
def test_adam_consts_are_the_restatements_bits(lib, step, wd):
  out = np.full(8 + 8, 12345.0, np.float32)
  assert lib.rk_adam_consts(LR, B1, B2, EPS, wd, step, 1, 8, out.ctypes.data) == 0
  assert np.array_equal(out[:8].view(np.int32), _consts_bits(LR, wd, step))
  assert np.all(out[8:] == 12345.0)


def test_adam_consts_strided_table_leaves_the_gaps(lib):
  stride, n_steps, first = 16, 3, 7
  out = np.full(stride * n_steps + 8, 12345.0, np.float32)
  assert lib.rk_adam_consts(3e-4, B1, B2, EPS, 1e-5, first, n_steps, stride, out.ctypes.data) == 0
  for i in range(n_steps):
    assert np.array_equal(out[i * stride:i * stride + 8].view(np.int32), _consts_bits(3e-4, 1e-5, first + i)), i
    assert np.all(out[i * stride + 8:(i + 1) * stride] == 12345.0), i
  assert np.all(out[stride * n_steps:] == 12345.0)
  # n_steps 0 writes nothing; step 0 is refused
  out[:] = 7.0
  assert lib.rk_adam_consts(3e-4, B1, B2, EPS, 1e-5, 1, 0, stride, out.ctypes.data) == 0
  assert np.all(out == 7.0)
  assert lib.rk_adam_consts(3e-4, B1, B2, EPS, 1e-5, 0, 1, stride, out.ctypes.data) != 0


# ------------------------------------------------------------------ refusals in front of any launch
class _Host:
  """Host buffers that stand in for device arrays: a refused call reads none of them."""

  def __init__(self):
    self.f = torch.zeros(4096, dtype=torch.float32)
    self.i = torch.zeros(64, dtype=torch.int32)
    assert self.f.data_ptr() % 16 == 0

  def job(self, h=4, n_rows=8, **kw):
    from recoder_amd._lib import RkAdamJob
    j = RkAdamJob()
    a = j.par
    a.p, a.m, a.v = self.f.data_ptr(), self.f.data_ptr() + 1024 * 4, self.f.data_ptr() + 2048 * 4
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step, a.sparse = LR, B1, B2, EPS, 0.0, 1, 0
    j.n_rows, j.h, j.g, j.g_parts, j.g_stride = n_rows, h, self.f.data_ptr() + 3072 * 4, 1, 0
    for k, val in kw.items():
      if k in ("step", "sparse", "p", "m", "v"):
        setattr(a, k, val)
      else:
        setattr(j, k, val)
    return j


def _refused(lib, rc, text):
  assert rc != 0
  msg = lib.rk_last_error().decode()
  assert text in msg, msg


def test_adam_multi_refusals_return_before_any_launch(lib):
  H = _Host()
  ip, fp = H.i.data_ptr(), H.f.data_ptr()

  def multi(j, n=1, loss_part=None, loss_out=None):
    return lib.rk_adam_multi(ctypes.byref(j) if not isinstance(j, ctypes.Array) else j, n, loss_part, 4, 1.0,
                             loss_out, None)

  from recoder_amd._lib import RkAdamJob
  eleven = (RkAdamJob * 11)(*[H.job() for _ in range(11)])
  _refused(lib, multi(eleven, 11), "too many jobs for one launch")
  _refused(lib, multi(H.job(step=0)), "step must be >= 1")
  _refused(lib, multi(H.job(g_parts=0)), "g_parts must be >= 1")
  _refused(lib, multi(H.job(sparse=1, rows=None, n_dev=ip, n_cap=4)), "SparseAdam job needs rows and n_dev")
  _refused(lib, multi(H.job(sparse=1, rows=ip, n_dev=None, n_cap=4)), "SparseAdam job needs rows and n_dev")
  for field in ("p", "m", "v", "g"):                      # h % 4 == 0: every operand 16-byte aligned
    base = H.job()
    at = getattr(base, field) if field == "g" else getattr(base.par, field)
    _refused(lib, multi(H.job(**{field: at + 4})), "vector jobs need 16-byte aligned operands / strides")
  _refused(lib, multi(H.job(g_parts=2, g_stride=34)), "vector jobs need 16-byte aligned operands / strides")
  _refused(lib, multi(H.job(g_parts=2, g_stride=32, gstride_dev=ip)), "vector jobs need 16-byte aligned operands / strides")
  _refused(lib, multi(H.job(sparse=1, rows=ip, n_dev=ip, n_cap=4, row_step=2)), "row0 / row_step apply to dense jobs")
  _refused(lib, multi(H.job(sparse=1, rows=ip, n_dev=ip, n_cap=4, row0=1)), "row0 / row_step apply to dense jobs")
  _refused(lib, multi(H.job(), loss_part=fp, loss_out=None), "loss_part and loss_out go together")
  _refused(lib, multi(H.job(), loss_part=None, loss_out=fp), "loss_part and loss_out go together")
  # a lazy job outside a replay bracket: no cursor, no constants table
  _refused(lib, multi(H.job(pos=ip, lazy_stamp=ip, lazy_period=4)), "lazy jobs take their constants from the replay table")


def test_lazy_flush_refuses_a_step_in_front_of_the_epoch(lib):
  H = _Host()
  j = H.job(lazy_stamp=H.i.data_ptr(), lazy_period=1)
  slots = (ctypes.c_int32 * 1)(0)
  rc = lib.rk_adam_lazy_flush(ctypes.byref(j), 1, H.f.data_ptr(), 1, slots, 99, 100, None)
  _refused(lib, rc, "next_step >= epoch_base")
  # the epoch's first step: nothing can be behind, nothing is launched (no device is needed for the call)
  assert lib.rk_adam_lazy_flush(ctypes.byref(j), 1, H.f.data_ptr(), 1, slots, 100, 100, None) == 0
