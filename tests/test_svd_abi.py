"""CPU: librecoder_svd.so is built beside the other five libraries and exports exactly what
include/recoder_svd.h declares (each bound in _svd_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os
import re

from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVD_HEADER = os.path.join(ROOT, "include", "recoder_svd.h")


def test_build_produces_the_svd_library(built):
  assert os.path.basename(built.SVD_LIB) == "librecoder_svd.so"
  assert os.path.exists(built.SVD_LIB)
  assert "six HIP libraries" in built.__doc__


def test_svd_library_exports_exactly_its_header(built):
  from recoder_amd import _svd_lib, svd
  for name in ("rk_svd_version", "rk_svd_last_error", "rk_svd_max_l", "rk_svd_gaussian", "rk_svd_spmm",
               "rk_svd_chol_inverse", "rk_svd_rotate"):
    assert name in declared([SVD_HEADER])
  lib = _svd_lib.load()
  assert lib.rk_svd_max_l() == svd.MAX_L == 512
  # the long-row threshold of the sparse product: one value in the header, the binding and the driver
  m = re.search(r"#define\s+RK_SVD_LONG_ROW\s+(\d+)", open(SVD_HEADER).read())
  assert int(m.group(1)) == _svd_lib.LONG_ROW == svd.LONG_ROW
  # the workspace query is host arithmetic: no device needed
  assert lib.rk_svd_chol_inverse_workspace_bytes(20) == 0
  assert lib.rk_svd_chol_inverse_workspace_bytes(216) == 216 * 216 * 8
  assert lib.rk_svd_chol_inverse_workspace_bytes(0) < 0 and lib.rk_svd_chol_inverse_workspace_bytes(513) < 0
  for l in (1, 80, 128, 129, 512):
    assert svd.required_bytes(0, 0, l, 0) - 16 == lib.rk_svd_chol_inverse_workspace_bytes(l)
