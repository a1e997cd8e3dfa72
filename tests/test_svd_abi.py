"""CPU: librecoder_svd.so is built beside the other five libraries and exports exactly what
include/recoder_svd.h declares (each bound in _svd_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SVD_HEADER = os.path.join(INC, "recoder_svd.h")
TRAIN_HEADERS = [os.path.join(INC, "recoder_hip.h"), os.path.join(INC, "recoder_hip_probe.h")]


def _declared(paths):
  src = "".join(open(p).read() for p in paths)
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  return sorted(set(re.findall(r"\b(rk_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
  out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
  return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)


@pytest.fixture(scope="module")
def built():
  from recoder_amd import build
  build.build_library(verbose=False)
  return build


def test_build_produces_the_svd_library(built):
  assert os.path.basename(built.SVD_LIB) == "librecoder_svd.so"
  assert os.path.exists(built.SVD_LIB)
  assert "six HIP libraries" in built.__doc__


def test_svd_library_exports_exactly_its_header(built):
  from recoder_amd import _svd_lib, svd
  declared = _declared([SVD_HEADER])
  assert declared and all(s.startswith("rk_svd_") for s in declared)
  for name in ("rk_svd_version", "rk_svd_last_error", "rk_svd_max_l", "rk_svd_gaussian", "rk_svd_spmm",
               "rk_svd_chol_inverse", "rk_svd_rotate"):
    assert name in declared
  assert _exports(built.SVD_LIB) == declared
  assert sorted(_svd_lib.SIGNATURES) == declared
  lib = _svd_lib.load()
  assert lib.rk_svd_version() >= 100
  assert isinstance(lib.rk_svd_last_error(), bytes)
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


def test_other_libraries_exports_are_unchanged(built):
  exported = _exports(built.LIB)
  assert exported == _declared(TRAIN_HEADERS)
  assert len(exported) == 80
  others = ((built.INDEX_LIB, "recoder_index.h", "rk_ix_"), (built.ALS_LIB, "recoder_als.h", "rk_als_"),
            (built.VAE_LIB, "recoder_vae.h", "rk_vae_"), (built.EASE_LIB, "recoder_ease.h", "rk_ease_"))
  for lib, header, prefix in others:
    got = _exports(lib)
    assert got == _declared([os.path.join(INC, header)])
    assert got and all(s.startswith(prefix) for s in got)
  assert not any(s.startswith("rk_svd_") for lib in (built.LIB,) + tuple(o[0] for o in others) for s in _exports(lib))
