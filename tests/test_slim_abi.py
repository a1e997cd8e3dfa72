"""CPU: librecoder_slim.so is built beside the other seven libraries and exports exactly what
include/recoder_slim.h declares (each bound in _slim_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SLIM_HEADER = os.path.join(INC, "recoder_slim.h")
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


def test_build_produces_the_slim_library(built):
  assert os.path.basename(built.SLIM_LIB) == "librecoder_slim.so"
  assert os.path.exists(built.SLIM_LIB)
  assert built.SLIM_SOURCES == ["slim.hip"]
  assert "eighth" in built.__doc__ and "librecoder_slim.so" in built.__doc__


def test_slim_library_exports_exactly_its_header(built):
  from recoder_amd import _slim_lib, slim
  declared = _declared([SLIM_HEADER])
  assert declared and all(s.startswith("rk_slim_") for s in declared)
  for name in ("rk_slim_version", "rk_slim_last_error", "rk_slim_max_neighbours", "rk_slim_lds_candidates",
               "rk_slim_fit_workspace_bytes", "rk_slim_fit", "rk_slim_scores"):
    assert name in declared
  assert _exports(built.SLIM_LIB) == declared
  assert sorted(_slim_lib.SIGNATURES) == declared
  lib = _slim_lib.load()
  assert lib.rk_slim_version() >= 100
  assert isinstance(lib.rk_slim_last_error(), bytes)
  assert lib.rk_slim_max_neighbours() == slim.MAX_NEIGHBOURS >= 1024
  assert lib.rk_slim_lds_candidates() == slim.LDS_CANDIDATES > 64
  # the workspace query is host arithmetic: no device needed
  lds = lib.rk_slim_lds_candidates()
  for n in (1, 37, lds, lds + 1, lds + 1000, 7915, 100000):
    assert lib.rk_slim_fit_workspace_bytes(n) == slim.workspace_bytes(n) > 0
  assert lib.rk_slim_fit_workspace_bytes(lds) < lib.rk_slim_fit_workspace_bytes(lds + 1)
  assert lib.rk_slim_fit_workspace_bytes(0) < 0 and lib.rk_slim_fit_workspace_bytes(-5) < 0
  assert b"n_items" in lib.rk_slim_last_error()


def test_other_libraries_exports_are_unchanged(built):
  exported = _exports(built.LIB)
  assert exported == _declared(TRAIN_HEADERS)
  assert len(exported) == 80
  others = ((built.INDEX_LIB, "recoder_index.h", "rk_ix_"), (built.ALS_LIB, "recoder_als.h", "rk_als_"),
            (built.VAE_LIB, "recoder_vae.h", "rk_vae_"), (built.EASE_LIB, "recoder_ease.h", "rk_ease_"),
            (built.SVD_LIB, "recoder_svd.h", "rk_svd_"), (built.RP3_LIB, "recoder_rp3.h", "rk_rp3_"))
  for lib, header, prefix in others:
    got = _exports(lib)
    assert got == _declared([os.path.join(INC, header)])
    assert got and all(s.startswith(prefix) for s in got)
  assert not any(s.startswith("rk_slim_") for lib in (built.LIB,) + tuple(o[0] for o in others) for s in _exports(lib))
