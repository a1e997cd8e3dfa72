"""CPU: librecoder_ease.so is built beside the other four libraries and exports exactly what
include/recoder_ease.h declares (each bound in _ease_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
EASE_HEADER = os.path.join(INC, "recoder_ease.h")
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


def test_build_produces_the_ease_library(built):
  assert os.path.basename(built.EASE_LIB) == "librecoder_ease.so"
  assert os.path.exists(built.EASE_LIB)


def test_ease_library_exports_exactly_its_header(built):
  from recoder_amd import _ease_lib
  declared = _declared([EASE_HEADER])
  assert declared and all(s.startswith("rk_ease_") for s in declared)
  assert _exports(built.EASE_LIB) == declared
  assert sorted(_ease_lib.SIGNATURES) == declared
  lib = _ease_lib.load()
  assert lib.rk_ease_version() >= 100
  assert isinstance(lib.rk_ease_last_error(), bytes)
  # the workspace query is host arithmetic: no device needed; the driver restates it for its memory check
  from recoder_amd import ease
  for n in (1, 64, 129, 7915, 20108, 41140):
    assert lib.rk_ease_spd_inverse_workspace_bytes(n) == ease.inverse_workspace_bytes(n) > 0
  assert lib.rk_ease_spd_inverse_workspace_bytes(0) < 0


def test_other_libraries_exports_are_unchanged(built):
  exported = _exports(built.LIB)
  assert exported == _declared(TRAIN_HEADERS)
  assert len(exported) == 80
  for lib, header, prefix in ((built.INDEX_LIB, "recoder_index.h", "rk_ix_"), (built.ALS_LIB, "recoder_als.h", "rk_als_"),
                              (built.VAE_LIB, "recoder_vae.h", "rk_vae_")):
    got = _exports(lib)
    assert got == _declared([os.path.join(INC, header)])
    assert got and all(s.startswith(prefix) for s in got)
  assert not any(s.startswith("rk_ease_") for lib in (built.LIB, built.INDEX_LIB, built.ALS_LIB, built.VAE_LIB)
                 for s in _exports(lib))
