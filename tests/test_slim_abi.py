"""CPU: librecoder_slim.so is built beside the other seven libraries and exports exactly what
include/recoder_slim.h declares (each bound in _slim_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os

from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLIM_HEADER = os.path.join(ROOT, "include", "recoder_slim.h")


def test_build_produces_the_slim_library(built):
  assert os.path.basename(built.SLIM_LIB) == "librecoder_slim.so"
  assert os.path.exists(built.SLIM_LIB)
  assert built.SLIM_SOURCES == ["slim.hip"]
  assert "eighth" in built.__doc__ and "librecoder_slim.so" in built.__doc__


def test_slim_library_exports_exactly_its_header(built):
  from recoder_amd import _slim_lib, slim
  for name in ("rk_slim_version", "rk_slim_last_error", "rk_slim_max_neighbours", "rk_slim_lds_candidates",
               "rk_slim_fit_workspace_bytes", "rk_slim_fit", "rk_slim_scores"):
    assert name in declared([SLIM_HEADER])
  lib = _slim_lib.load()
  assert lib.rk_slim_max_neighbours() == slim.MAX_NEIGHBOURS >= 1024
  assert lib.rk_slim_lds_candidates() == slim.LDS_CANDIDATES > 64
  # the workspace query is host arithmetic: no device needed
  lds = lib.rk_slim_lds_candidates()
  for n in (1, 37, lds, lds + 1, lds + 1000, 7915, 100000):
    assert lib.rk_slim_fit_workspace_bytes(n) == slim.workspace_bytes(n) > 0
  assert lib.rk_slim_fit_workspace_bytes(lds) < lib.rk_slim_fit_workspace_bytes(lds + 1)
  assert lib.rk_slim_fit_workspace_bytes(0) < 0 and lib.rk_slim_fit_workspace_bytes(-5) < 0
  assert b"n_items" in lib.rk_slim_last_error()
