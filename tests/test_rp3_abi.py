"""CPU: librecoder_rp3.so is built beside the other six libraries and exports exactly what
include/recoder_rp3.h declares (each bound in _rp3_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os

from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RP3_HEADER = os.path.join(ROOT, "include", "recoder_rp3.h")


def test_build_produces_the_rp3_library(built):
  assert os.path.basename(built.RP3_LIB) == "librecoder_rp3.so"
  assert os.path.exists(built.RP3_LIB)
  assert built.RP3_SOURCES == ["rp3.hip"]
  assert "seventh" in built.__doc__ and "librecoder_rp3.so" in built.__doc__


def test_rp3_library_exports_exactly_its_header(built):
  from recoder_amd import _rp3_lib, rp3
  for name in ("rk_rp3_version", "rk_rp3_last_error", "rk_rp3_max_neighbours", "rk_rp3_lds_items",
               "rk_rp3_fit_workspace_bytes", "rk_rp3_fit", "rk_rp3_scores"):
    assert name in declared([RP3_HEADER])
  lib = _rp3_lib.load()
  assert lib.rk_rp3_max_neighbours() == rp3.MAX_NEIGHBOURS >= 1024
  assert lib.rk_rp3_lds_items() == rp3.LDS_ITEMS > 0
  # the workspace query is host arithmetic: no device needed
  lds = lib.rk_rp3_lds_items()
  for n in (1, 37, lds, lds + 1, lds + 1000, 250000, 10 ** 6):
    assert lib.rk_rp3_fit_workspace_bytes(n) == rp3.workspace_bytes(n) > 0
  assert lib.rk_rp3_fit_workspace_bytes(lds) < lib.rk_rp3_fit_workspace_bytes(lds + 1)
  assert lib.rk_rp3_fit_workspace_bytes(0) < 0 and lib.rk_rp3_fit_workspace_bytes(-5) < 0
  assert b"n_items" in lib.rk_rp3_last_error()
