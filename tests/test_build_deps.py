"""CPU: a side library's private headers (csrc/<stem>/*.h) rebuild that library and no other."""
import os

from recoder_amd import build


def test_private_headers_are_their_own_librarys_dependencies():
  private = os.path.join(build.CSRC, "als")
  mine = sorted(os.path.join(private, f) for f in os.listdir(private) if f.endswith(".h"))
  assert os.path.join(private, "ssm.h") in mine and os.path.join(private, "common.h") in mine
  assert set(mine) <= set(build.headers_of("als"))
  for row in build.LIBRARIES:
    if row[0] != "als":
      assert not set(mine) & set(build.headers_of(row[0])), row[0]


def test_headers_of_keeps_every_librarys_public_and_shared_headers():
  for stem, _, public, needs_training, _ in build.LIBRARIES:
    got = build.headers_of(stem)
    assert all(os.path.exists(h) for h in got)
    assert {os.path.join(build.INCLUDE, h) for h in public} <= set(got)
    shared = "common.h" if needs_training else "side_error.h"
    assert os.path.join(build.CSRC, shared) in got
