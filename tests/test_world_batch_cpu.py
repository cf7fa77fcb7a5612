"""CPU: the batched world (egs_world_create_batch / egs_world_batch_info) is part of
the C ABI -- declared in the header, exported by the library, listed in capi.EXPORTS
and reachable from capi.World.  No compute calls here."""
import os
import re

from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_world_create_batch", "egs_world_batch_info")


def test_header_declares_batched_world():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\begs_status\s+" + name + r"\s*\(", code), name
    # the per-ensemble read-out takes the four tables, any of them NULL
    assert re.search(r"egs_world_batch_info\s*\(\s*egs_world\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s*\*", code)


def test_library_exports_batched_world():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name


def test_python_world_has_batch_interface():
    assert callable(getattr(capi.World, "batch", None))
    assert callable(getattr(capi.World, "batch_info", None))
