"""CPU: stabilisation of a whole world (egs_world_stabilize / egs_world_stabilize_info) is part of the C ABI --
declared in the header, exported by the library, listed in capi.EXPORTS and reachable from capi.World.
No compute calls here."""
import os
import re

import numpy as np

from eggshell_amd import capi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_world_stabilize", "egs_world_stabilize_info")


def _code():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_world_stabilize():
    code = _code()
    for name in NEW:
        assert re.search(r"\begs_status\s+" + name + r"\s*\(\s*egs_world\s*\*", code), name
        assert name in capi.EXPORTS, name
    # mode, max_steps, detect_contacts, params, n_unsettled
    assert re.search(r"egs_world_stabilize\s*\(\s*egs_world\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*int32_t\s+\w+\s*,\s*const\s+egs_solve_params\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)", code)
    # n_ensembles, steps, err_sq
    assert re.search(r"egs_world_stabilize_info\s*\(\s*egs_world\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*double\s*\*\s*\w+\s*\)", code)
    assert re.search(r"#define\s+EGS_STABILIZE_INIT\s+0\b", code)
    assert re.search(r"#define\s+EGS_STABILIZE_POST\s+1\b", code)


def test_library_exports_world_stabilize():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_world_has_stabilize_interface():
    assert callable(getattr(capi.World, "stabilize", None))
    assert callable(getattr(capi.World, "stabilize_info", None))
    assert (capi.STABILIZE_INIT, capi.STABILIZE_POST) == (0, 1)


def test_cairn_is_deterministic_and_overlapping():
    a, b = scenes.cairn(5, seed=3), scenes.cairn(5, seed=3)
    assert np.array_equal(a["p"], b["p"]) and np.array_equal(a["R"], b["R"])
    assert not np.array_equal(a["R"], scenes.cairn(5, seed=4)["R"])
    for R in a["R"].reshape(-1, 3, 3):
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    gaps = np.diff(a["p"][:, 2])
    assert (gaps < scenes.SIDE).all() and a["p"][0, 2] < scenes.SIDE / 2
