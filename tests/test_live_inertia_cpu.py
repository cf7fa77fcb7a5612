"""CPU: live inertia (egs_problem_set_live_inertia / egs_problem_get_mass and their world twins) is part of the C ABI --
declared in the header, exported by the library, listed in capi.EXPORTS and reachable from capi.Problem / capi.World
-- and the oracle twin of the free brick shows what it is for: with M^-1 and the gyroscopic torque recomputed at every
step's start the angular momentum holds and the brick flips about its intermediate axis; frozen at Init (quirk Q5)
neither is true.  No compute calls on the device here."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import live_inertia_cases as lic
from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_problem_set_live_inertia", "egs_problem_get_mass", "egs_world_set_live_inertia", "egs_world_get_mass")


def test_header_declares_live_inertia():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\begs_status\s+" + name + r"\s*\(", code), name
    for handle, stem in (("egs_problem", "egs_problem"), ("egs_world", "egs_world")):
        assert re.search(stem + r"_set_live_inertia\s*\(\s*" + handle + r"\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                         r"\s*const\s+double\s*\*\s*\w+\s*\)", code)
        assert re.search(stem + r"_get_mass\s*\(\s*" + handle + r"\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", code)


def test_library_exports_live_inertia():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 3


def test_python_classes_have_the_interface():
    for cls in (capi.Problem, capi.World):
        assert callable(getattr(cls, "set_live_inertia", None))
        assert callable(getattr(cls, "mass", None))


def test_the_skip_rule():
    I = np.array([np.eye(3) * 0.1, lic.BRICK, np.diag([0.1, 0.1, 0.1 + 2.0 ** -56]), np.eye(3) * 0.1 + 1e-300 * np.eye(3)[::-1]])
    assert lic.is_skipped(I).tolist() == [True, False, False, False]


@pytest.fixture(scope="module")
def random_runs():
    return {live: lic.twin_run("random", 1000, live)[0] for live in (True, False)}


def test_twin_live_keeps_the_angular_momentum(random_runs):
    t = random_runs[True]
    print("live: L drift %.3e, energy change %.3e" % (t.drift, t.energy_change))
    assert t.drift <= 1e-2


def test_twin_frozen_does_not(random_runs):
    t = random_runs[False]
    print("frozen: L drift %.3e, energy change %.3e" % (t.drift, t.energy_change))
    assert t.drift >= 0.5


def test_adapter_explicit_path_on_the_host():
    """Ensemble::SetLiveInertia on the explicit path of Step (use_device_step = false): a body without constraints is
    stepped on the host, with both arrays recomputed by Init()'s own code -- the twin's figures, no device."""
    demo = os.path.join(ROOT, "eggshell_amd", "host", "tumble_demo")
    if not os.path.exists(demo):
        pytest.fail("tumble_demo is not built: run __graft_entry__.build()")
    out = subprocess.run([demo, "--explicit"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = {(r["start"], r["live"]): r for r in map(json.loads, out.stdout.splitlines())}
    assert rows[("random", 1)]["L_drift"] <= 1e-2 and rows[("random", 0)]["L_drift"] >= 0.5
    assert 1000 < rows[("intermediate", 1)]["flip_step"] < 2000 and rows[("intermediate", 0)]["flip_step"] == -1


def test_twin_intermediate_axis_flips_live_only():
    live = lic.twin_run("intermediate", 4000, True)[0]
    frozen = lic.twin_run("intermediate", 4000, False)[0]
    print("live flips at", live.flips, "frozen at", frozen.flips)
    assert live.flips and 1000 < live.flips[0] < 2000
    assert frozen.flips == []
