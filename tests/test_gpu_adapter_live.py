"""GPU (-m gpu): live inertia through the C++ adapter (Ensemble::SetLiveInertia, tumble_demo): the free brick keeps its
angular momentum and flips about its intermediate axis with it on, does neither with it off (quirk Q5, the default), and
M_inverse() / external_force_torque() read back from the device are the oracle's at the pose the device holds."""
import json
import os
import subprocess

import numpy as np
import pytest

import live_inertia_cases as lic
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "tumble_demo")


def run_demo(*args):
    if not os.path.exists(DEMO):
        pytest.fail("tumble_demo is not built: run __graft_entry__.build()")
    out = subprocess.run([DEMO] + list(args), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.fixture(scope="module")
def runs():
    rows = run_demo()
    return {(r["start"], r["live"]): r for r in rows}


def test_demo_prints_the_four_runs(runs):
    assert sorted(runs) == [("intermediate", 0), ("intermediate", 1), ("random", 0), ("random", 1)]
    print(runs)


def test_angular_momentum_holds_with_live_inertia_only(runs):
    assert runs[("random", 1)]["L_drift"] <= 1e-2
    assert runs[("random", 0)]["L_drift"] >= 0.5


def test_the_brick_flips_with_live_inertia_only(runs):
    assert 1000 < runs[("intermediate", 1)]["flip_step"] < 2000
    assert runs[("intermediate", 0)]["flip_step"] == -1
    # the adapter's device world is the C ABI's: the oracle twin flips at the same step
    assert runs[("intermediate", 1)]["flip_step"] == lic.twin_run("intermediate", 2000, True)[0].flips[0]


def test_m_inverse_is_the_oracles_at_the_device_pose():
    row = run_demo("--minv")[0]
    R, w = np.array(row["R"]).reshape(1, 9), np.array(row["w"]).reshape(1, 3)
    assert np.abs(R - lic.R_START).max() > 1e-4      # after a step: not the pose Init() saw
    M = orc.minv_blocks(R, np.ones(1), lic.BRICK.reshape(1, 9)).reshape(6, 6)
    f = orc.external_force(R, w, np.ones(1), lic.BRICK.reshape(1, 9)).reshape(6)
    assert np.array_equal(np.array(row["Minv_angular"]).reshape(3, 3), M[3:, 3:])
    assert np.array_equal(np.array(row["torque"]), f[3:])
    assert row["inv_mass"] == 1.0 and row["force"] == [0.0, 0.0, 0.0]      # the linear rows stay the caller's
