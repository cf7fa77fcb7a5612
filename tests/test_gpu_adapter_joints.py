"""GPU (-m gpu): welds and hinges of the reference-shaped C++ API (eggshell_amd/host: AngularLockJoint, HingeAxisJoint,
Ensemble::AddWeld / AddHinge / SetHingeMotor), driven by `hinge_demo`: a door swinging on one hinge, the same door on
a motor, a welded two-box beam, and the refusal of a free hinge on the dense path.

The steps are solved by SOR to a residual tol with cfm = 0, so a row of an equality block leaves a step with
    |J v'| <= erp |err| / dt + dt tol
(rhs = -(erp / dt^2) err - J (v / dt + M^-1 f), residual w = A lambda - rhs, J v' = dt (J (v/dt + M^-1 f) + A lambda)),
and an error that each step multiplies by (1 - erp) and feeds with d stays below d / erp."""
import json
import os
import subprocess

import pytest

from eggshell_amd import capi

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "hinge_demo")
ERP, U = 0.2, 2.0 ** -53


@pytest.fixture(scope="module")
def scenes():
    if not os.path.exists(DEMO):
        pytest.fail("hinge_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO], check=True, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    return {r["scene"]: r for r in map(json.loads, p.stdout.strip().splitlines())}


def test_door_swings_about_its_axis_only(scenes):
    r = scenes["door"]
    bound = ERP * r["max_err"] / r["dt"] + r["dt"] * r["tol"] + 64 * U * max(1.0, abs(r["w_axis"]))
    print("door: across %.3g, bound %.3g (max err %.3g), swing %.3g, w about the axis %.3g" %
          (r["across"], bound, r["max_err"], r["swing"], r["w_axis"]))
    assert r["across"] <= bound
    assert r["swing"] > 0.3 and abs(r["w_axis"]) > 0.1      # it fell: half a metre of arm, one second
    assert r["lambda_axis"] == 0.0                          # the free hinge's axis row is pinned


def test_motor_reaches_its_speed(scenes):
    r = scenes["motor"]
    # w_axis is the world-y component; the axis itself is within max_err of world y
    bound = r["dt"] * r["tol"] + r["max_err"] * abs(r["w_axis"]) + 64 * U
    print("motor: w about the axis %.17g, target %.3g, bound %.3g; multiplier %.6g of %.3g" %
          (r["w_axis"], r["speed"], bound, r["lambda_axis"], r["tau"]))
    assert abs(r["w_axis"] - r["speed"]) <= bound
    assert 0 < abs(r["lambda_axis"]) < r["tau"]             # holding the speed against gravity, inside its limit
    assert r["across"] <= ERP * r["max_err"] / r["dt"] + r["dt"] * r["tol"] + 64 * U


def test_welded_beam_stays_straight(scenes):
    r = scenes["beam"]
    feed = r["dt"] ** 2 * r["tol"] + 64 * U * 3.0           # the solve's residual, the rounding of a pose of size <= 3
    print("beam: lock error %.3g (bound %.3g), twist %.3g, tip sag %.3g" % (r["max_err"], feed / ERP, r["twist"], r["tip_sag"]))
    assert r["joints"] == 4
    assert r["max_err"] <= feed / ERP
    assert r["twist"] <= 2 * 3 ** 0.5 * r["max_err"] + 16 * U     # |R0^T R1 - I| <= theta, sin(theta) = |err|_2
    # the tip: two anchor errors and the turns of the two welds (<= 2 sqrt(3) max_err each) on arms of 0.9 and 0.3 m
    assert abs(r["tip_sag"]) <= (2 + 2 * 3 ** 0.5 * 1.2) * r["max_err"] + 64 * U * 3


def test_free_hinge_on_the_dense_path_is_refused():
    p = subprocess.run([DEMO, "--dense-free"], capture_output=True, text=True, timeout=120)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0 and r["refused"] == capi.ERR_UNSUPPORTED and r["names_hinge"] == 1
