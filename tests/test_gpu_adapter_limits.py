"""GPU (-m gpu): hinge angle limits of the reference-shaped C++ API (eggshell_amd/host: HingeAxisJoint::SetLimits,
Ensemble::SetHingeLimits / HingeAngle), driven by `hinge_limit_demo`: a door that falls onto its stop, the same door on
a motor that stalls there, and the refusal of a limited hinge on the dense path.

The bounds.  About its hinge the door is a pendulum with theta'' = a cos(theta), a = m g r / (I + m r^2) <= g / r
whatever its mass (r = 0.5 m, the arm).  tests/test_gpu_limits_world.py derives, for the step w' = w + a cos(theta) dt;
theta += dt (w + w') / 2 from rest at theta = 0, that the step which first crosses hi ends at most W dt past it, W the
least fixed point of W = sqrt(2 a sin(hi + W dt) (1 + (hi + W dt) W dt)); W grows with a, so a = g / r bounds it.  Past
the stop the solve asks for s^ . w' = -erp sin(excess) / dt.  The first step in which the row acts still moves by
dt (w + w') / 2 with w <= W the speed the door arrived with: W dt / 2 - erp sin(excess) / 2 more, so at most
(1 + (1 - erp) / 2) W dt past the stop in all (the crossing step itself ending W dt past it).  From then on
excess_k+1 = excess_k - erp (sin(excess_k-1) + sin(excess_k)) / 2 <= (1 - erp / 2) excess_k.  One per cent on top covers
the ball joint solved with the hinge and the solve's tolerance (dt tol on a velocity)."""
import json
import math
import os
import subprocess

import pytest

from eggshell_amd import capi

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "hinge_limit_demo")
ERP, U, G = 0.2, 2.0 ** -53, 9.8


@pytest.fixture(scope="module")
def scenes():
    if not os.path.exists(DEMO):
        pytest.fail("hinge_limit_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO], check=True, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    return {r["scene"]: r for r in map(json.loads, p.stdout.strip().splitlines())}


def crossing_speed(a, hi, dt):
    W = math.sqrt(2 * a * math.sin(hi))
    for _ in range(60):
        W = math.sqrt(2 * a * math.sin(hi + W * dt) * (1 + (hi + W * dt) * W * dt))
    return W


def test_door_stops_at_its_limit_and_hinge_angle_reports_it(scenes):
    r = scenes["door"]
    dt, hi, a = r["dt"], r["hi"], G / r["arm"]
    over = 1.01 * crossing_speed(a, hi, dt) * dt * (1 + (1 - ERP) / 2)
    print("door: largest angle %.6g of hi %.3g (bound on the excess %.3g), first over at step %d; at the end angle %.12g, "
          "from the position %.12g, w %.3g; multiplier at the stop %.4g" %
          (r["max_angle"], hi, over, r["first_over"], r["angle_end"], r["angle_from_position"], r["w_axis_end"], r["lambda_stop"]))
    assert r["first_over"] > 10                                   # a free swing first
    assert hi < r["max_angle"] <= hi + over
    assert r["lambda_stop"] < 0.0                                 # the upper stop pushes back only
    # at rest on the stop: the excess has shrunk by at least (1 - erp / 2) a step since the crossing; should it ever reach
    # 0, one free step brings it back by at most a dt^2
    left = 200 - 1 - r["first_over"]
    rest = 1.01 * a * dt * dt
    assert over * (1 - ERP / 2) ** left <= rest
    assert hi - 1e-9 <= r["angle_end"] <= hi + rest
    assert abs(r["w_axis_end"]) <= 1.01 * a * dt
    # HingeAngle against the angle of the centre about the anchor: the anchor may be off by |err|_2 <= sqrt(3) max_err on
    # an arm r, the axis tilted by max_err
    assert abs(r["angle_end"] - r["angle_from_position"]) <= (3 ** 0.5 / r["arm"] + 2) * r["max_err"] + 64 * U


def test_motor_holds_its_speed_inside_the_range_and_stalls_at_the_stop(scenes):
    r = scenes["motor"]
    dt, hi = r["dt"], r["hi"]
    print("motor: at step 40 angle %.4g, w %.17g (target %.3g), multiplier %.4g of %.3g; largest angle %.6g of hi %.3g; at the end "
          "angle %.12g, w %.3g, multiplier at the stop %.4g" %
          (r["angle_mid"], r["w_axis_mid"], r["speed"], r["lambda_mid"], r["tau"], r["max_angle"], hi, r["angle_end"], r["w_axis_end"],
           r["lambda_stop"]))
    # inside the range the motor works as without the table (test_gpu_adapter_joints' bound)
    assert r["angle_mid"] < hi
    assert abs(r["w_axis_mid"] - r["speed"]) <= dt * r["tol"] + r["max_err"] * abs(r["w_axis_mid"]) + 64 * U
    assert 0 < abs(r["lambda_mid"]) < r["tau"]
    # it arrives at the motor's speed: one step's travel past the stop at the most, half a step's more while the row
    # first acts, then the row is the limit's
    over = 1.01 * r["speed"] * dt * (1 + (1 - ERP) / 2)
    assert r["first_over"] > 40 and hi < r["max_angle"] <= hi + over
    assert r["lambda_stop"] < 0.0
    assert hi - 1e-9 <= r["angle_end"] <= hi + over
    # stalled: the limit row asks for s^ . w' = -erp sin(excess) / dt, never the motor's +speed
    assert -ERP * over / dt <= r["w_axis_end"] <= dt * r["tol"]


def test_limited_hinge_on_the_dense_path_is_refused():
    p = subprocess.run([DEMO, "--dense"], capture_output=True, text=True, timeout=120)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0 and r["refused"] == capi.ERR_UNSUPPORTED and r["names_hinge"] == 1
