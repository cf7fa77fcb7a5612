"""GPU (-m gpu): slider joints of the reference-shaped C++ API (eggshell_amd/host: SliderAxisJoint, Ensemble::AddSlider /
SetSliderMotor / SetSliderLimits / SliderPosition), driven by `slider_demo`: a lift lowered by its motor that stalls at
its upper stop, a drawer that falls to its lower stop and rests there (unit boxes on vertical rails, every step a
tolerance-terminated solve; gravity presses either into its stop, so the stop's row stays active), and the refusal of a
free slider on the dense path.

The bounds.  The steps are solved by SOR to a residual tol with cfm = 0, so a row leaves a step within dt tol of its
target.  Both rails are vertical, a = g along them.  The drawer's free fall is stepped as v' = v - a dt;
x += dt (v + v') / 2, exact for a constant acceleration: x = -a (k dt)^2 / 2 after k steps, and the drawer goes under its
stop lo in step K, the least k with a (k dt)^2 / 2 > |lo|, at the speed v = a K dt, at most v dt under it.  The lift arrives at its motor's speed v, at most
v dt over its stop.  Either way the step in which the stop's row first acts still moves by dt (v_old + v') / 2 with v_old
the arrival speed, which no row of that step can change, and v' = -erp excess / dt against it: v dt / 2 - erp excess / 2
further, so the largest excess is at most (1 + (1 - erp) / 2) v dt.  From then on both velocities of every update are the
row's, excess_k+1 = excess_k - erp (excess_k-1 + excess_k) / 2 <= (1 - erp / 2) excess_k: the excess shrinks and stays
positive (the recurrence's roots are real and positive for erp = 0.2), so the motor never gets its row back.  One per
cent on top covers the lock and the two rail equality rows solved with it and the solve's tolerance."""
import json
import os
import subprocess

import pytest

from eggshell_amd import capi

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "slider_demo")
ERP, U, G = 0.2, 2.0 ** -53, 9.8


@pytest.fixture(scope="module")
def scenes():
    if not os.path.exists(DEMO):
        pytest.fail("slider_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO], check=True, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    return {r["scene"]: r for r in map(json.loads, p.stdout.strip().splitlines())}


def test_lift_holds_its_speed_then_stalls_at_its_stop(scenes):
    r = scenes["lift"]
    dt, hi, v = r["dt"], r["stop"], r["speed"]
    print("lift: at step 20 x %.4g, v %.17g (target %.3g), multiplier %.4g of %.3g; largest x %.6g of hi %.3g, first over at step %d; "
          "at the end x %.12g, v %.3g, multiplier at the stop %.4g" %
          (r["x_mid"], r["v_mid"], v, r["lambda_mid"], r["force"], r["extreme"], hi, r["first_over"], r["x_end"], r["v_end"], r["lambda_stop"]))
    assert r["x_start"] == 0.0                                    # AddSlider: x = 0 at creation
    # inside the range the motor holds its speed against gravity with m g < f to spare
    assert r["x_mid"] < hi
    assert abs(r["v_mid"] - v) <= dt * r["tol"] + r["max_err"] * abs(r["v_mid"]) + 64 * U
    assert abs(r["lambda_mid"] + r["mass"] * G * r["g_along"]) <= 1e-6 and abs(r["lambda_mid"]) < r["force"]      # it brakes the load
    # it arrives at the motor's speed
    over = 1.01 * v * dt * (1 + (1 - ERP) / 2)
    assert r["first_over"] > 20 and hi < r["extreme"] <= hi + over
    assert r["lambda_stop"] < 0.0                                 # the upper stop pushes back only
    left = r["steps"] - 1 - r["first_over"]
    assert hi - 1e-9 <= r["x_end"] <= hi + over * (1 - ERP / 2) ** (left - 1)
    # stalled: the stop's row asks for v' = -erp excess / dt, never the motor's +speed
    assert -ERP * over / dt <= r["v_end"] <= dt * r["tol"]


def test_drawer_falls_to_its_stop_and_rests_there(scenes):
    r = scenes["drawer"]
    dt, lo = r["dt"], r["stop"]
    a = G * r["g_along"]
    K = next(k for k in range(1, 1000) if a * (k * dt) ** 2 / 2 > -lo)
    v = a * K * dt
    over = 1.01 * v * dt * (1 + (1 - ERP) / 2)
    print("drawer: smallest x %.6g of lo %.3g (bound on the excess %.3g), first under at step %d (closed form %d); at the end x %.12g, "
          "from the position %.12g, v %.3g; multiplier at the stop %.4g" %
          (r["extreme"], lo, over, r["first_over"], K - 1, r["x_end"], r["x_from_position"], r["v_end"], r["lambda_stop"]))
    assert r["first_over"] == K - 1                               # a free fall first, by the closed form
    assert lo - over <= r["extreme"] < lo
    assert r["lambda_stop"] > 0.0                                 # the lower stop pushes forward only
    left = r["steps"] - 1 - r["first_over"]
    assert lo - over * (1 - ERP / 2) ** (left - 1) <= r["x_end"] <= lo + 1e-9
    assert -dt * r["tol"] <= r["v_end"] <= ERP * over * (1 - ERP / 2) ** (left - 2) / dt + dt * r["tol"]
    # SliderPosition against the height of the centre: the rail direction is tilted by the lock's error at the most, the
    # rail's point off by the equality rows' error
    assert abs(r["x_end"] - r["x_from_position"]) <= 2 * r["max_err"] * (abs(r["x_end"]) + 1) + 64 * U


def test_free_slider_on_the_dense_path_is_refused():
    p = subprocess.run([DEMO, "--dense"], capture_output=True, text=True, timeout=120)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert p.returncode == 0 and r["refused"] == capi.ERR_UNSUPPORTED and r["names_slider"] == 1
