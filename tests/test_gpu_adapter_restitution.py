"""GPU (-m gpu): Ensemble::SetRestitution of the reference-shaped C++ API (eggshell_amd/host), driven by
`restitution_demo`: a ball and a flat cube released 5 cm above the plate come back up at e times the speed they
arrived with -- the reference's value (tests/test_restitution_reference_cpu.py) -- and rise to the apex that speed
gives; with restitution off they stop dead."""
import json
import os
import subprocess

import pytest

from eggshell_amd import capi

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "restitution_demo")
G, ERP, CFM = 9.8, 0.2, 0.01


def run(*args):
    if not os.path.exists(DEMO):
        pytest.fail("restitution_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO, *args], check=True, capture_output=True, text=True, timeout=120)
    return {r["body"]: r for r in map(json.loads, p.stdout.strip().splitlines())}


@pytest.fixture(scope="module")
def bounced():
    return run("0.8", "0.1")


@pytest.mark.parametrize("body", ["sphere", "cube"])
def test_dropped_body_comes_back_up(bounced, body):
    """after = -e before: exactly (a few roundings of values of order |before| / dt) for the ball, whose row is solved
    with cfm 0; for the cube within dt cfm lambda_max, the regularisation's share of J v' (cfm 0.01, its four rows
    being solved to SOR's 60-sweep residual, below 1e-9 of lambda).  The body then flies freely: the midpoint rule
    samples the parabola exactly, so the largest sampled height is within g dt^2 / 8 of z + after^2 / 2g."""
    r = bounced[body]
    dt, e = r["dt"], r["e"]
    assert r["impact_step"] > 0 and r["contacts"] == (1 if body == "sphere" else 4)
    assert r["before"] < -0.9      # sqrt(2 g 0.05) = 0.99 m/s
    want = -e * r["before"]
    bound = 64 * 2.0 ** -53 * (abs(r["before"]) + dt * (G + r["lambda_max"])) if body == "sphere" else \
        dt * CFM * r["lambda_max"] * (1 + 1e-6) + 1e-12
    print("%s: before %.17g after %.17g, -e before %.17g, bound %.3g" % (body, r["before"], r["after"], want, bound))
    assert abs(r["after"] - want) <= bound
    apex = r["z_after"] + r["after"] ** 2 / (2 * G)
    assert abs(r["apex"] - apex) <= G * dt * dt / 8 + 1e-12
    assert r["apex"] > r["z_after"] + 0.02


def test_off_stops_dead():
    for body, r in run("-1").items():
        assert r["impact_step"] > 0 and 0 < r["after"] <= ERP * 0.02 / r["dt"], body     # the Baumgarte velocity of < 2 cm


def test_refusals():
    p = subprocess.run([DEMO, "--refuse"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    assert [json.loads(l)["refused"] for l in p.stdout.strip().splitlines()] == [capi.ERR_INVALID] * 2
