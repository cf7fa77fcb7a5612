"""GPU (-m gpu): Ensemble::CastRays / CastRay and EnsembleGroup::CastRays of the reference-shaped C++ API
(eggshell_amd/host), driven by `ray_demo`: a cube carrying a downward fan falls towards a ball, a log and a cube; the
demo checks every reading against its closed form and the device world's table against the stateless entry, and exits
non-zero on a disagreement."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "ray_demo")
DT, G = 5e-3, 9.8


@pytest.fixture(scope="module")
def out():
    if not os.path.exists(DEMO):
        pytest.fail("ray_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_every_reading_agrees_with_its_closed_form(out):
    assert out["failures"] == 0 and out["steps"] == 60 and len(out["readings"]) == 60


def test_readings_follow_the_falling_carrier(out):
    """Per step (z_carrier, above the ball, above the ground, above the log, above the cube): the ground reading is the
    carrier's height itself, every reading shrinks by the carrier's displacement (the resting bodies move by less than
    the erp residue g dt^2 a step), and the carrier is in free fall: after k steps it has dropped g dt^2 k^2 / 2 if the
    positions move by the mean of the old and the new velocity, g dt^2 k (k + 1) / 2 if by the new one; the bound
    takes either (nothing touches the carrier)."""
    r = np.array(out["readings"])
    z, ball, ground, log, cube = r.T
    assert np.array_equal(ground, z)
    k = np.arange(1, 61)
    drop = (1.5 - z) / (G * DT * DT)
    assert (drop >= k * k / 2 - 1e-6).all() and (drop <= k * (k + 1) / 2 + 1e-6).all()
    for t in (ball, log, cube):
        assert (np.diff(t) < 0).all() and np.abs(np.diff(t) - np.diff(z)).max() <= G * DT * DT
    assert abs(ball[0] - (z[0] - 0.3)) <= 2e-3 and abs(log[0] - (z[0] - 0.2)) <= 2e-3 and abs(cube[0] - (z[0] - 0.3)) <= 2e-3


def test_group_members_read_their_own_scene(out):
    za, ta, zb, tb = out["group"]
    assert ta == za and tb == zb and za < 1.2 < zb < 1.8
    # b sat one of the ten steps out: nine steps of free fall against ten
    da, db = (1.2 - za) / (G * DT * DT), (1.8 - zb) / (G * DT * DT)
    assert 50 - 1e-6 <= da <= 55 + 1e-6 and 40.5 - 1e-6 <= db <= 45 + 1e-6
    assert abs(out["single"] - (2.0 - 0.2) / 2.0) <= 1e-3       # |d| = 2: t is in units of d
