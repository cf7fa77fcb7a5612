"""GPU (-m gpu): Body::Sphere of the reference-shaped C++ API (eggshell_amd/host), driven by `sphere_demo`: the adapter's
ball on the ground and ball on a cube are the same bodies through the C ABI bit for bit, and an EnsembleGroup of a ball
ensemble and a cube ensemble leaves what its members leave when stepped alone."""
import json
import os
import subprocess

import numpy as np
import pytest

from eggshell_amd import capi

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "sphere_demo")


def run(*args):
    if not os.path.exists(DEMO):
        pytest.fail("sphere_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO, *args], check=True, capture_output=True, text=True, timeout=120)
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def out():
    return run()


@pytest.mark.parametrize("scene", ["ball_ground", "ball_on_cube"])
def test_adapter_scene_is_the_c_abi_bit_for_bit(ctx, out, scene):
    s = out[scene]
    a = lambda k, *shape: np.array(s[k], np.float64).reshape(*shape)
    n = len(s["shape"])
    shape = np.array(s["shape"], np.int32)
    assert (shape == capi.SHAPE_SPHERE).any()
    side = a("side", n, 3)
    assert (side[shape == 1] == 0.3).all()                       # (2r, 2r, 2r) with r = 0.15
    assert np.allclose(a("Minv", n, 36)[shape == 1][:, [21, 28, 35]], 1.0 / (0.4 * 1.0 * 0.15 * 0.15), rtol=1e-14, atol=0)   # I = (2/5) m r^2
    w = capi.World(ctx, n)
    w.set_bodies(a("p0", n, 3), np.tile(np.eye(3).reshape(9), (n, 1)), np.zeros((n, 3)), np.zeros((n, 3)), a("Minv", n, 36),
                 a("f_ext", n, 6), side=side)
    w.set_shapes(shape)
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01, omega=1.5)
    for _ in range(s["steps"]):
        w.step(5e-3, 0.2, prm)
    p, R, v, wv = w.bodies()
    b0, b1, data = w.contacts()
    for got, key, cols in ((p, "p", 3), (R, "R", 9), (v, "v", 3), (wv, "w", 3)):
        assert got.tobytes() == a(key, n, cols).tobytes(), key
    assert len(b0) > 0
    assert np.array_equal(b0, np.array(s["contact_b0"], np.int32)) and np.array_equal(b1, np.array(s["contact_b1"], np.int32))
    assert data[:, :3].tobytes() == a("contact_pos", len(b0), 3).tobytes()
    assert w.lambda_().tobytes() == a("lambda", 3 * len(b0)).tobytes()
    if scene == "ball_on_cube":
        assert ((b0 == 0) & (b1 == 1)).sum() == 1 and ((b0 == -1) & (b1 == 0)).sum() == 4
    w.close()


def test_group_equals_its_members_stepped_alone(out):
    g = out["group"]
    assert g["max_abs_diff"] == 0.0
    assert g["world_ensembles"] == 2
    assert g["contacts_balls_first"] == 3                                 # two on the ground, one between the balls
    assert g["contacts_balls"] == g["contacts_balls_alone"] >= 2          # (which the erp term may have pushed apart)
    assert g["contacts_cubes"] == g["contacts_cubes_alone"] > 8


def test_sphere_ensemble_without_detection_is_refused():
    res = run("--refuse")            # exit status 0: the refusal is EGS_ERR_UNSUPPORTED
    assert res["refused"] == capi.ERR_UNSUPPORTED and "detect_contacts" in res["message"]
