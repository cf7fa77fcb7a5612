"""GPU (-m gpu): Body::Capsule of the reference-shaped C++ API (eggshell_amd/host), driven by `capsule_demo`: mass,
inertia and side row of the body, the adapter's scenes through the C ABI bit for bit, a lying capsule coming to rest."""
import json
import os
import subprocess

import numpy as np
import pytest

from eggshell_amd import capi, scenes

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "capsule_demo")
RAD, LEN, MASS = 0.1, 0.6, 2.0


def run(*args):
    if not os.path.exists(DEMO):
        pytest.fail("capsule_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO, *args], check=True, capture_output=True, text=True, timeout=120)
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def out():
    return run()


def test_mass_inertia_and_side_row(out):
    s = out["lying"]
    assert s["shape"] == [capi.SHAPE_CAPSULE] and s["mass"] == [MASS]
    assert s["side"] == [2 * RAD, 2 * RAD, LEN]
    ixx, izz = scenes.capsule_inertia(MASS, RAD, LEN)        # (checked against quadrature in the CPU test)
    I = np.array(s["I_body"]).reshape(3, 3)
    assert np.allclose(I, np.diag([ixx, ixx, izz]), rtol=1e-14, atol=0)
    # the body lies along x: its z axis is the world's x axis, so the world-frame inertia is diag(I_zz, I_xx, I_xx)
    Minv = np.array(s["Minv"]).reshape(6, 6)
    assert np.allclose(Minv, np.diag([1 / MASS] * 3 + [1 / izz, 1 / ixx, 1 / ixx]), rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("scene", ["lying", "on_cube"])
def test_adapter_scene_is_the_c_abi_bit_for_bit(ctx, out, scene):
    s = out[scene]
    a = lambda k, *shape: np.array(s[k], np.float64).reshape(*shape)
    n = len(s["shape"])
    shape = np.array(s["shape"], np.int32)
    w = capi.World(ctx, n)
    w.set_bodies(a("p0", n, 3), a("R0", n, 9), np.zeros((n, 3)), np.zeros((n, 3)), a("Minv", n, 36), a("f_ext", n, 6),
                 side=a("side", n, 3))
    w.set_shapes(shape)
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01, omega=1.5)
    for _ in range(s["steps"]):
        w.step(5e-3, 0.2, prm)
    p, R, v, wv = w.bodies()
    b0, b1, data = w.contacts()
    for got, key, cols in ((p, "p", 3), (R, "R", 9), (v, "v", 3), (wv, "w", 3)):
        assert got.tobytes() == a(key, n, cols).tobytes(), key
    assert np.array_equal(b0, np.array(s["contact_b0"], np.int32)) and np.array_equal(b1, np.array(s["contact_b1"], np.int32))
    assert data[:, :3].tobytes() == a("contact_pos", len(b0), 3).tobytes()
    assert w.lambda_().tobytes() == a("lambda", 3 * len(b0)).tobytes()
    if scene == "on_cube":
        assert ((b0 == -1) & (b1 == 0)).sum() == 4 and ((b0 == 0) & (b1 == 1)).sum() <= 1
    w.close()


def test_lying_capsule_comes_to_rest(out):
    """200 steps from 1 mm in the ground: within g dt^2 of z = r (the erp residue of the resting-ball test), and so is
    each end ball, which bounds the tilt: e |u_z| <= g dt^2 with e = 0.2.  Nothing acts sideways: the centre stays
    within 1e-6 of where it was (the solve stops at a residual of 1e-9)."""
    s = out["lying"]
    p, v, R = np.array(s["p"]), np.array(s["v"]), np.array(s["R"])
    assert abs(p[2] - RAD) <= 9.8 * 5e-3 * 5e-3
    assert abs(p[0]) <= 1e-6 and abs(p[1]) <= 1e-6 and 0.2 * abs(R[8]) <= 9.8 * 5e-3 * 5e-3 and abs(v[2]) <= 9.8 * 5e-3


def test_a_capsule_no_longer_than_its_diameter_is_refused():
    res = run("--refuse")            # exit status 0: the refusal is EGS_ERR_INVALID
    assert res["refused"] == capi.ERR_INVALID and "Body::Sphere" in res["message"]
