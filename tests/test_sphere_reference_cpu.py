"""No GPU: the fp64 twin of the device's sphere narrow phase (sphere_twin.py) against the 50-digit reference
(sphere_reference.py) on every seeded family, and the reference against itself."""
import mpmath as mp
import numpy as np
import pytest

import sphere_reference as ref
import sphere_twin as twin
from collision_reference import TOL


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_twin_agrees_with_the_reference(name):
    """Normal, depth and position within TOL; contact / no contact exactly outside the guard bands; no property leaves
    out more than 10 % of the family (check_family asserts all three)."""
    f = ref.family(name)
    b0, b1, data = twin.contacts(f["pos"], f["R"], f["side"], f["shape"], pairs=f["pairs"] or [])
    worst, left_out = ref.check_family(name, b0, b1, data)
    print("%s: %d contacts, largest error %.3g, left out %s" % (name, len(b0), worst, left_out))
    assert worst <= TOL


def test_families_are_what_their_names_say():
    refs = {name: ref.family_reference(name) for name in ref.FAMILIES}
    for name in ("ground", "spheres", "face", "edge", "corner"):      # both decisions occur
        hits = sum(r["contact"] for r in refs[name])
        assert 8 <= hits <= ref.CASES - 8, (name, hits)
    assert not any(r["contact"] for r in refs["near_miss"])
    assert all(0 < r["s"] < 2e-3 for r in refs["near_miss"])
    assert all(r["inside"] and r["contact"] for r in refs["inside"])
    for name, region in (("face", 1), ("edge", 2), ("corner", 3)):
        f = ref.family(name)
        for i, j in f["pairs"]:
            s, b = (i, j) if f["shape"][i] == ref.SPHERE else (j, i)
            p = f["R"][b].reshape(3, 3).T @ (f["pos"][s] - f["pos"][b])
            assert (np.abs(p) > f["side"][b] / 2).sum() == region
    assert len({tuple(f) for f in ref.family("spheres")["side"][:, :1].reshape(-1, 2)}) == ref.CASES   # unequal radii
    f = ref.family("inside")
    assert all(len({*f["side"][b]}) == 3 for b in range(len(f["shape"])) if f["shape"][b] == ref.BOX)


def _close(a, b, eps=mp.mpf("1e-40")):
    with mp.workdps(ref.DPS):
        return all(abs(x - y) <= eps for x, y in zip(a, b))


def _neg(a):
    with mp.workdps(ref.DPS):
        return [-x for x in a]


@pytest.mark.parametrize("name", ["spheres", "face", "edge", "corner", "inside"])
def test_reference_swapping_the_bodies_negates_the_normal(name):
    f = ref.family(name)
    for i, j in f["pairs"][:16]:
        a = ref.pair(f["pos"], f["R"], f["side"], f["shape"], i, j)
        sw = [j, i]
        b = ref.pair(f["pos"][sw], f["R"][sw], f["side"][sw], f["shape"][sw], 0, 1)
        assert a["contact"] == b["contact"]
        assert _close(a["row"][:3], b["row"][:3]) and _close(a["row"][3:6], _neg(b["row"][3:6]))
        assert _close(a["row"][6:], b["row"][6:])


def test_reference_moves_with_a_rigid_motion_of_both_bodies():
    """Q from the quaternion (1, 2, 2, 4) / 5: rational entries, orthogonal to working precision."""
    with mp.workdps(ref.DPS):
        w, x, y, z = [mp.mpf(k) / 5 for k in (1, 2, 2, 4)]
        Q = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        t = [mp.mpf("0.3"), mp.mpf("-1.7"), mp.mpf("2.2")]
        rot = lambda v: [sum(Q[a][k] * v[k] for k in range(3)) for a in range(3)]
        move = lambda c: [a + b for a, b in zip(rot(ref._v(c)), t)]
        for name in ("face", "edge", "corner", "inside"):
            f = ref.family(name)
            for i, j in f["pairs"][:8]:
                s, b = (i, j) if f["shape"][i] == ref.SPHERE else (j, i)
                a = ref.sphere_box(f["pos"][s], f["side"][s][0], f["pos"][b], f["R"][b], f["side"][b])
                R = ref._v(f["R"][b])
                QR = [sum(Q[r][k] * R[3 * k + c] for k in range(3)) for r in range(3) for c in range(3)]
                m = ref.sphere_box(move(f["pos"][s]), f["side"][s][0], move(f["pos"][b]), QR, f["side"][b])
                assert _close(m["row"][:3], [u + v for u, v in zip(rot(a["row"][:3]), t)])
                assert _close(m["row"][3:6], rot(a["row"][3:6])) and _close(m["row"][6:], a["row"][6:])
        f = ref.family("spheres")
        for i, j in f["pairs"][:8]:
            a = ref.sphere_sphere(f["pos"][i], f["side"][i][0], f["pos"][j], f["side"][j][0])
            m = ref.sphere_sphere(move(f["pos"][i]), f["side"][i][0], move(f["pos"][j]), f["side"][j][0])
            assert _close(m["row"][:3], [u + v for u, v in zip(rot(a["row"][:3]), t)])
            assert _close(m["row"][3:6], rot(a["row"][3:6])) and _close(m["row"][6:], a["row"][6:])


def test_reference_depth_falls_by_t_along_the_normal():
    with mp.workdps(ref.DPS):
        t = mp.mpf("1e-3")
        for name in ("spheres", "face", "edge", "corner", "inside"):
            f = ref.family(name)
            for i, j in f["pairs"][:16]:
                a = ref.pair(f["pos"], f["R"], f["side"], f["shape"], i, j)
                if a["guard_n"]:
                    continue
                cj = [c + t * n for c, n in zip(ref._v(f["pos"][j]), a["row"][3:6])]    # body1 moves away along the normal
                if f["shape"][i] == ref.SPHERE and f["shape"][j] == ref.SPHERE:
                    b = ref.sphere_sphere(f["pos"][i], f["side"][i][0], cj, f["side"][j][0])
                elif f["shape"][i] == ref.SPHERE:
                    b = ref.sphere_box(f["pos"][i], f["side"][i][0], cj, f["R"][j], f["side"][j])
                else:
                    b = ref.sphere_box(cj, f["side"][j][0], f["pos"][i], f["R"][i], f["side"][i])
                # a box's R is orthonormal only to a few ulp, so its n_BS = R e / L has length 1 +- ~1e-15 and the
                # centre travels t (1 +- 1e-15) along it: 1e-14 t there, working precision between two spheres
                eps = mp.mpf("1e-40") if name == "spheres" else t * mp.mpf("1e-14")
                assert abs((a["row"][6] - b["row"][6]) - t) <= eps, name


def test_a_cube_in_the_spheres_place_is_not_a_sphere():
    """A (d, d, d) box where the sphere is gives another answer: a test that passes with the shape flag ignored would
    pass here too, and must not.  Sphere d = 0.3 at the origin, cube 0.3 at (0.25, 0.25, 0): the sphere touches the
    cube's vertical EDGE, normal along the diagonal, depth 0.15 - 0.1 sqrt(2); two cubes overlap by 0.05 along an axis."""
    from oracle import oracle as orc
    pos = np.array([[0.0, 0.0, 0.0], [0.25, 0.25, 0.0]])
    R = np.tile(np.eye(3).reshape(9), (2, 1))
    side = np.full((2, 3), 0.3)
    shape = np.array([ref.SPHERE, ref.BOX], np.int32)
    a = ref.pair(pos, R, side, shape)
    rows = twin.pair(pos, R, side, shape, 0, 1)
    assert ref.compare(a, rows, {}) <= TOL
    assert abs(rows[0][6] - (0.15 - 0.1 * np.sqrt(2.0))) < 1e-15
    assert np.allclose(rows[0][3:6], [np.sqrt(0.5), np.sqrt(0.5), 0.0], atol=1e-15)
    boxes, _ = orc.collide_boxes(pos[0], R[0], pos[1], R[1], side[0], side[1])
    assert all(abs(c[6] - rows[0][6]) > 1e-3 or np.abs(c[3:6] - rows[0][3:6]).max() > 0.1 for c in boxes)
    assert len(boxes) != 1 or np.abs(boxes[0][3:6] - rows[0][3:6]).max() > 0.1


def test_rolling_restatement_reaches_rolling():
    """The figures of DESIGN 6e: the one-contact step loop in fp64 and at 50 digits, 80 steps of the rolling-ball test.
    The loop reaches rolling (v = w r exactly once the friction row leaves its bound) and keeps m v r + I w about the
    contact point only as far as the lever arm rho = (z - r) - z is r."""
    r, v0, dt, erp, steps = 0.15, 0.7, 0.005, 0.2, 80
    x, z, vx, vz, wy = twin.ball_steps(r, 1.0, v0, steps, dt, erp)
    with mp.workdps(ref.DPS):
        X, Z, VX, VZ, WY = twin.ball_steps(r, 1.0, v0, steps, dt, erp, num=mp.mpf)
        d_fp = max(abs(mp.mpf(vx) - VX), abs(mp.mpf(wy) - WY) * mp.mpf(r))
        e_57, e_roll = abs(VX - mp.mpf(5) / 7 * mp.mpf(v0)), abs(VX - WY * mp.mpf(r))
    print("restatement: |v - 5/7 v0| = %.3g, |v - w r| = %.3g, fp64 vs mpmath = %.3g" % (float(e_57), float(e_roll), float(d_fp)))
    assert float(e_57) < 1e-9 and float(e_roll) < 1e-9 and float(d_fp) < 1e-13
