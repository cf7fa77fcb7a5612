"""GPU (-m gpu): the sphere narrow phase of collide.hip through egs_update_contacts_shapes -- bit for bit the fp64 twin
(sphere_twin.py), within TOL of the 50-digit reference (sphere_reference.py), and nothing changed for boxes."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import sphere_reference as ref
import sphere_twin as twin
from collision_reference import TOL
from eggshell_amd import capi, scenes

pytestmark = pytest.mark.gpu

BOX, SPHERE = capi.SHAPE_BOX, capi.SHAPE_SPHERE


def same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_family_is_the_twin_bit_for_bit_and_the_reference_within_tol(ctx, name):
    """64 disjoint cases in one call: count, order, body0 / body1 and all seven values equal the twin's bits; the
    device's own output passes the reference comparison of the CPU test."""
    f = ref.family(name)
    got = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"])
    want = twin.contacts(f["pos"], f["R"], f["side"], f["shape"], pairs=f["pairs"] or [])
    assert same(got, want)
    assert got[2].tobytes() == want[2].tobytes()          # -0.0 and 0.0 are different bits
    worst, left_out = ref.check_family(name, *got)
    print("%s: %d contacts, largest error %.3g, left out %s" % (name, len(got[0]), worst, left_out))
    assert worst <= TOL


def test_all_boxes_is_update_contacts_joints(ctx):
    """32 rotated unequal boxes, some on the ground, some touching: shape = NULL and shape = all EGS_SHAPE_BOX (which
    runs the SHAPES = true kernels) both give the bits of egs_update_contacts_joints."""
    rng = np.random.default_rng(41)
    n = 32
    p = rng.uniform([-0.6, -0.6, 0.05], [0.6, 0.6, 0.7], (n, 3))
    R = Rotation.random(n, random_state=41).as_matrix().reshape(n, 9)
    side = rng.uniform(0.15, 0.45, (n, 3))
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)))
    base = ctx.update_contacts(p, R, side=side, joints=none)
    assert (base[0] >= 0).sum() > 20 and (base[0] < 0).sum() > 4
    assert same(ctx.update_contacts_shapes(p, R, side, None), base)
    assert same(ctx.update_contacts_shapes(p, R, side, np.zeros(n, np.int32)), base)


def mixed_scene():
    """6 boxes (even bodies) and 6 spheres (odd) in one loose heap: some on the ground, some touching."""
    rng = np.random.default_rng(7)
    n = 12
    shape = np.array([BOX, SPHERE] * 6, np.int32)
    p = np.array([[0.32 * (k % 4), 0.26 * (k // 4), 0.14 + 0.05 * (k % 3)] for k in range(n)]) + rng.uniform(-0.02, 0.02, (n, 3))
    R = Rotation.random(n, random_state=7).as_matrix().reshape(n, 9)
    side = rng.uniform(0.22, 0.36, (n, 3))
    side[shape == SPHERE] = side[shape == SPHERE][:, :1]
    return p, R, side, shape


def test_mixed_scene_order_and_box_pairs(ctx):
    p, R, side, shape = mixed_scene()
    b0, b1, data = ctx.update_contacts_shapes(p, R, side, shape)
    assert same((b0, b1, data), twin.contacts(p, R, side, shape))
    g = int((b0 < 0).sum())
    assert g > 0 and (b0[:g] == -1).all() and (b0[g:] >= 0).all()            # ground first ...
    assert (np.diff(b1[:g]) >= 0).all()                                          # ... by body
    keys = b0[g:].astype(np.int64) * 100 + b1[g:]
    assert (b0[g:] < b1[g:]).all() and (np.diff(keys) >= 0).all()               # then pairs i < j
    kinds = set()
    for i, j in {(int(a), int(b)) for a, b in zip(b0[g:], b1[g:])}:
        sel = (b0 == i) & (b1 == j)
        kinds.add((int(shape[i]), int(shape[j])))
        if shape[i] == SPHERE or shape[j] == SPHERE:
            assert sel.sum() == 1
        else:   # the box-only call on those two bodies
            c0, c1, cd = ctx.update_contacts(p[[i, j]], R[[i, j]], side=side[[i, j]])
            assert np.array_equal(cd[c0 >= 0], data[sel])
    assert kinds == {(BOX, BOX), (BOX, SPHERE), (SPHERE, BOX), (SPHERE, SPHERE)}
    for b in np.flatnonzero(shape == SPHERE):
        assert ((b0 == -1) & (b1 == b)).sum() <= 1
    assert ((b0 == -1) & (shape[b1] == SPHERE)).any() and ((b0 == -1) & (shape[b1] == BOX)).any()


def test_both_broad_phases_on_balls_on_a_plate(ctx, monkeypatch):
    """200 small balls in contact with each other on a big plate (body 0, more than 64 partners: the uncapped
    candidate pass too): the all-pairs scan and the uniform grid give the same list."""
    sc = scenes.ball_pile(20, 10, 1, radius=0.05, sink=1e-3, gap=-1e-3)
    n = 201
    p = np.vstack([[[0.95, 0.45, 0.049]], sc["p"] + [0.0, 0.0, 0.098]])   # plate 1 mm in the ground, balls 2 mm in the plate
    R = np.tile(np.eye(3).reshape(9), (n, 1))
    side = np.vstack([[[2.4, 1.4, 0.1]], sc["side"]])
    shape = np.concatenate([[BOX], sc["shape"]]).astype(np.int32)
    out = {}
    for mode in ("pairs", "grid"):
        monkeypatch.setenv("EGS_BROADPHASE", mode)
        out[mode] = ctx.update_contacts_shapes(p, R, side, shape)
    assert same(out["pairs"], out["grid"])
    b0, b1, _ = out["grid"]
    assert ((b0 == 0) & (b1 > 0)).sum() == 200                       # every ball rests on the plate
    assert (b0 > 0).sum() == 19 * 10 + 20 * 9                        # and touches its grid neighbours
    assert (b0 == -1).sum() == 4                                     # the plate's lower corners are in the ground


def test_a_joint_at_the_contact_point_removes_that_contact_only(ctx):
    f = ref.family("face")
    base = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"])
    k = 5
    i, j = int(base[0][k]), int(base[1][k])
    at = base[2][k, :3]
    loc = lambda b: f["R"][b].reshape(3, 3).T @ (at - f["pos"][b])
    jd = np.concatenate([loc(i), loc(j), [0.0]]).reshape(1, 7)
    # the joint's position (p0 + R0 c0 + p1 + R1 c1) / 2 is within rounding of the contact, far inside the 1e-6
    got = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"], joints=([i], [j], jd))
    keep = np.arange(len(base[0])) != k
    assert same(got, tuple(a[keep] for a in base))
    # the same joint between two OTHER bodies prunes nothing
    i2, j2 = int(base[0][k + 1]), int(base[1][k + 1])
    got = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"], joints=([i2], [j2], jd))
    assert same(got, base)


@pytest.mark.parametrize("what", ["unknown", "unequal", "zero", "negative"])
def test_refusals_leave_the_world_unchanged(ctx, what):
    sc = scenes.ball_pile(2, 1, 1)
    shape, side = sc["shape"].copy(), sc["side"].copy()
    if what == "unknown":
        shape[1] = 2
    elif what == "unequal":
        side[1] = [0.3, 0.3, 0.2]
    else:
        side[1] = 0.0 if what == "zero" else -0.3
    with pytest.raises(capi.EgsError) as e:
        ctx.update_contacts_shapes(sc["p"], sc["R"], side, shape)
    assert e.value.status == capi.ERR_INVALID
    from oracle import oracle as orc
    Minv = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    prm = capi.params(method=capi.SOR)

    def run(w):
        w.step(5e-3, 0.2, prm)
        return w.bodies() + w.contacts()

    good = capi.World(ctx, 2)
    good.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=sc["side"])
    good.set_shapes(sc["shape"])
    # shapes first, then sides that do not fit (set_bodies refuses); or sides first, then shapes that do not fit
    w = capi.World(ctx, 2)
    w.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=sc["side"])
    w.set_shapes(sc["shape"])
    with pytest.raises(capi.EgsError) as e:
        if what == "unknown":
            w.set_shapes(shape)
        else:
            w.set_bodies(sc["p"] + 1.0, sc["R"], sc["v"], sc["w"], Minv, f_ext, side=side)
    assert e.value.status == capi.ERR_INVALID
    want = run(good)
    assert all(np.array_equal(a, b) for a, b in zip(run(w), want))
    w2 = capi.World(ctx, 2)
    w2.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=sc["side"] if what == "unknown" else side)
    with pytest.raises(capi.EgsError) as e:
        w2.set_shapes(shape)
    assert e.value.status == capi.ERR_INVALID
    if what == "unknown":      # still a box world: the step of a fresh box world
        fresh = capi.World(ctx, 2)
        fresh.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=sc["side"])
        assert all(np.array_equal(a, b) for a, b in zip(run(w2), run(fresh)))
    for x in (good, w, w2):
        x.close()
