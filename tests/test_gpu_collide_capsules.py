"""GPU (-m gpu): the capsule narrow phase of collide.hip through egs_update_contacts_shapes -- bit for bit the fp64 twin
(capsule_twin.py), within TOL of the 50-digit reference (capsule_reference.py), and nothing changed for boxes and
spheres."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import capsule_reference as ref
import capsule_twin as twin
from collision_reference import TOL
from eggshell_amd import capi, scenes

pytestmark = pytest.mark.gpu

BOX, SPHERE, CAPSULE = capi.SHAPE_BOX, capi.SHAPE_SPHERE, capi.SHAPE_CAPSULE


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


def test_two_families_in_one_call(ctx):
    """crossed and box_edge side by side, 128 pairs: narrow_kernel's second block."""
    fa, fb = ref.family("crossed"), ref.family("box_edge")
    shift = np.array([0.0, 4.0, 0.0])
    pos = np.vstack([fa["pos"], fb["pos"] + shift])
    R, side = np.vstack([fa["R"], fb["R"]]), np.vstack([fa["side"], fb["side"]])
    shape = np.concatenate([fa["shape"], fb["shape"]])
    n = len(fa["shape"])
    pairs = fa["pairs"] + [(i + n, j + n) for i, j in fb["pairs"]]
    got = ctx.update_contacts_shapes(pos, R, side, shape)
    want = twin.contacts(pos, R, side, shape, pairs=pairs)
    assert len(pairs) > 64 and same(got, want) and got[2].tobytes() == want[2].tobytes()
    assert (got[0] < n).any() and (got[0] >= n).any()


def mixed_scene():
    """4 boxes, 4 spheres and 4 capsules in one loose heap, like beside like and beside unlike: some on the ground,
    some touching."""
    rng = np.random.default_rng(5)
    n = 12
    shape = np.array([BOX, BOX, SPHERE, SPHERE, CAPSULE, CAPSULE, BOX, SPHERE, CAPSULE, SPHERE, BOX, CAPSULE], np.int32)
    p = np.array([[0.3 * (k % 4), 0.24 * (k // 4), 0.13 + 0.05 * (k % 3)] for k in range(n)]) + rng.uniform(-0.02, 0.02, (n, 3))
    R = Rotation.random(n, random_state=5).as_matrix().reshape(n, 9)
    side = rng.uniform(0.22, 0.36, (n, 3))
    side[shape == SPHERE] = side[shape == SPHERE][:, :1]
    side[shape == CAPSULE] = np.array([0.2, 0.2, 0.55]) + rng.uniform(0, 0.05, (4, 1)) * [1, 1, 2]
    return p, R, side, shape


def test_mixed_scene_order_caps_and_untouched_pairs(ctx):
    p, R, side, shape = mixed_scene()
    b0, b1, data = ctx.update_contacts_shapes(p, R, side, shape)
    want = twin.contacts(p, R, side, shape)
    assert same((b0, b1, data), want) and data.tobytes() == want[2].tobytes()
    g = int((b0 < 0).sum())
    assert g > 0 and (b0[:g] == -1).all() and (b0[g:] >= 0).all()            # ground first ...
    assert (np.diff(b1[:g]) >= 0).all()                                          # ... by body
    keys = b0[g:].astype(np.int64) * 100 + b1[g:]
    assert (b0[g:] < b1[g:]).all() and (np.diff(keys) >= 0).all()               # then pairs i < j
    keep = np.flatnonzero(shape != CAPSULE)                                      # the call with the capsules removed
    back = {int(b): k for k, b in enumerate(keep)}
    n0, n1, nd = ctx.update_contacts_shapes(p[keep], R[keep], side[keep], shape[keep])
    kinds = set()
    for i, j in sorted({(int(a), int(b)) for a, b in zip(b0[g:], b1[g:])}):
        sel = (b0 == i) & (b1 == j)
        kind = tuple(sorted((int(shape[i]), int(shape[j]))))
        kinds.add(kind)
        if CAPSULE in kind:
            assert sel.sum() <= {BOX: 3, SPHERE: 1, CAPSULE: 5}[kind[0]]
            continue
        assert data[sel].tobytes() == nd[(n0 == back[i]) & (n1 == back[j])].tobytes()
        if kind == (BOX, BOX):   # the box-only call on those two bodies
            c0, c1, cd = ctx.update_contacts(p[[i, j]], R[[i, j]], side=side[[i, j]])
            assert np.array_equal(cd[c0 >= 0], data[sel])
        else:
            assert sel.sum() == 1
    assert kinds == {(BOX, BOX), (BOX, SPHERE), (SPHERE, SPHERE), (BOX, CAPSULE), (SPHERE, CAPSULE), (CAPSULE, CAPSULE)}
    for b in range(len(shape)):
        sel = (b0 == -1) & (b1 == b)
        assert sel.sum() <= {BOX: 8, SPHERE: 1, CAPSULE: 2}[int(shape[b])]
        if shape[b] != CAPSULE:
            assert data[sel].tobytes() == nd[(n0 == -1) & (n1 == back[b])].tobytes()
    assert all(((b0 == -1) & (shape[b1] == s)).any() for s in (BOX, SPHERE, CAPSULE))


def test_both_broad_phases_on_a_log_pile(ctx, monkeypatch):
    """A crib of 96 logs, 8 layers of 12, each layer 1 mm into the one below: the all-pairs scan and the uniform grid
    give the same list, and every log rests on every log below it."""
    sc = scenes.log_pile(1, 12, 8, radius=0.05, length=1.4, sink=1e-3, gap=0.01)
    out = {}
    for mode in ("pairs", "grid"):
        monkeypatch.setenv("EGS_BROADPHASE", mode)
        out[mode] = ctx.update_contacts_shapes(sc["p"], sc["R"], sc["side"], sc["shape"])
    assert same(out["pairs"], out["grid"]) and out["pairs"][2].tobytes() == out["grid"][2].tobytes()
    want = twin.contacts(sc["p"], sc["R"], sc["side"], sc["shape"])
    assert same(out["grid"], want) and out["grid"][2].tobytes() == want[2].tobytes()
    b0, b1, _ = out["grid"]
    assert (b0 == -1).sum() == 2 * 12                         # the lowest layer lies in the ground: two contacts a log
    assert (b0 >= 0).sum() == 7 * 12 * 12                      # crossed pairs between neighbouring layers, one each
    assert ((b1[b0 >= 0] // 12) - (b0[b0 >= 0] // 12) == 1).all()


def test_a_joint_at_the_contact_point_removes_that_contact_only(ctx):
    f = ref.family("box_flat")            # two contacts per pair: the joint takes one of them
    base = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"])
    k = 4
    i, j = int(base[0][k]), int(base[1][k])
    assert ((base[0] == i) & (base[1] == j)).sum() == 2
    at = base[2][k, :3]
    loc = lambda b: f["R"][b].reshape(3, 3).T @ (at - f["pos"][b])
    jd = np.concatenate([loc(i), loc(j), [0.0]]).reshape(1, 7)
    got = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"], joints=([i], [j], jd))
    keep = np.arange(len(base[0])) != k
    assert same(got, tuple(a[keep] for a in base))
    others = np.flatnonzero((base[0] != i) & (base[0] >= 0))
    i2, j2 = int(base[0][others[0]]), int(base[1][others[0]])
    got = ctx.update_contacts_shapes(f["pos"], f["R"], f["side"], f["shape"], joints=([i2], [j2], jd))
    assert same(got, base)


BAD_ROWS = {"sphere_row": [0.2, 0.2, 0.2], "shorter": [0.2, 0.2, 0.1], "unequal": [0.2, 0.25, 0.6], "zero": [0.0, 0.0, 0.6],
            "negative": [-0.2, -0.2, 0.6], "inf": [0.2, 0.2, np.inf], "nan": [np.nan, np.nan, 0.6]}


@pytest.mark.parametrize("what", sorted(BAD_ROWS))
def test_refusals_leave_the_world_unchanged(ctx, what):
    sc = scenes.log_pile(1, 2, 1)
    side = sc["side"].copy()
    side[1] = BAD_ROWS[what]
    with pytest.raises(capi.EgsError) as e:
        ctx.update_contacts_shapes(sc["p"], sc["R"], side, sc["shape"])
    assert e.value.status == capi.ERR_INVALID
    if what == "sphere_row":
        assert "EGS_SHAPE_SPHERE" in str(e.value)
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
    w = capi.World(ctx, 2)                # shapes in force, then sides that do not fit: set_bodies refuses
    w.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=sc["side"])
    w.set_shapes(sc["shape"])
    with pytest.raises(capi.EgsError) as e:
        w.set_bodies(sc["p"] + 1.0, sc["R"], sc["v"], sc["w"], Minv, f_ext, side=side)
    assert e.value.status == capi.ERR_INVALID
    want = run(good)
    assert len(want[4]) == 4
    assert all(np.array_equal(a, b) for a, b in zip(run(w), want))
    w2 = capi.World(ctx, 2)               # sides first, then shapes that do not fit: still a box world
    w2.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=side)
    with pytest.raises(capi.EgsError) as e:
        w2.set_shapes(sc["shape"])
    assert e.value.status == capi.ERR_INVALID
    for x in (good, w, w2):
        x.close()
