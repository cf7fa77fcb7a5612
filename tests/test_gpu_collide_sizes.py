"""GPU (-m gpu): the device collider on rotated boxes that are NOT cubes of side 0.3.  collide.hip indexes half-extents
by hand in the fifteen axis tests, the choice of the incident face, the clipping slabs, the ground corners and the broad
phase's radii; with three equal half-extents every slip among them gives the right answer.  Here the sides are unequal:

  * bit for bit against the oracle's list (indices, order, seven values per contact) on the five seeded families of
    tests/collision_reference.py, in both broad phases;
  * the device's own list against the 50-digit statement of the geometry (same properties, tolerance and caps as the
    oracle meets in tests/test_collision_reference_cpu.py); run with -s for the measured errors and counts;
  * broad phase with very unequal radii, with and without the more-than-64-partners spill;
  * the same pair listed in both orders;
  * the world and the batched world with heterogeneous side lengths."""
import functools

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import collision_reference as ref
from eggshell_amd import capi
from oracle import oracle as orc
from test_gpu_collide import reference_contacts

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle_list(f):
    return reference_contacts(*ref.family(f))


def assert_same_list(got, want, what=""):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what


@pytest.mark.parametrize("mode", ["pairs", "grid"])
@pytest.mark.parametrize("f", ref.FAMILIES)
def test_families_equal_the_oracle_bit_for_bit(ctx, monkeypatch, f, mode):
    monkeypatch.setenv("EGS_BROADPHASE", mode)
    p, R, side = ref.family(f)
    want = oracle_list(f)
    assert (want[0] >= 0).sum() > 300 and (want[0] < 0).sum() > 20
    assert_same_list(ctx.update_contacts(p, R, side), want, (f, mode))


@pytest.mark.parametrize("f", ref.FAMILIES)
def test_families_against_the_50_digit_reference(ctx, f):
    """The device's own contact list: a pair it omits is separated, a pair it reports collides, and every contact has
    the properties the mathematics states, at 1e-12, with the exclusion caps as a condition."""
    p, R, side = ref.family(f)
    b0, b1, data = ctx.update_contacts(p, R, side)
    tally = ref.Tally()
    ref.check_scene(ref.family_reference(f), b0, b1, data, tally, "family %d" % f)
    print("\n" + tally.line("device, family %d" % f))
    tally.assert_caps(f)


def partners(p, side):
    """Per body i, how many j > i pass the broad phase's bounding-sphere test (more than 64: the spill path)."""
    r = 0.5 * np.linalg.norm(side, axis=1)
    d = np.linalg.norm(p[:, None, :] - p[None, :, :], axis=2)
    hit = d <= (r[:, None] + r[None, :]) * 1.0000001 + 1e-12
    return np.triu(hit, 1).sum(axis=1)


@pytest.mark.parametrize("large_first", [False, True])
def test_broad_phase_with_unequal_radii(ctx, monkeypatch, large_first):
    """300 rotated bodies, four of them ten times the size of the rest: the grid's cell edge comes from the large ones,
    so hundreds of small bodies share a bucket.  Large bodies last: every candidate list stays short.  Large bodies
    first: each has more than 64 partners j > i, the uncapped spill pass runs with non-cubes.  grid == pairs == oracle."""
    rng = np.random.default_rng(7200 + int(large_first))
    n = 300
    p = rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 1.0], (n, 3))
    R = Rotation.from_quat(rng.normal(size=(n, 4))).as_matrix().reshape(n, 9)
    side = rng.uniform(0.05, 0.25, (n, 3))
    large = slice(0, 4) if large_first else slice(n - 4, n)
    side[large] = rng.uniform(1.5, 2.5, (4, 3))
    k = partners(p, side)
    if large_first:
        assert (k[large] > 80).all(), k[large]
    else:
        assert k.max() < 48, k.max()
    want = reference_contacts(p, R, side)
    big = np.arange(n)[large]
    assert (np.isin(want[0], big) | np.isin(want[1], big)).sum() > 100      # the large bodies do collide with the rest
    for mode in ("pairs", "grid"):
        monkeypatch.setenv("EGS_BROADPHASE", mode)
        assert_same_list(ctx.update_contacts(p, R, side), want, mode)


def test_pair_order_matters(ctx):
    """The same two unequal, rotated boxes as (i, j) and as (j, i): box 1 and box 2 swap roles, and with them the
    codes 1-3 and 4-6 and the sign of the normal.  Each order equals the oracle for that order.  Four seeded pairs
    for each of: a face of the first box, a face of the second, an edge pair."""
    rng = np.random.default_rng(7300)
    group = lambda code: 0 if 1 <= code <= 3 else 1 if 4 <= code <= 6 else 2 if 7 <= code <= 15 else None
    picked = {0: [], 1: [], 2: []}
    while min(len(v) for v in picked.values()) < 4:
        p = rng.uniform(-0.2, 0.2, (2, 3)) + [0.0, 0.0, 3.0]
        R = Rotation.from_quat(rng.normal(size=(2, 4))).as_matrix().reshape(2, 9)
        side = rng.uniform(0.08, 0.6, (2, 3))
        g = group(orc.collide_boxes(p[0], R[0], p[1], R[1], side[0], side[1])[1])
        if g is not None and len(picked[g]) < 4:
            picked[g].append((p, R, side))
    cases = [c for g in (0, 1, 2) for c in picked[g]]
    lists = []
    for order in ([0, 1], [1, 0]):      # all twelve pairs in one scene, 5 apart, in one order and in the other
        p = np.concatenate([c[0][order] + [5.0 * k, 0.0, 0.0] for k, c in enumerate(cases)])
        R = np.concatenate([c[1][order] for c in cases])
        side = np.concatenate([c[2][order] for c in cases])
        want = reference_contacts(p, R, side)
        assert_same_list(ctx.update_contacts(p, R, side), want, order)
        assert len(np.unique(want[0])) == len(cases)
        codes = [orc.collide_boxes(p[2 * k], R[2 * k], p[2 * k + 1], R[2 * k + 1], side[2 * k], side[2 * k + 1])[1]
                 for k in range(len(cases))]
        lists.append((want, codes))
    (fwd, cf), (rev, cr) = lists
    assert [group(c) for c in cf] == [0] * 4 + [1] * 4 + [2] * 4
    assert [group(c) for c in cr] == [1] * 4 + [0] * 4 + [2] * 4
    for k in range(len(cases)):         # one common normal per pair; it points from the first box listed to the second
        nf, nr = fwd[2][fwd[0] == 2 * k][0, 3:6], rev[2][rev[0] == 2 * k][0, 3:6]
        assert np.abs(nf + nr).max() < 1e-12, k


def cloud(n, side, seed):
    """n bodies of the given side lengths in a loose cloud above the ground, at rest: a scene dict as scenes.* give."""
    rng = np.random.default_rng(seed)
    p = rng.uniform([-0.7, -0.7, 0.1], [0.7, 0.7, 1.3], (n, 3))
    R = Rotation.from_quat(rng.normal(size=(n, 4))).as_matrix().reshape(n, 9)
    return dict(p=p, R=R, v=np.zeros((n, 3)), w=np.zeros((n, 3)), mass=np.ones(n),
                I_body=np.tile((np.eye(3) * 0.1).reshape(9), (n, 1)), side=np.array(side[:n]))


@pytest.mark.parametrize("precision", [capi.F64, capi.F32])
def test_world_step_with_unequal_sides_equals_problem_step(ctx, precision):
    """test_gpu_world.test_world_step_equals_problem_step with family 0's side lengths: the world's collider sees the
    sides given to set_bodies, and the step built on its contacts equals the pieces called one by one."""
    sc = cloud(30, ref.family(0)[2], 7400)
    n, side = 30, sc["side"]
    Minv = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=40, tol=0.0, cfm=0.01)
    wd = capi.World(ctx, n, precision)
    wd.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext, side=side)
    pos, R, v, w = sc["p"], sc["R"], sc["v"], sc["w"]
    try:
        for step in range(3):
            wd.step(0.005, 0.2, prm)
            b0, b1, data = ctx.update_contacts(pos, R, side)
            assert (b0 >= 0).sum() > 10 and (b0 < 0).sum() > 0
            c0, c1, cd = ctx.update_contacts(pos, R)
            assert len(c0) != len(b0) or not np.array_equal(cd, data)     # cubes of 0.3 would give another list
            assert_same_list(wd.contacts(), (b0, b1, data), step)
            pr = capi.Problem(ctx, n, b0, b1, precision)
            pr.set_state(pos, R, v, w, Minv, f_ext)
            pr.set_constraints(np.full(len(b0), capi.CONTACT_BOX, np.int32), data)
            pr.step(0.005, 0.2, prm)
            assert np.array_equal(wd.lambda_(), pr.lambda_()), step
            pr.advance(0.005)
            pos, R, v, w = pr.state()
            pr.close()
            assert np.isfinite(pos).all() and np.isfinite(v).all()
            for a, b in zip(wd.bodies(), (pos, R, v, w)):
                assert np.array_equal(a, b), step
    finally:
        wd.close()


def test_batched_world_with_unequal_sides(ctx):
    """Three ensembles in one batched world -- cubes of 0.3, family 0's sides, family 4's (thin and long) sides: after
    each of three steps every ensemble has the bits of a world that holds it alone."""
    from test_gpu_world_batch import ensemble, run_against_singles
    ens = []
    for side, seed in ((np.full((30, 3), 0.3), 7500), (ref.family(0)[2], 7501), (ref.family(4)[2], 7502)):
        sc = cloud(30, side, seed)
        e = ensemble(sc)
        e["side"] = sc["side"]
        ens.append(e)
    ens[0]["side"] = None       # the default of set_bodies, next to explicit sides
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=40, tol=0.0, cfm=0.01)
    seen = []

    def contacts_present(step, bw, off, info, bst):
        seen.append(np.diff(info["contact_offset"]))

    run_against_singles(ctx, ens, prm, 3, after_step=contacts_present)
    assert (np.array(seen) > 10).all(), seen
