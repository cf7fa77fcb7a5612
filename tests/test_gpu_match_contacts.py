"""GPU (-m gpu): egs_match_contacts (eggshell_amd/csrc/warm_start.hip) against the numpy matcher of
tests/warm_start_reference.py on synthetic lists: x0 and source exactly equal."""
import numpy as np
import pytest

import warm_start_reference as wsr
from eggshell_amd import capi

pytestmark = pytest.mark.gpu

Q = 2.0 ** -10      # positions are small integers times this: squared distances are exact


def sorted_list(rng, m, n_bodies, span=6):
    """m contacts in the collider's order: (b0, b1) ascending with the ground (-1) first, b0 < b1."""
    b0 = rng.integers(-1, n_bodies - 1, m)
    b1 = np.array([rng.integers(a + 1, n_bodies) for a in b0], np.int64) if m else np.zeros(0, np.int64)
    order = np.lexsort((b1, b0))
    pos = rng.integers(-span, span + 1, (m, 3)).astype(np.float64) * Q
    return b0[order].astype(np.int32), b1[order].astype(np.int32), pos


def both(ctx, old, new, off_old, off_new, valid, radius):
    ob0, ob1, opos, olam = old
    nb0, nb1, npos, nrhs = new
    want = wsr.match_contacts(ob0, ob1, opos, olam, off_old, valid, nb0, nb1, npos, nrhs, off_new, radius)
    got = ctx.match_contacts(ob0, ob1, opos, olam, off_old, valid, nb0, nb1, npos, nrhs, off_new, radius)
    assert np.array_equal(got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes()        # bits: -0.0 and denormals included
    return got


@pytest.mark.parametrize("m_old", [0, 1, 63, 64, 65, 257])
def test_random_lists(ctx, m_old):
    rng = np.random.default_rng(200 + m_old)
    for m_new in (0, 1, 63, 64, 65, 257):
        for n_bodies, radius in ((3, 4 * Q), (9, 7 * Q), (40, 100.0)):
            ob0, ob1, opos = sorted_list(rng, m_old, n_bodies)
            nb0, nb1, npos = sorted_list(rng, m_new, n_bodies)
            olam, nrhs = rng.uniform(-1, 1, 3 * m_old), rng.uniform(-1, 1, 3 * m_new)
            x0, src = both(ctx, (ob0, ob1, opos, olam), (nb0, nb1, npos, nrhs), [0, m_old], [0, m_new], [1], radius)
            if m_old >= 63 and m_new >= 63 and n_bodies == 3:
                assert (src >= 0).any() and (src == -1).any()


def test_pairs_present_on_one_side_only_and_a_long_run(ctx):
    # old: pair (0, 1) eight times, pair (1, 2) once; new: pair (0, 1) twice, pair (0, 2) once (not in the old list)
    ob0 = np.array([0] * 8 + [1], np.int32); ob1 = np.array([1] * 8 + [2], np.int32)
    opos = np.array([[k, 0, 0] for k in range(8)] + [[0, 0, 0]], np.float64) * Q
    olam = np.arange(27, dtype=np.float64)
    nb0 = np.array([0, 0, 0], np.int32); nb1 = np.array([1, 1, 2], np.int32)
    npos = np.array([[6, 1, 0], [2, 0, 1], [0, 0, 0]], np.float64) * Q
    x0, src = both(ctx, (ob0, ob1, opos, olam), (nb0, nb1, npos, -np.ones(9)), [0, 9], [0, 3], [1], 3 * Q)
    assert src.tolist() == [6, 2, -1]


def test_ties_radius_edge_and_shared_sources(ctx):
    ob0 = np.array([-1, -1, -1], np.int32); ob1 = np.array([0, 0, 0], np.int32)
    opos = np.array([[4, 0, 0], [-4, 0, 0], [0, 9, 0]], np.float64) * Q
    olam = np.array([1.0, 2, 3, 4, 5, 6, 7, 8, 9])
    nb0 = np.array([-1, -1, -1], np.int32); nb1 = np.array([0, 0, 0], np.int32)
    # an exact tie between old 0 and old 1; two new contacts next to old 2
    npos = np.array([[0, 0, 0], [0, 8, 0], [0, 10, 0]], np.float64) * Q
    x0, src = both(ctx, (ob0, ob1, opos, olam), (nb0, nb1, npos, np.zeros(9)), [0, 3], [0, 3], [1], 4 * Q)
    assert src.tolist() == [0, 2, 2]
    # exactly on the radius: taken; a radius one ulp smaller: not taken
    r = 4 * Q
    one = (ob0[:1], ob1[:1], opos[:1], olam[:3])
    new = (nb0[:1], nb1[:1], npos[:1], np.zeros(3))
    assert both(ctx, one, new, [0, 1], [0, 1], [1], r)[1].tolist() == [0]
    assert both(ctx, one, new, [0, 1], [0, 1], [1], np.nextafter(r, 0.0))[1].tolist() == [-1]
    # radius 0 with identical positions
    same = (nb0[:1], nb1[:1], opos[:1].copy(), np.zeros(3))
    x0, src = both(ctx, one, same, [0, 1], [0, 1], [1], 0.0)
    assert src.tolist() == [0] and np.array_equal(x0, olam[:3])


def test_three_ensembles_the_middle_one_empty_and_one_without_history(ctx):
    rng = np.random.default_rng(9)
    # ensembles 0 and 2 hold the same local list: a source must never cross an ensemble's border
    b0, b1, pos = sorted_list(rng, 5, 3)
    ob0, ob1, opos = np.tile(b0, 2), np.tile(b1, 2), np.tile(pos, (2, 1))
    olam = rng.uniform(-1, 1, 30)
    nrhs = rng.uniform(-1, 1, 30)
    for valid in ([1, 0, 1], [0, 1, 1], [1, 1, 0]):
        x0, src = both(ctx, (ob0, ob1, opos, olam), (ob0, ob1, opos, nrhs), [0, 5, 5, 10], [0, 5, 5, 10], valid, Q)
        for e, (lo, hi) in enumerate(((0, 5), (5, 5), (5, 10))):
            if hi > lo and valid[e]:
                assert ((src[lo:hi] >= lo) & (src[lo:hi] < hi)).all()
            elif hi > lo:
                assert (src[lo:hi] == -2).all() and np.array_equal(x0[3 * lo:3 * hi], nrhs[3 * lo:3 * hi])
    # an empty first and last ensemble
    both(ctx, (b0, b1, pos, olam[:15]), (b0, b1, pos, nrhs[:15]), [0, 0, 5, 5], [0, 0, 5, 5], [1, 1, 1], Q)


def test_signed_zeros_and_denormals_are_copied_bit_for_bit(ctx):
    ob0 = np.array([-1, 0], np.int32); ob1 = np.array([0, 1], np.int32)
    opos = np.zeros((2, 3))
    olam = np.array([-0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308 / 4, -0.0])
    x0, src = both(ctx, (ob0, ob1, opos, olam), (ob0, ob1, opos, np.ones(6)), [0, 2], [0, 2], [1], 0.0)
    assert src.tolist() == [0, 1] and x0.tobytes() == olam.tobytes()
    assert np.signbit(x0[0]) and not np.signbit(x0[1]) and x0[2] != 0.0


def test_refusals(ctx):
    z = np.zeros(0, np.int32)
    b = np.array([0], np.int32); c = np.array([1], np.int32)
    ok = (b, c, np.zeros(3), np.zeros(3))
    for args in ((ok, ok, [0, 1], [0, 1], [1], -1.0),              # radius < 0
                 (ok, ok, [0, 1], [0, 1], [1], float("nan")),
                 (ok, ok, [0, 2], [0, 1], [1], 1.0),               # offsets do not end at m
                 (ok, ok, [1, 1], [0, 1], [1], 1.0)):              # ... or start at 0
        with pytest.raises(capi.EgsError) as e:
            ctx.match_contacts(*args[0], args[2], args[4], *args[1], args[3], args[5])
        assert e.value.status == capi.ERR_INVALID
    unsorted = (np.array([1, 0], np.int32), np.array([2, 1], np.int32), np.zeros(6), np.zeros(6))
    with pytest.raises(capi.EgsError) as e:
        ctx.match_contacts(*unsorted, [0, 2], [1], *ok, [0, 1], 1.0)
    assert e.value.status == capi.ERR_INVALID
    x0, src = ctx.match_contacts(z, z, np.zeros(0), np.zeros(0), [0, 0], [1], z, z, np.zeros(0), np.zeros(0), [0, 0], 1.0)
    assert x0.size == 0 and src.size == 0
