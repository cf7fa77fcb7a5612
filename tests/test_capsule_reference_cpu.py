"""The fp64 twin of the device's capsule geometry (capsule_twin.py) against the 50-digit reference
(capsule_reference.py) on every seeded family, and the solid capsule's inertia against quadrature.  No GPU."""
import itertools

import mpmath as mp
import numpy as np
import pytest

import capsule_reference as ref
import capsule_twin as twin
from collision_reference import TOL
from eggshell_amd import scenes


def test_sorting_network_sorts():
    """The fixed network of collide_capsule_box sorts every 0-1 input, hence every input."""
    for bits in itertools.product((0.0, 1.0), repeat=6):
        x = list(bits)
        for a, b in twin._NETWORK:
            x[a], x[b] = min(x[a], x[b]), max(x[a], x[b])
        assert x == sorted(x)


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_twin_within_tol_of_the_reference(name):
    f = ref.family(name)
    b0, b1, data = twin.contacts(f["pos"], f["R"], f["side"], f["shape"], pairs=f["pairs"] or [])
    worst, left_out = ref.check_family(name, b0, b1, data)
    print("capsule family %-12s contacts %3d  largest error %.3g  left out %s" % (name, len(b0), worst, left_out))
    assert worst <= TOL


def test_families_hold_what_they_are_named_for():
    """Contact counts that show each family reaches its case: two ground contacts when lying, one interior contact when
    crossed or on an edge, two when flat on a face, the interior point of a narrow box and of a pierced one."""
    def counts(name):
        f = ref.family(name)
        b0, b1, _ = twin.contacts(f["pos"], f["R"], f["side"], f["shape"], pairs=f["pairs"] or [])
        if name == "ground":
            return [int(((b0 == -1) & (b1 == k)).sum()) for k in range(ref.CASES)]
        return [int(((b0 == i) & (b1 == j)).sum()) for i, j in f["pairs"]]
    g = counts("ground")
    assert set(g) == {0, 1, 2} and g.count(2) >= 16
    for name in ("collinear", "box_end", "box_edge", "box_corner", "box_narrow", "cap_sphere"):
        c = counts(name)
        assert set(c) <= {0, 1} and c.count(1) >= 32, (name, c)
    for name in ("crossed", "tee"):     # a deep or short pair may add an end's contact to the one the family is about
        c = counts(name)
        assert c.count(1) >= 32 and max(c) <= 5, (name, c)
    assert set(counts("box_flat")) == {0, 2}
    assert set(counts("parallel")) <= {0, 1, 2, 3, 4} and counts("parallel").count(2) >= 16
    assert counts("box_through").count(0) == 0
    assert set(counts("near_miss")) == {0}
    for name in ref.FAMILIES[1:]:     # half the pair cases, give or take, have the capsule first
        f = ref.family(name)
        first = sum(int(f["shape"][i] == ref.CAPSULE) for i, _ in f["pairs"])
        assert first >= 20, (name, first)


@pytest.mark.parametrize("name", ["box_end", "box_flat", "box_edge", "box_corner", "box_narrow", "box_through"])
def test_reference_minimiser_against_a_ternary_search(name):
    """The reference finds the minimisers of dist from breakpoints and stationary points; here the same minimum by a
    method that knows neither: 300 steps of ternary search on the convex dist(t) over [-e, e] at 50 digits (the bracket
    shrinks to (2/3)^300 e).  The minimum values agree to 1e-30 and the point found lies in the reference's set of
    minimisers [t_lo, t_hi] to 1e-20: around a quadratic minimum two values 1e-50 apart are 1e-25 apart in t, which is
    as far as comparing values at 50 digits can place it.  Where the axis enters the box, dist is 0 at the reference's
    midpoint and at the point found.  Every fourth case of the family."""
    f = ref.family(name)
    for i, j in f["pairs"][::4]:
        c, b = (i, j) if f["shape"][i] == ref.CAPSULE else (j, i)
        with mp.workdps(ref.DPS):
            cc, d, e, u = ref._capsule(f["pos"][c], f["R"][c], f["side"][c])
            cB, R, h = ref._v(f["pos"][b]), ref._v(f["R"][b]), [x / 2 for x in ref._v(f["side"][b])]
            ax = [ref._col(R, k) for k in range(3)]
            rel = [cc[k] - cB[k] for k in range(3)]
            p0, ub = [ref._dot(ax[k], rel) for k in range(3)], [ref._dot(ax[k], u) for k in range(3)]
            dist = lambda t: ref.box_distance(p0, ub, h, t)
            lo, hi = -e, e
            for _ in range(300):
                a1, a2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
                if dist(a1) <= dist(a2):
                    hi = a2
                else:
                    lo = a1
            t = (lo + hi) / 2
            t_lo, t_hi, enters = ref.box_axis_minimisers(p0, ub, h, e)
            assert abs(dist(t) - dist(t_lo)) <= mp.mpf("1e-30"), (name, i, j)
            if enters:
                assert dist(t_lo) == 0
            else:
                assert t_lo - mp.mpf("1e-20") <= t <= t_hi + mp.mpf("1e-20"), (name, i, j)


def test_capsule_inertia_against_quadrature():
    """scenes.capsule_inertia (the adapter's Body::Capsule formula) against mpmath quadrature of the uniform solid:
    slices of radius rho(z), I_zz = int (pi / 2) rho^4 dz, I_xx = int (pi / 4) rho^4 + pi rho^2 z^2 dz, per unit density."""
    for m, r, length in ((1.0, 0.1, 0.6), (2.5, 0.15, 0.31), (0.7, 0.05, 1.3)):
        with mp.workdps(30):
            rr, H = mp.mpf(r), mp.mpf(length) - 2 * mp.mpf(r)
            rho2 = lambda z: rr * rr if abs(z) <= H / 2 else rr * rr - (abs(z) - H / 2) ** 2
            cuts = [-H / 2 - rr, -H / 2, H / 2, H / 2 + rr]
            vol = mp.quad(lambda z: mp.pi * rho2(z), cuts)
            izz = mp.quad(lambda z: mp.pi / 2 * rho2(z) ** 2, cuts) * m / vol
            ixx = mp.quad(lambda z: mp.pi / 4 * rho2(z) ** 2 + mp.pi * rho2(z) * z * z, cuts) * m / vol
        got = scenes.capsule_inertia(m, r, length)
        assert abs(got[0] - float(ixx)) <= 1e-14 * float(ixx) + 1e-18 and abs(got[1] - float(izz)) <= 1e-14 * float(izz) + 1e-18


def test_log_pile_scene():
    s = scenes.log_pile(2, 3, 2, radius=0.1, length=0.6)
    assert s["p"].shape == (12, 3) and (s["shape"] == 2).all() and (s["side"] == [0.2, 0.2, 0.6]).all()
    assert np.array_equal(s["R"][0].reshape(3, 3)[:, 2], [1, 0, 0]) and np.array_equal(s["R"][6].reshape(3, 3)[:, 2], [0, 1, 0])
    for R in (s["R"][0], s["R"][6]):
        assert np.linalg.det(R.reshape(3, 3)) == 1.0
