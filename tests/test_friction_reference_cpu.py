"""CPU: the friction pyramid's 50-digit reference (tests/friction_reference.py) checked against the mathematics -- its
degenerate coefficients are sweep_reference's sweeps exactly, a converged run satisfies the pyramid's KKT conditions,
the tilted-gravity cube slides and sticks as Coulomb says -- and the plain numpy port (tests/friction_port.py) checked
against it within friction_reference.BOUNDS on every case and both precisions.  The two tolerance-terminated runs of
the device tests keep clear of tol.  Every test prints its figures (pytest -s); DESIGN.md section 6d records them."""
import mpmath as mp
import numpy as np
import pytest

import friction_port as port
import friction_reference as fr
import sweep_reference as ref
from helpers import random_system
from oracle import oracle as orc


@pytest.mark.parametrize("method", ref.ALL)
def test_degenerate_coefficients_are_the_plain_sweeps(method):
    """mu = -1 everywhere is sweep_reference.sweeps; mu = 0 on every contact is sweep_reference.sweeps with
    lo = hi = 0 on the contacts' tangential rows.  Exactly, in mpmath."""
    s, rhs = random_system(np.random.default_rng(730), 8, 14)
    A = ref.system(s, 0.05)
    plain = ref.sweeps(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 6)
    assert fr.sweeps_pyramid(A, rhs, s.is_eq, s.lo, s.hi, np.full(s.m, -1.0), method, 1.5, 6) == plain
    c = ref.case("joint-contact")
    A = ref.case_system("joint-contact")
    mu = np.where(fr.case_mu("joint-contact") >= 0, 0.0, -1.0)
    assert (mu == 0).any() and (mu < 0).any()
    lo, hi, eq = c.s.lo.copy(), c.s.hi.copy(), c.s.is_eq.copy()
    for i in np.nonzero(mu == 0)[0]:
        lo[3 * i:3 * i + 2] = 0.0; hi[3 * i:3 * i + 2] = 0.0; eq[3 * i:3 * i + 2] = 0
    pinned = ref.sweeps(A, c.rhs, eq, lo, hi, method, 1.5, 6)
    assert fr.sweeps_pyramid(A, c.rhs, c.s.is_eq, c.s.lo, c.s.hi, mu, method, 1.5, 6) == pinned
    assert pinned != ref.sweeps(A, c.rhs, c.s.is_eq, c.s.lo, c.s.hi, method, 1.5, 6)


def test_a_converged_run_satisfies_the_pyramid_kkt():
    """Backward SOR to a fixed point on a random system of mixed row types, mu from {-1, 0, 0.3, 0.5}: every condition
    holds to 1e-30 and some row sits on a face of its pyramid.  (The backward sweep clamps against the x_n it has just
    made, so its iterate is inside its own cone at every sweep.  The forward sweep clamps against the previous x_n: a
    row on a face with w != 0 reads as strictly inside, or outside, the new cone for as long as x_n still moves in the
    last digit, so its residual reaches zero only once x_n has stopped exactly -- DESIGN.md section 6d.)"""
    s, rhs = random_system(np.random.default_rng(731), 6, 9)
    A = ref.system(s, 0.3)
    mu = np.random.default_rng(732).choice((-1.0, 0.0, 0.3, 0.5), size=s.m)
    assert (mu > 0).any()
    x = fr.sweeps_pyramid(A, rhs, s.is_eq, s.lo, s.hi, mu, ref.SOR, 1.2, 600)
    with mp.workdps(ref.DPS):
        worst = fr.pyramid_violation(A, rhs, x, s.is_eq, s.lo, s.hi, mu)
        res, _ = fr.residual_pyramid(A, rhs, x, s.is_eq, s.lo, s.hi, mu)
        print("worst KKT violation %s, residual %s" % (mp.nstr(worst, 3), mp.nstr(res, 3)))
        assert worst < mp.mpf("1e-30") and res < mp.mpf("1e-30")
        on_face = sum(1 for i in range(s.m) if mu[i] > 0 and x[3 * i + 2] > 0
                      for r in (0, 1) if abs(x[3 * i + r]) == mp.mpf(float(mu[i])) * x[3 * i + 2])
    assert on_face > 0      # a point on the pyramid's faces, not inside it


@pytest.mark.parametrize("method", [ref.GAUSS_SEIDEL, ref.SOR], ids=["gs", "sor"])
def test_the_sticking_cube_satisfies_the_pyramid_kkt(method):
    """mu = 0.8 > tan theta: no tangential row ends on a face with w != 0, and both sweeps converge."""
    case, s, rhs = cube_system()
    A = ref.system(s, 0.0)
    mus = np.full(4, 0.8)
    x = fr.sweeps_pyramid(A, rhs, s.is_eq, s.lo, s.hi, mus, method, 1.5, fr.CUBE_SWEEPS)
    with mp.workdps(ref.DPS):
        worst = fr.pyramid_violation(A, rhs, x, s.is_eq, s.lo, s.hi, mus)
        print("method %d: worst KKT violation %s" % (method, mp.nstr(worst, 3)))
        assert worst < mp.mpf("1e-30")


def port_ratios(cid, method, K, f32):
    c = ref.case(cid)
    mu = fr.case_mu(cid)
    x, a, w, res = port.sweeps(c.s, c.rhs, c.cfm, mu, method, c.omega, K, f32, c.x0)
    return fr.measure(ref.case_system(cid, f32), c.rhs, c.s.is_eq, c.s.lo, c.s.hi, mu, fr.case_iterates(cid, method, f32)[K],
                      x, a, w, res)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", fr.CASES)
def test_port_against_the_reference(cid, f32):
    c = ref.case(cid)
    bound = fr.BOUNDS[(c.cls, f32)]
    bad = []
    for method, ks in c.runs.items():
        for K in ks:
            r = port_ratios(cid, method, K, f32)
            print("%s %s method %d K %d: " % (cid, "f32" if f32 else "f64", method, K) +
                  " ".join("%s=%.3g/%g" % (q, v, bound[q]) for q, v in sorted(r.items())))
            bad += [(method, K, q, v) for q, v in r.items() if not v <= bound[q]]
    assert not bad, bad


def cube_system(cfm=0.0):
    """The cube's assembled system (the oracle's assembly makes INPUTS only) and its rhs."""
    case = fr.cube_case()
    J0, J1, is_eq, lo, hi, err = orc.assemble(case["p"], case["R"], case["kind"], case["body0"], case["body1"], case["data"])
    s = orc.Sys(case["Minv"], case["body0"], case["body1"], J0, J1, is_eq, lo, hi)
    rhs = orc.ode_rhs(case["v"], case["w"], s.Minv, case["f_ext"], s.body0, s.body1, J0, J1, err, case["dt"], case["erp"])
    return case, s, rhs


@pytest.mark.parametrize("method", [ref.GAUSS_SEIDEL, ref.SOR], ids=["gs", "sor"])
@pytest.mark.parametrize("mu", [0.2, 0.8])
def test_tilted_gravity_cube(mu, method):
    """v_x = dt g (sin theta - mu cos theta) at mu = 0.2 (2.632299e-3), 0 at mu = 0.8, every other component 0: the
    reference after 500 sweeps within CUBE_REF_DISTANCE (8 x its measured distance from the analytic value), the fp64
    port likewise; the reference's friction box gives neither value."""
    case, s, rhs = cube_system()
    A = ref.system(s, 0.0)
    mus = np.full(4, mu)
    want = fr.cube_velocity(mu)
    if mu == 0.2:
        assert "%.6e" % want[0] == "2.632299e-03"
    x = fr.sweeps_pyramid(A, rhs, s.is_eq, s.lo, s.hi, mus, method, 1.5, fr.CUBE_SWEEPS)
    v = ref.velocity_after(case, s.J0, s.J1, np.array([float(t) for t in x])).array()
    dist = np.abs(v - want).max()
    xp, ap, _, _ = port.sweeps(s, rhs, 0.0, mus, method, 1.5, fr.CUBE_SWEEPS)
    vp = case["dt"] * ((case["Minv"].reshape(6, 6) @ case["f_ext"].reshape(6)) + ap)
    print("cube mu %.1f method %d: reference v = %s, distance %.3g; port distance %.3g" % (mu, method, v, dist, np.abs(vp - want).max()))
    assert dist <= fr.CUBE_REF_DISTANCE
    assert np.abs(vp - want).max() <= fr.CUBE_REF_DISTANCE
    box = ref.sweeps(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, fr.CUBE_SWEEPS)
    vb = ref.velocity_after(case, s.J0, s.J1, np.array([float(t) for t in box])).array()
    assert np.abs(vb - want).max() > 1e-4      # the box saturates at 1 per contact: 4 < m g sin(theta) = 4.387


@pytest.mark.parametrize("method", fr.STOP_METHODS, ids=["gs", "sor"])
def test_the_tolerance_terminated_runs_keep_clear_of_tol(method):
    """singular222 with mu = 0.5, tol 1e-9: the reference stops after 134 (GS) / 110 (SOR 1.5) sweeps and its residuals
    keep clear of tol by gap_condition's 1.01 on both sides of the crossing."""
    K, clear, res = fr.stop_reference(method)
    with mp.workdps(ref.DPS):
        tol = mp.mpf(fr.STOP_TOL)
        print("method %d: reference stops after %s sweeps; last above %s x tol, first below %s x tol" %
              (method, K, mp.nstr(res[-2] / tol, 4), mp.nstr(res[-1] / tol, 4)))
    assert K == {ref.GAUSS_SEIDEL: 134, ref.SOR: 110}[method]
    assert clear
