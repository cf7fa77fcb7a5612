"""CPU: the 50-digit sweep reference (tests/sweep_reference.py) checked against the mathematics, and the oracle's three
restatements of the sweeps -- orc.lit_iterate(quirks=0), orc.fast_iterate, orc.fast_iterate_f32 -- checked against it:
lambda, the accumulators, fast_wres, the reported residual against residual() at the oracle's own x, and the sweep count
of a tolerance-terminated run.  Bounds: sweep_reference.BOUNDS.  Every test prints its measured
error / u per quantity (pytest -s); tests/test_gpu_sweep_reference.py holds the device to the same cases and bounds."""
import mpmath as mp
import numpy as np
import pytest

import sweep_reference as ref
import warm_start_reference as wsr
from helpers import check_mixed_solution, dense_numpy, numpy_pgs, random_system
from oracle import oracle as orc


# ---- (a) the reference against the mathematics ------------------------------------------------------------------------
def small_spd(cfm=0.3, seed=720, n=6, m=7):
    """7 constraints on 6 bodies: with cfm 0.3 A is positive definite and GS / SOR converge linearly; with cfm 50 it is
    diagonally dominant as well and so does Jacobi."""
    s, rhs = random_system(np.random.default_rng(seed), n, m)
    return s, rhs, ref.system(s, cfm)


def test_fixed_point_satisfies_the_mixed_lcp():
    s, rhs, A = small_spd()
    x = ref.sweeps(A, rhs, s.is_eq, s.lo, s.hi, ref.GAUSS_SEIDEL, 1.0, 800)
    with mp.workdps(ref.DPS):
        worst = ref.mixed_lcp_violation(A, rhs, x, s.is_eq, s.lo, s.hi)
        res, _ = ref.residual(A, rhs, x, s.is_eq, s.lo, s.hi)
        print("fixed point: worst violation %s, residual %s" % (mp.nstr(worst, 3), mp.nstr(res, 3)))
        assert worst < mp.mpf("1e-30") and res < mp.mpf("1e-30")
        on_bound = sum(1 for r in range(3 * s.m) if not s.is_eq[r] and (x[r] == s.lo[r] or x[r] == s.hi[r]))
    assert on_bound > 0          # a fixed point of the projected problem, not of the linear one
    # ... and the fp64 rule agrees on the rounded result
    Ad, _, _ = dense_numpy(s, 0.3)
    assert check_mixed_solution(Ad, rhs, np.array([float(t) for t in x]), s.is_eq, s.lo, s.hi)


@pytest.mark.parametrize("method", ref.ALL)
def test_all_equality_rows_converge_to_lu_solve(method):
    s, rhs, A = small_spd(50.0 if method == ref.JACOBI else 0.3)
    eq = np.ones(3 * s.m, np.uint8)
    x = ref.sweeps(A, rhs, eq, s.lo, s.hi, method, 1.2, 800)
    with mp.workdps(ref.DPS):
        want = mp.lu_solve(A.dense(), mp.matrix([mp.mpf(float(t)) for t in rhs]))
        d = max(abs(x[r] - want[r]) for r in range(3 * s.m))
        print("method %d: |x - lu_solve| = %s" % (method, mp.nstr(d, 3)))
        assert d < mp.mpf("1e-30")


def test_backward_sor_at_omega_one_is_gs_on_the_reversed_list():
    rng = np.random.default_rng(721)
    s, rhs = random_system(rng, 6, 11)
    rev = np.arange(s.m)[::-1]
    rows = (3 * rev[:, None] + np.arange(3)[::-1][None, :]).reshape(-1)        # row r of the reversed list
    sr = orc.Sys(s.Minv, s.body0[rev], s.body1[rev], s.J0.reshape(-1, 3, 6)[rev][:, ::-1].reshape(-1, 18),
                 s.J1.reshape(-1, 3, 6)[rev][:, ::-1].reshape(-1, 18), s.is_eq[rows], s.lo[rows], s.hi[rows])
    x = ref.sweeps(ref.system(s, 0.05), rhs, s.is_eq, s.lo, s.hi, ref.SOR, 1.0, 5)
    y = ref.sweeps(ref.system(sr, 0.05), rhs[rows], sr.is_eq, sr.lo, sr.hi, ref.GAUSS_SEIDEL, 1.0, 5)
    with mp.workdps(ref.DPS):
        assert max(abs(x[rows[r]] - y[r]) for r in range(3 * s.m)) < mp.mpf("1e-40")


def test_jacobi_is_gs_on_a_diagonal_matrix():
    """Every constraint on bodies of its own, one row direction per linear axis: A is diagonal."""
    rng = np.random.default_rng(722)
    m = 5
    J0 = np.zeros((m, 3, 6)); J0[:, [0, 1, 2], [0, 1, 2]] = rng.uniform(0.5, 2.0, (m, 3))
    Minv = np.tile(np.diag(rng.uniform(0.5, 2.0, 6)).reshape(36), (m, 1))
    is_eq = (rng.uniform(size=3 * m) < 0.4).astype(np.uint8)
    lo, hi = -rng.uniform(0.1, 1.0, 3 * m), rng.uniform(0.1, 1.0, 3 * m)
    s = orc.Sys(Minv, np.arange(m), np.full(m, -1), J0.reshape(m, 18), np.zeros((m, 18)), is_eq, lo, hi)
    rhs = rng.uniform(-1, 1, 3 * m)
    A = ref.system(s, 0.1)
    assert all(len(c) == 1 for c in A.cols)
    x = ref.sweeps(A, rhs, is_eq, lo, hi, ref.JACOBI, 1.5, 3)
    y = ref.sweeps(A, rhs, is_eq, lo, hi, ref.GAUSS_SEIDEL, 1.5, 3)
    assert x == y


@pytest.mark.parametrize("method", ref.ALL)
def test_equals_numpy_pgs_on_its_own_shapes(method):
    """tests/test_oracle_sparse.py::test_fixed_sweeps_three_ways' two shapes, seed and sweep counts, to 1e-12; and from a
    start other than rhs, which the oracle does not take, against warm_start_reference.pgs."""
    rng = np.random.default_rng(5)
    for n, m in ((5, 9), (12, 30)):
        s, rhs = random_system(rng, n, m)
        Ad, J, W = dense_numpy(s, 0.05)
        A = ref.system(s, 0.05)
        hist = ref.sweeps(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 10, history=True)
        for K in (1, 3, 10):
            xn = numpy_pgs(Ad, rhs, s.is_eq, s.lo, s.hi, method, 1.5, K)
            scale = max(1.0, np.abs(xn).max())
            assert np.abs(np.array([float(t) for t in hist[K]]) - xn).max() < 1e-12 * scale
        x0 = np.random.default_rng(m).uniform(-1, 1, 3 * m)
        xs = ref.sweeps(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 3, x0=x0)
        xn, _ = wsr.pgs(Ad, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 3, x0)
        assert np.abs(np.array([float(t) for t in xs]) - xn).max() < 1e-12 * max(1.0, np.abs(xn).max())
        assert ref.sweeps(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 0, x0=x0) == [mp.mpf(float(t)) for t in x0]
        # the other statements: accumulators, w and the residual at a given x against plain numpy
        a, _ = ref.accumulators(A, xn)
        assert np.abs(np.array([float(t) for t in a]) - W @ (J.T @ xn)).max() < 1e-12 * max(1.0, np.abs(xn).max())
        w, _ = ref.wres(A, rhs, xn)
        assert np.abs(np.array([float(t) for t in w]) - (Ad @ xn - rhs)).max() < 1e-12 * max(1.0, np.abs(xn).max())
        res, _ = ref.residual(A, rhs, xn, s.is_eq, s.lo, s.hi)
        assert abs(float(res) - wsr.residual(Ad, rhs, xn, s.is_eq, s.lo, s.hi)) < 1e-12 * max(1.0, float(res))


# ---- (b) the oracle against the reference -------------------------------------------------------------------------------
def oracle_ratios(cid, method, K, f32):
    """Error ratios (units of u) of orc.fast_iterate / fast_iterate_f32 and, in fp64, orc.lit_iterate(quirks=0) on one
    run of a case: {"fast": {x, a, w, r}, "lit": {x, r}}."""
    c = ref.case(cid)
    A = ref.case_system(cid, f32)
    x_ref = ref.case_iterates(cid, method, f32)[K]
    s = c.s
    if f32:
        x, a, it, res = orc.fast_iterate_f32(s, c.rhs, c.cfm, method, c.omega, max_iters=K, tol=0.0)
        w = orc.fast_wres_f32(s, c.rhs, c.cfm, x, a)
        out = {"fast": ref.measure(A, c.rhs, s.is_eq, s.lo, s.hi, x_ref, x, a, w, float(res))}
    else:
        x, a, it, res = orc.fast_iterate(s, c.rhs, c.cfm, method, c.omega, max_iters=K, tol=0.0)
        w = orc.fast_wres(s, c.rhs, c.cfm, x, a)
        out = {"fast": ref.measure(A, c.rhs, s.is_eq, s.lo, s.hi, x_ref, x, a, w, res)}
        xl, itl, rl = orc.lit_iterate(s, c.rhs, c.cfm, method, c.omega, max_iters=K, tol=0.0, quirks=0)
        assert itl == K
        out["lit"] = ref.measure(A, c.rhs, s.is_eq, s.lo, s.hi, x_ref, xl, None, None, rl)
    assert it == K
    return out


ORACLE_CASES = [cid for cid in ref.CASE_IDS if cid != "start"]      # the oracle starts from rhs only: that case is the device's


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", ORACLE_CASES)
def test_oracle_against_the_reference(cid, f32):
    c = ref.case(cid)
    bound = ref.BOUNDS[(c.cls, f32)]
    bad = []
    for method, ks in c.runs.items():
        for K in ks:
            got = oracle_ratios(cid, method, K, f32)
            for who, r in got.items():
                print("%s %s method %d K %d %s: " % (cid, "f32" if f32 else "f64", method, K, who) +
                      " ".join("%s=%.3g/%g" % (q, v, bound[q]) for q, v in sorted(r.items())))
                bad += [(who, method, K, q, v) for q, v in r.items() if not v <= bound[q]]
    assert not bad, bad


def test_rows_on_a_bound_in_the_large_pile():
    """The 4 x 4 x 4 pile after 8 sweeps is a projected problem in earnest: more than 100 rows sit on a bound."""
    c = ref.case("pile444")
    x = ref.case_iterates("pile444", ref.GAUSS_SEIDEL)[8]
    on = sum(1 for r in range(3 * c.s.m) if not c.s.is_eq[r] and (x[r] == c.s.lo[r] or x[r] == c.s.hi[r]))
    print("pile444: %d of %d rows on a bound" % (on, 3 * c.s.m))
    assert on > 100


# ---- (c) the sweep count of a tolerance-terminated run ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(ref.STOP_RUNS))
def test_a_tolerance_terminated_run_stops_where_the_reference_stops(cid):
    method, tol, limit = ref.STOP_RUNS[cid]
    K, clear, res = ref.stop_reference(cid)
    with mp.workdps(ref.DPS):
        print("%s: reference stops after %s sweeps; residuals around the crossing %s" % (cid, K, [mp.nstr(r, 4) for r in res[-3:]]))
    assert K is not None and 0 < K < limit
    assert clear, "the reference's residual comes within 1 % of tol: choose another tol for this case"
    c = ref.case(cid)
    x, a, it, r = orc.fast_iterate(c.s, c.rhs, c.cfm, method, c.omega, max_iters=limit, tol=tol)
    assert it == K and r <= tol


def test_singular_pile_reported_and_true_residual():
    """The finding of DESIGN.md section 6c: on the 2 x 2 x 2 pile with cfm = 0 (redundant contacts, A singular) the
    residual reduced from the carried accumulators after 500 sweeps understates A x - rhs of the oracle's own x by
    orders of magnitude.  Both are far below any tol in use; the gap is what the singular class's constants admit."""
    c = ref.case("singular222")
    x, a, it, res = orc.fast_iterate(c.s, c.rhs, c.cfm, ref.GAUSS_SEIDEL, c.omega, max_iters=500, tol=0.0)
    A = ref.case_system("singular222")
    true, scale = ref.residual(A, c.rhs, x, c.s.is_eq, c.s.lo, c.s.hi)
    with mp.workdps(ref.DPS):
        print("singular pile, 500 GS sweeps: reported residual %.3g, true %s, |mag|_2 %s" % (res, mp.nstr(true, 3), mp.nstr(scale, 3)))
        assert true < 1e-9 and res < 1e-9
    assert ref.err_scalar(res, true, scale) <= ref.BOUNDS[("singular", False)]["r"]
