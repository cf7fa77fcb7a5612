"""GPU (-m gpu): a solve that starts from a given x0 (egs_problem_set_start) instead of rhs.  A start equal to rhs
must be the default solve bit for bit on every schedule; from any other start every schedule gives the same bits,
those bits are the projected sweeps from that start (numpy), and w = A x - rhs keeps the true rhs."""
import numpy as np
import pytest

import warm_start_reference as wsr
from eggshell_amd import capi, scenes
from helpers import dense_numpy, grouped_system, random_system
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
ENV = ("EGS_QUAD", "EGS_STEP", "EGS_PATCH", "EGS_QUAD_PATCH", "EGS_RUNS", "EGS_ISO", "EGS_STEP_GROUP")
# name -> (environment, method): every kernel a sweep can run on
SCHEDULES = {
    "tile": (dict(EGS_QUAD="0", EGS_STEP="0"), capi.GAUSS_SEIDEL),
    "timetable": (dict(EGS_QUAD="0", EGS_STEP="1"), capi.SOR),
    "quad_tickets": (dict(EGS_QUAD="1", EGS_STEP="0"), capi.SOR),
    "quad_timetable": (dict(EGS_QUAD="1", EGS_STEP="1", EGS_RUNS="1"), capi.GAUSS_SEIDEL),
    "quad_timetable_runs": (dict(EGS_QUAD="1", EGS_STEP="1", EGS_RUNS="2"), capi.SOR),
    "quad_patches": (dict(EGS_QUAD="0", EGS_PATCH="1", EGS_QUAD_PATCH="1"), capi.GAUSS_SEIDEL),
    "lane_patches": (dict(EGS_QUAD="0", EGS_PATCH="1", EGS_QUAD_PATCH="0"), capi.SOR),
    "all_global": (dict(EGS_QUAD="0", EGS_PATCH="0"), capi.SOR),
    "jacobi": (dict(EGS_QUAD="0"), capi.JACOBI),
}


def set_schedule(monkeypatch, name):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    env, method = SCHEDULES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return method


def isotropic(rng, s, antisymmetric):
    """The same system on bodies with M^-1 = diag(a, a, a, b, b, b) (the isotropic kernels), optionally with
    J1_lin = -J0_lin and one linear weight for all (the LINSYM form of the timetable kernel)."""
    w = np.zeros((s.n, 6, 6))
    for b in range(s.n):
        a_, b_ = (1.25, rng.uniform(0.2, 3.0)) if antisymmetric else rng.uniform(0.2, 3.0, 2)
        w[b] = np.diag([a_, a_, a_, b_, b_, b_])
    J0 = s.J0.copy().reshape(-1, 3, 6)
    if antisymmetric:
        both = (s.body0 >= 0) & (s.body1 >= 0)
        J0[both, :, :3] = -s.J1.reshape(-1, 3, 6)[both, :, :3]
    return orc.Sys(w.reshape(s.n, 36), s.body0, s.body1, J0.reshape(s.J0.shape), s.J1, s.is_eq, s.lo, s.hi)


def systems(rng, sizes=SIZES):
    """Small systems of every size at which a tile fills up, one with groups of four (the 4-lane plan's runs) and one
    oversize island of the size tests/test_gpu_patch.py uses."""
    out = [random_system(rng, max(2, m // 3 + 2), m) for m in sizes]
    base, _ = random_system(rng, 30, 40, world_frac=0.1)
    out.append(grouped_system(rng, base, None, 4))
    out.append(random_system(rng, 300, 2500, connected=True))
    return out


def solve(ctx, s, rhs, prm, precision=capi.F64, start=None, mode=capi.START_GIVEN):
    pr = capi.Problem(ctx, s.n, s.body0, s.body1, precision)
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, rhs)
    if start is not None:
        pr.set_start(mode, start)
    st = pr.solve(prm)
    out = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), it=st.iterations, res=st.residual, sched=st.schedule,
               status=st.status)
    pr.close()
    return out


def same_bits(p, q):
    return all(p[k].tobytes() == q[k].tobytes() for k in ("x", "a", "w")) and p["it"] == q["it"] and \
        np.float64(p["res"]).tobytes() == np.float64(q["res"]).tobytes()


@pytest.mark.parametrize("precision", [capi.F64, capi.F32])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_a_start_equal_to_rhs_is_the_default_solve(ctx, name, precision, monkeypatch):
    method = set_schedule(monkeypatch, name)
    rng = np.random.default_rng(300)
    cases = systems(rng)
    if name in ("tile", "timetable"):       # the isotropic kernels: plain, LINSYM (fp64), tile groups (fp32)
        monkeypatch.setenv("EGS_ISO", "2")
        base, rhs = random_system(rng, 40, 300, world_frac=0.15)
        cases += [(isotropic(rng, base, False), rhs), (isotropic(rng, base, True), rhs)]
    for s, rhs in cases:
        for prm in (capi.params(method=method, max_iters=4, tol=0.0, cfm=0.05),
                    capi.params(method=method, max_iters=40, tol=1e-4, cfm=0.5)):
            cold = solve(ctx, s, rhs, prm, precision)
            if precision == capi.F32:
                rhs = rhs.astype(np.float32).astype(np.float64)      # what the device holds
            warm = solve(ctx, s, rhs, prm, precision, start=rhs)
            assert cold["status"] == capi.OK and warm["status"] == capi.OK
            assert same_bits(cold, warm), (name, s.m, prm.tol)
            assert not cold["sched"] & capi.SCHED_START
            assert warm["sched"] == cold["sched"] | capi.SCHED_START, (name, s.m)


@pytest.mark.parametrize("precision", [capi.F64, capi.F32])
def test_every_schedule_gives_the_same_bits_from_a_random_start(ctx, precision, monkeypatch):
    rng = np.random.default_rng(301)
    cases = systems(rng, sizes=(65, 513))
    starts = [rng.uniform(-1, 1, 3 * s.m) for s, _ in cases]
    for method in (capi.GAUSS_SEIDEL, capi.SOR, capi.JACOBI):
        names = [n for n, (_, m) in SCHEDULES.items() if (m == capi.JACOBI) == (method == capi.JACOBI)]
        for (s, rhs), x0 in zip(cases, starts):
            for prm in (capi.params(method=method, max_iters=3, tol=0.0, cfm=0.05),
                        capi.params(method=method, max_iters=40, tol=1e-4, cfm=0.5)):
                first = None
                for name in names:
                    set_schedule(monkeypatch, name)
                    got = solve(ctx, s, rhs, prm, precision, start=x0)
                    assert got["status"] == capi.OK and got["sched"] & capi.SCHED_START
                    first = first or got
                    assert same_bits(first, got), (name, method, s.m, prm.tol)
                cold = solve(ctx, s, rhs, prm, precision)
                assert cold["x"].tobytes() != first["x"].tobytes() or s.m == 0


@pytest.mark.parametrize("method", [capi.JACOBI, capi.GAUSS_SEIDEL, capi.SOR])
def test_sweeps_from_a_random_start_are_the_numpy_sweeps(ctx, method, monkeypatch):
    """The bound of tests/test_oracle_sparse.py::test_fixed_sweeps_three_ways: 1e-9 x max(1, |x|inf)."""
    rng = np.random.default_rng(302)
    for n, m in ((5, 9), (12, 30)):
        s, rhs = random_system(rng, n, m)
        x0 = rng.uniform(-1, 1, 3 * m)
        A, J, W = dense_numpy(s, 0.05)
        for K in (1, 3, 10):
            xn, _ = wsr.pgs(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, K, x0)
            scale = max(1.0, np.abs(xn).max())
            for name in [n_ for n_, (_, me) in SCHEDULES.items() if (me == capi.JACOBI) == (method == capi.JACOBI)]:
                set_schedule(monkeypatch, name)
                got = solve(ctx, s, rhs, capi.params(method=method, max_iters=K, tol=0.0, cfm=0.05), start=x0)
                err = np.abs(got["x"] - xn).max()
                print(name, m, K, "x", err, "acc", np.abs(got["a"].reshape(-1) - W @ (J.T @ got["x"])).max())
                assert err < 1e-9 * scale, (name, K)
                assert np.abs(got["a"].reshape(-1) - W @ (J.T @ got["x"])).max() < 1e-9 * scale
                assert np.abs(got["w"] - (A @ got["x"] - rhs)).max() < 1e-9 * scale       # the true rhs
                assert abs(got["res"] - wsr.residual(A, rhs, got["x"], s.is_eq, s.lo, s.hi)) < 1e-9 * scale
        # no sweep at all: lambda is the start, the accumulators and w are the start's
        got = solve(ctx, s, rhs, capi.params(method=method, max_iters=0, tol=0.0, cfm=0.05), start=x0)
        assert np.array_equal(got["x"], x0)
        assert np.abs(got["w"] - (A @ x0 - rhs)).max() < 1e-9
        assert np.abs(got["a"].reshape(-1) - W @ (J.T @ x0)).max() < 1e-9


@pytest.mark.parametrize("precision", [capi.F64, capi.F32])
def test_previous_is_given_with_the_lambda_read_back(ctx, precision, monkeypatch):
    rng = np.random.default_rng(303)
    for name in ("timetable", "quad_tickets", "lane_patches", "jacobi"):
        method = set_schedule(monkeypatch, name)
        s, rhs = random_system(rng, 300, 2500, connected=True) if name == "lane_patches" else random_system(rng, 40, 257)
        rhs2 = rng.uniform(-1, 1, 3 * s.m)
        prm = capi.params(method=method, max_iters=5, tol=0.0, cfm=0.05)
        pr = capi.Problem(ctx, s.n, s.body0, s.body1, precision)
        pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, rhs)
        pr.set_start(capi.START_PREVIOUS)
        st = pr.solve(prm)                   # no lambda yet: the default start
        first = pr.lambda_()
        assert not st.schedule & capi.SCHED_START
        assert first.tobytes() == solve(ctx, s, rhs, prm, precision)["x"].tobytes()
        pr.set_blocks(rhs=rhs2)
        st = pr.solve(prm)                   # from the first solve's lambda
        assert st.schedule & capi.SCHED_START
        second = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), it=st.iterations, res=st.residual)
        st = pr.solve(prm)                   # and again: from the second's
        third = pr.lambda_()
        pr.set_start(capi.START_RHS)
        st = pr.solve(prm)
        assert not st.schedule & capi.SCHED_START
        assert pr.lambda_().tobytes() == solve(ctx, s, rhs2, prm, precision)["x"].tobytes()
        pr.close()
        assert same_bits(second, solve(ctx, s, rhs2, prm, precision, start=first)), name
        assert third.tobytes() == solve(ctx, s, rhs2, prm, precision, start=second["x"])["x"].tobytes(), name


@pytest.mark.parametrize("defer", ["1", "0"])
def test_a_start_that_passes_the_test_takes_no_sweep(ctx, defer, monkeypatch):
    monkeypatch.setenv("EGS_DEFER_RESIDUAL", defer)
    rng = np.random.default_rng(304)
    small, big = random_system(rng, 40, 257), random_system(rng, 300, 2500, connected=True)
    cfm = 0.5
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    # a start that passes by construction: 300 SOR sweeps' lambda, against twice the residual it reached.  The test it
    # has to pass does not depend on the method of the solve that takes it.
    x_small, x_big = (solve(ctx, s, rhs, capi.params(method=capi.SOR, max_iters=300, tol=0.0, cfm=cfm)) for s, rhs in (small, big))
    assert 0 < x_small["res"] < np.inf and 0 < x_big["res"] < np.inf
    # (Jacobi on an oversize island is the one solve without recorded chunks: the plain loop)
    for name, oversize in (("tile", 0), ("timetable", 0), ("quad_tickets", 0), ("quad_timetable", 0), ("quad_patches", 1),
                           ("all_global", 1), ("jacobi", 0), ("jacobi", 1)):
        method = set_schedule(monkeypatch, name)
        (s, rhs), x0, tol = (big, x_big["x"], 2 * x_big["res"]) if oversize else (small, x_small["x"], 2 * x_small["res"])
        got = solve(ctx, s, rhs, capi.params(method=method, max_iters=500, tol=tol, cfm=cfm), start=x0)
        huge = solve(ctx, s, rhs, capi.params(method=method, max_iters=500, tol=1e30, cfm=cfm), start=x0)
        assert got["it"] == 0 and huge["it"] == 0, (name, got["it"])
        assert got["x"].tobytes() == x0.tobytes()
        assert same_bits(got, huge), name
        assert got["res"] <= tol
        zero = solve(ctx, s, rhs, capi.params(method=method, max_iters=0, tol=0.0, cfm=cfm), start=x0)
        assert zero["a"].tobytes() == got["a"].tobytes() and zero["w"].tobytes() == got["w"].tobytes()
        if method != capi.JACOBI:     # one that does not pass goes on sweeping, from x0
            rough = solve(ctx, s, rhs, capi.params(method=method, max_iters=50, tol=tol, cfm=cfm), start=0.5 * x0)
            assert rough["it"] > 0 and rough["sched"] & capi.SCHED_START


def test_a_started_step_assembles_with_the_assembly_kernel(ctx, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EGS_QUAD", "0")
    monkeypatch.setenv("EGS_ISO", "2")
    sc = scenes.box_stack(3, 3, 3)
    Minv = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20, tol=0.0, cfm=0.01)

    def problem():
        pr = capi.Problem(ctx, sc["p"].shape[0], sc["body0"], sc["body1"])
        pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
        pr.set_constraints(sc["kind"], sc["data"])
        return pr

    pr = problem()
    cold = pr.step(5e-3, 0.2, prm, want_stats=True)
    assert cold.schedule & capi.SCHED_FUSED_ASSEMBLY        # what the start has to switch off
    x0 = 0.9 * pr.lambda_()
    pr.set_start(capi.START_GIVEN, x0)
    st = pr.step(5e-3, 0.2, prm, want_stats=True)
    assert st.schedule & capi.SCHED_START and not st.schedule & (capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_DEFERRED_SYSTEM)
    lam, v6 = pr.lambda_(), pr.velocity()
    pr.close()
    pr = problem()
    pr.set_start(capi.START_GIVEN, x0)
    pr.assemble(5e-3, 0.2)
    pr.solve(prm)
    assert pr.lambda_().tobytes() == lam.tobytes()
    pr.close()
    assert not np.array_equal(lam, x0 / 0.9)
    # ... and PREVIOUS: the second step starts from the first one's lambda
    pr = problem()
    pr.set_start(capi.START_PREVIOUS)
    st = pr.step(5e-3, 0.2, prm, want_stats=True)
    assert st.schedule & capi.SCHED_FUSED_ASSEMBLY and not st.schedule & capi.SCHED_START
    first = pr.lambda_()
    st = pr.step(5e-3, 0.2, prm, want_stats=True)
    assert st.schedule & capi.SCHED_START and not st.schedule & capi.SCHED_FUSED_ASSEMBLY
    second, v6b = pr.lambda_(), pr.velocity()
    pr.close()
    pr = problem()
    pr.set_start(capi.START_GIVEN, first)
    pr.step(5e-3, 0.2, prm)
    assert pr.lambda_().tobytes() == second.tobytes() and pr.velocity().tobytes() == v6b.tobytes()
    pr.close()
    assert v6.shape == v6b.shape


@pytest.mark.parametrize("precision", [capi.F64, capi.F32])
def test_every_ensemble_of_a_started_batch_is_its_own_problem(ctx, precision, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(305)
    parts = [random_system(rng, 6, 9), random_system(rng, 40, 257), random_system(rng, 20, 64)]
    starts = [rng.uniform(-1, 1, 3 * s.m) for s, _ in parts]
    for method, tol in ((capi.SOR, 0.0), (capi.GAUSS_SEIDEL, 0.0), (capi.JACOBI, 0.0)):
        prm = capi.params(method=method, max_iters=6, tol=tol, cfm=0.05)
        pr, boff, coff = capi.Problem.batch(ctx, [s.n for s, _ in parts], [s.m for s, _ in parts],
                                            np.concatenate([s.body0 for s, _ in parts]), np.concatenate([s.body1 for s, _ in parts]),
                                            precision)
        cat = lambda f: np.concatenate([f(s, r) for s, r in parts])
        pr.set_blocks(cat(lambda s, r: s.Minv.reshape(-1)), cat(lambda s, r: s.J0.reshape(-1)), cat(lambda s, r: s.J1.reshape(-1)),
                      cat(lambda s, r: s.is_eq), cat(lambda s, r: s.lo), cat(lambda s, r: s.hi), cat(lambda s, r: r))
        pr.set_start(capi.START_GIVEN, np.concatenate(starts))
        st = pr.solve(prm)
        assert st.schedule & capi.SCHED_START
        x, a = pr.lambda_(), pr.accumulators()
        pr.close()
        for e, ((s, rhs), x0) in enumerate(zip(parts, starts)):
            own = solve(ctx, s, rhs, prm, precision, start=x0)
            assert x[3 * coff[e]:3 * coff[e + 1]].tobytes() == own["x"].tobytes(), (method, e)
            assert a[boff[e]:boff[e + 1]].tobytes() == own["a"].tobytes(), (method, e)


def test_refusals(ctx):
    s, rhs = random_system(np.random.default_rng(306), 5, 9)
    pr = capi.Problem(ctx, s.n, s.body0, s.body1)
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, rhs)
    bad = rhs.copy(); bad[7] = np.nan
    for mode, x0 in ((3, None), (-1, rhs), (capi.START_GIVEN, None), (capi.START_GIVEN, bad)):
        with pytest.raises(capi.EgsError) as e:
            pr.set_start(mode, x0)
        assert e.value.status == capi.ERR_INVALID
    # a refused call changes nothing: still the default start
    prm = capi.params(method=capi.SOR, max_iters=3, tol=0.0, cfm=0.05)
    st = pr.solve(prm)
    assert not st.schedule & capi.SCHED_START
    assert pr.lambda_().tobytes() == solve(ctx, s, rhs, prm)["x"].tobytes()
    pr.set_start(capi.START_GIVEN, np.full(3 * s.m, np.inf))       # not a NaN: the caller's business
    pr.close()
