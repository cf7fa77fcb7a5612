"""GPU (-m gpu): hinge angle limits on a problem (egs_problem_set_hinge_limits).  The assembly against the fp64 twin of
tests/limit_reference.py bit for bit; the table off is the run without the call; the refusals; lambda of a step against
a 50-digit direct solve of the same bounded system; the dense step's refusal."""
import math

import mpmath as mp
import numpy as np
import pytest

import joint_cases as jc
import joint_reference as jr
import limit_reference as lr
import model_reference as mr
from eggshell_amd import capi
from oracle import oracle as orc
from test_gpu_joints import _dv_bound, assert_twin, make_problem

pytestmark = pytest.mark.gpu

GS3 = dict(method=capi.GAUSS_SEIDEL, max_iters=3, tol=0.0, cfm=0.01)


# ---- 1. the assembly is the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("fam", list(lr.FAMILIES))
def test_limit_rows_are_the_twin(ctx, fam, precision):
    """The m = 8 list (a two-body hinge and a world-side one among the other kinds) under every family of tables, with
    and without the motor table beside it (tau = 0 and +inf on its hinges): egs_problem_assemble, then egs_problem_step."""
    case, motor, _, _, _ = jr.generated("n4m8-a")
    lim = lr.make_limits(case, lr.FAMILIES[fam])
    pr = make_problem(ctx, case, precision)
    for mt in (None, motor):
        tw = lr.twin_assemble(case, mt, lim)
        pr.set_motors(mt)
        pr.set_hinge_limits(lim)
        pr.assemble(case["dt"], case["erp"])
        assert_twin(pr.blocks(), tw, precision, what=fam + " assemble")
        st = pr.step(case["dt"], case["erp"], capi.params(**GS3), want_stats=True)
        assert st.status == capi.OK
        assert_twin(pr.blocks(), tw, precision, what=fam + " step")
    pr.close()


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_long_list_and_the_other_tables(ctx, precision):
    """259 constraints (two 256-thread blocks), the hinges cycling through every spec and every motor; then restitution
    and friction tables on the contacts: the joints' rows keep the twin's bits."""
    case, motor, _, _, _ = jr.generated("m259")
    lim = lr.make_limits(case, 0)
    tw = lr.twin_assemble(case, motor, lim)
    hinges = case["kind"] == jr.HINGE
    assert {-1, 0, 1} <= set(tw["active"][hinges]) and (tw["active"][hinges & (motor[:, 1] >= 0)] != 0).any()
    pr = make_problem(ctx, case, precision)
    pr.set_motors(motor)
    pr.set_hinge_limits(lim)
    pr.assemble(case["dt"], case["erp"])
    assert_twin(pr.blocks(), tw, precision, what="assemble")
    pr.step(case["dt"], case["erp"], capi.params(**GS3))
    assert_twin(pr.blocks(), tw, precision, what="step")
    pr.set_restitution(np.where(case["kind"] == jr.CONTACT, 0.5, -1.0), 0.0)
    pr.set_friction(np.where(case["kind"] == jr.CONTACT, 0.4, -1.0))
    pr.step(case["dt"], case["erp"], capi.params(**GS3))
    assert_twin(pr.blocks(), tw, precision, rows=np.nonzero(case["kind"] != jr.CONTACT)[0], what="tables")
    pr.close()


def _run(pr, case):
    st = pr.step(case["dt"], case["erp"], capi.params(**GS3), want_stats=True)
    return [np.asarray(x).tobytes() for x in pr.blocks()] + [pr.lambda_().tobytes(), pr.velocity().tobytes()], (st.schedule, pr.schedule())


def test_table_off_is_the_run_without_the_call(ctx):
    """No call; lim = None; rows that are all (0, 0) on the hinges (stops on the other kinds' rows, which are ignored); a
    table set and taken away: the same bits and the same schedule flags."""
    case, motor, _, _, driven = jr.generated("n4m8-a")
    runs = []
    for mode in ("none", "null", "zeros", "taken-away", "constraints-again"):
        pr = make_problem(ctx, case)
        pr.set_motors(motor)
        lim = lr.make_limits(case, 0)
        if mode == "null":
            pr.set_hinge_limits(None)
        elif mode == "zeros":
            z = lim.copy(); z[case["kind"] == jr.HINGE, 4:8] = 0.0
            pr.set_hinge_limits(z)
        elif mode == "taken-away":
            pr.set_hinge_limits(lim)
            pr.step(case["dt"], case["erp"], capi.params(**GS3))
            pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
            pr.set_hinge_limits(None)
        elif mode == "constraints-again":      # a new egs_problem_set_constraints turns the limits (and the motors) off
            pr.set_hinge_limits(lim)
            pr.set_constraints(case["kind"], case["data"])
            pr.set_motors(motor)
        runs.append(_run(pr, case))
        if mode == "none":
            assert_twin(pr.blocks(), driven, capi.F64, what="no table")
        pr.close()
    for r in runs[1:]:
        assert r[1] == runs[0][1]
        for a, b in zip(runs[0][0], r[0]):
            assert a == b


def test_refusals(ctx):
    """EGS_ERR_INVALID for every fault of the header's list, on a problem whose table is set: the blocks afterwards are
    those of the table in force."""
    case, motor, _, _, _ = jr.generated("n4m8-a")
    lim = lr.make_limits(case, 0)
    hinge = int(np.nonzero(case["kind"] == jr.HINGE)[0][0])
    ball = int(np.nonzero(case["kind"] == jr.BALL)[0][0])
    pr = make_problem(ctx, case)
    pr.set_hinge_limits(lim)
    pr.assemble(case["dt"], case["erp"])
    before = pr.blocks()
    bad = []
    for col, val in ((0, np.nan), (5, np.inf), (0, lim[hinge, 0] + 1e-9), (6, lim[hinge, 6] + 1e-9)):
        b = lim.copy(); b[hinge, col] = val; bad.append(b)
    b = lim.copy(); b[ball, 2] = np.nan; bad.append(b)                                   # non-finite on an ignored row
    b = lim.copy(); b[hinge, 6:8] = (math.sin(math.pi), -1.0); bad.append(b)             # a stop at pi
    b = lim.copy(); b[hinge, 4:8] = lr.pair(0.3) + lr.pair(0.2); bad.append(b)           # lo above hi
    b = lim.copy(); b[hinge, 4:8] = lr.pair(-3.0) + lr.pair(-3.1); bad.append(b)         # ... near -pi
    for b in bad:
        with pytest.raises(capi.EgsError) as ei:
            pr.set_hinge_limits(b)
        assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(ValueError):
        pr.set_hinge_limits(lim[:-1])
    ok = lim.copy(); ok[hinge, 4:8] = lr.pair(0.2) + lr.pair(0.2)      # lo = hi is a range
    pr.set_hinge_limits(ok)
    pr.set_hinge_limits(lim)
    pr.assemble(case["dt"], case["erp"])
    for a, c in zip(before, pr.blocks()):
        assert a.tobytes() == c.tobytes()
    assert_twin(before, lr.twin_assemble(case, None, lim), capi.F64, what="after the refusals")
    pr.close()


def test_dense_step_refuses_a_limited_hinge(ctx):
    """Whether the row is pinned is decided on the device: EGS_ERR_UNSUPPORTED naming the hinge, before anything is
    launched, even with a motor that would make the row a box row; the problem steps on, and without the table the
    dense step runs."""
    sc = jc.pendulum((1.0, 3.0))
    lim = np.zeros((2, 8)); lim[1] = lr.limit_row(jc.EYE, [0.0, 1.0, 0.0], None, 0.1, -0.3, 0.5)
    pr = jc.make_problem(ctx, sc)
    pr.set_hinge_limits(lim)
    with pytest.raises(capi.EgsError) as ei:
        pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=1)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "hinge constraint 1" in str(ei.value)
    st = pr.step(sc["dt"], sc["erp"], capi.params(method=capi.SOR, max_iters=50, tol=0.0, cfm=0.0), want_stats=True)
    assert st.status == capi.OK and np.isfinite(pr.lambda_()).all()
    pr.set_hinge_limits(None)
    ok, _ = pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=1)
    assert ok
    pr.close()


# ---- 2. the solve against the reference --------------------------------------------------------------------------------------
DELTA, HI = 0.02, 0.3
# (motor, theta now, lo, hi): the pendulum of joint_cases (gravity turns it about +y, towards the upper stop)
SCENES = {"door-past-stop": (None, HI + DELTA, -0.5, HI), "motor-into-stop": ((1.0, 5.0), HI + DELTA, None, HI),
          "door-inside": (None, 0.1, -0.5, HI)}
_solved = {}


def solved(ctx, name):
    """One egs_problem_step (SOR, tol 1e-12, cfm 0) per scene, with the reference's lambda and test_gpu_joints' bound
    |lambda - lambda_ref|_inf <= |A_ff^-1|_1 (residual + 32u max_r mag_r): the device's system is the twin's bit for bit
    (asserted), the reference solves that system exactly with the active set decided in mpmath."""
    if name not in _solved:
        motor, theta, lo, hi = SCENES[name]
        sc = jc.pendulum(motor)
        lim = np.zeros((2, 8)); lim[1] = lr.limit_row(jc.EYE, [0.0, 1.0, 0.0], None, theta, lo, hi)
        pr = jc.make_problem(ctx, sc)
        pr.set_hinge_limits(lim)
        st = pr.step(sc["dt"], sc["erp"], capi.params(method=capi.SOR, max_iters=20000, tol=1e-12, cfm=0.0, omega=1.2), want_stats=True)
        lam, v6, blocks = pr.lambda_(), pr.velocity(), pr.blocks()
        pr.close()
        tw = lr.twin_assemble(sc, sc["motor"], lim)
        assert_twin(blocks, tw, capi.F64, what=name)
        x, norm1, margin = jr.solve_reference(sc, tw, 0.0)
        assert margin > 1e-9, "the scene sits on a tie of its active set: choose another"
        with mp.workdps(mr.DPS):
            from sweep_reference import system as sweep_system
            s = orc.Sys(sc["Minv"].reshape(-1, 6, 6), sc["body0"], sc["body1"], tw["J0"].reshape(-1, 3, 6), tw["J1"].reshape(-1, 3, 6),
                        tw["is_eq"], tw["lo"], tw["hi"])
            mag = sweep_system(s, 0.0).mag(x, tw["rhs"])
            bound = norm1 * (mp.mpf(st.residual) + 32 * mr.U * max(mag))
        _solved[name] = dict(sc=sc, st=st, lam=lam, v6=v6, x=x, bound=float(bound), tw=tw)
        print("%s: %d sweeps, residual %.3g, |A_ff^-1|_1 %.3g, bound %.3g, lambda2 %.6g" %
              (name, st.iterations, st.residual, float(norm1), float(bound), lam[5]))
    return _solved[name]


@pytest.mark.parametrize("name", list(SCENES))
def test_lambda_against_the_direct_solve(ctx, name):
    r = solved(ctx, name)
    assert r["st"].status == capi.OK and r["st"].iterations < 20000 and r["st"].residual <= 1e-12
    with mp.workdps(mr.DPS):
        worst = max(abs(mp.mpf(float(a)) - b) for a, b in zip(r["lam"], r["x"]))
    print("%s: |lambda - reference|_inf %.3g, bound %.3g" % (name, float(worst), r["bound"]))
    assert worst <= r["bound"]


@pytest.mark.parametrize("name", ["door-past-stop", "motor-into-stop"])
def test_a_door_past_its_stop_is_pushed_back(ctx, name):
    """Past the stop by delta the row is active (also under a motor that drives into the stop, whose row it replaces for
    the step): the door leaves with s^ . w' = -erp sin(delta) / dt and lambda2 < 0."""
    r = solved(ctx, name)
    sc, tw = r["sc"], r["tw"]
    assert tw["active"][1] == 1 and (tw["lo"][5], tw["hi"][5]) == (-math.inf, 0.0)
    assert abs(tw["err"][5] - math.sin(DELTA)) < 1e-15
    want = -sc["erp"] * tw["err"][5] / sc["dt"]
    b = _dv_bound(r) + 4 * 2.0 ** -53 * abs(want)
    print("%s: s^ . w' %.17g, want %.17g, bound %.3g" % (name, r["v6"][0, 4], want, b))
    assert abs(r["v6"][0, 4] - want) <= b
    assert r["lam"][5] < 0.0 and float(r["x"][5]) < 0.0


def test_a_door_inside_its_range_swings_free(ctx):
    r = solved(ctx, "door-inside")
    sc = r["sc"]
    assert r["tw"]["active"][1] == 0 and r["lam"][5] == 0.0
    want = sc["dt"] * jc.PENDULUM_M * jc.G * jc.PENDULUM_R / (jc.PENDULUM_I + jc.PENDULUM_M * jc.PENDULUM_R ** 2)
    b = _dv_bound(r) + 4 * 2.0 ** -53 * want
    assert abs(r["v6"][0, 4] - want) <= b
