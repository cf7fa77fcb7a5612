"""GPU (-m gpu): the slider block (EGS_JOINT_SLIDER_AXIS), its motor and its travel stops on a problem.  The assembly
against the fp64 twin of tests/slider_reference.py bit for bit; tables off are the run without them; the schedule flags;
the refusals; lambda of a step against a 50-digit direct solve of the same bounded system; the closed forms of a piston;
the dense step and its refusals."""
import math

import mpmath as mp
import numpy as np
import pytest

import joint_reference as jr
import model_reference as mr
import slider_cases as sc_
import slider_reference as sr
from eggshell_amd import capi
from oracle import oracle as orc
from test_gpu_joints import FORMS, _dv_bound, assert_twin, make_problem

pytestmark = pytest.mark.gpu

GS3 = dict(method=capi.GAUSS_SEIDEL, max_iters=3, tol=0.0, cfm=0.01)
ALL_FORMS = FORMS | capi.SCHED_SHARE | capi.SCHED_FACE


# ---- 1. the assembly is the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", sr.IDS)
def test_assembly_is_the_twin(ctx, cid, precision):
    """egs_problem_assemble, then egs_problem_step (whose system is read back after it); then the motor table (f < 0, 0,
    finite and +inf on sliders and on other kinds); then the stop table beside it; then restitution and friction tables
    beside both (the joints' rows keep their bits); the tables taken away again restore the first bytes.  The 259-row
    list crosses the 256-thread workgroup."""
    case, motor = sr.generated(cid)
    travel = sr.make_travel(case, "mixed")
    fs = {float(motor[i][1]) for i in range(len(motor)) if case["kind"][i] == sr.SLIDER}
    if cid == "m259":
        assert fs == {t for _, t in jr.MOTORS}
    prm = capi.params(**GS3)
    pr = make_problem(ctx, case, precision)
    first = None
    for mt, tv in ((None, None), (motor, None), (None, travel), (motor, travel)):
        tw = sr.twin_assemble(case, mt, tv)
        pr.set_motors(mt)
        pr.set_slider_limits(tv)
        pr.assemble(case["dt"], case["erp"])
        got = pr.blocks()
        first = got if first is None else first
        assert_twin(got, tw, precision, what="assemble %s %s" % (mt is not None, tv is not None))
        st = pr.step(case["dt"], case["erp"], prm, want_stats=True)
        assert st.status == capi.OK and (st.schedule | pr.schedule()) & ALL_FORMS == 0
        assert_twin(pr.blocks(), tw, precision, what="step %s %s" % (mt is not None, tv is not None))
        pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    sl = case["kind"] == sr.SLIDER
    assert (tw["active"][sl] != 0).any()
    if cid == "m259":      # every decision, and a stop under a motor
        assert {-1, 0, 1} <= set(tw["active"][sl]) and (tw["active"][sl & (motor[:, 1] >= 0)] != 0).any()
    pr.set_restitution(np.where(case["kind"] == jr.CONTACT, 0.5, -1.0), 0.0)
    pr.set_friction(np.where(case["kind"] == jr.CONTACT, 0.4, -1.0))
    pr.step(case["dt"], case["erp"], prm)
    assert_twin(pr.blocks(), tw, precision, rows=np.nonzero(case["kind"] != jr.CONTACT)[0], what="tables")
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_restitution(None, 0.0)
    pr.set_friction(None)
    pr.set_motors(None)
    pr.set_slider_limits(None)
    pr.assemble(case["dt"], case["erp"])
    for a, b in zip(first, pr.blocks()):
        assert a.tobytes() == b.tobytes()
    pr.close()


@pytest.mark.parametrize("fam", [f for f in sr.FAMILIES if f != "mixed"])
def test_stop_rows_are_the_twin(ctx, fam):
    """The m = 8 families under every family of stop tables (upper active, lower active, inside, one-sided,
    all-infinite), with the motor table beside them."""
    for cid in ("n4m8-a", "n4m8-b", "n4m8-c"):
        case, motor = sr.generated(cid)
        travel = sr.make_travel(case, fam)
        tw = sr.twin_assemble(case, motor, travel)
        pr = make_problem(ctx, case)
        pr.set_motors(motor)
        pr.set_slider_limits(travel)
        pr.assemble(case["dt"], case["erp"])
        assert_twin(pr.blocks(), tw, capi.F64, what=cid + " " + fam)
        pr.close()


def test_hinge_limits_beside_the_sliders(ctx):
    """A list with a limited hinge and a slider runs the slider form with the hinge limits behind a run-time pointer: the
    m = 8 list with the hinge-limit table, the travel table and the motor table all on, through egs_problem_assemble and
    egs_problem_step, in both precisions; a hinge's stop and a slider's stop are both active."""
    import limit_reference as lr
    case, motor = sr.generated("n4m8-a")
    travel = sr.make_travel(case, "mixed")
    for off in (0, 1):      # upper / lower first on the hinges
        lim = lr.make_limits(case, off)
        for mt in (None, motor):
            tw = sr.twin_assemble(case, mt, travel, hinge_lim=lim)
            hinges, sl = case["kind"] == jr.HINGE, case["kind"] == sr.SLIDER
            assert (tw["active"][hinges] != 0).any() and (tw["active"][sl] != 0).any()
            for precision in (capi.F64, capi.F32):
                pr = make_problem(ctx, case, precision)
                pr.set_motors(mt)
                pr.set_hinge_limits(lim)
                pr.set_slider_limits(travel)
                pr.assemble(case["dt"], case["erp"])
                assert_twin(pr.blocks(), tw, precision, what="both tables, assemble")
                pr.step(case["dt"], case["erp"], capi.params(**GS3))
                assert_twin(pr.blocks(), tw, precision, what="both tables, step")
                pr.close()


@pytest.mark.parametrize("tol", [1e-9, 0.0], ids=["tol", "fixed"])
@pytest.mark.parametrize("travel", [None, (-0.05, math.inf), (-0.5, 0.1)], ids=["no-table", "lower-stop", "both-stops"])
def test_a_vertical_free_piston_falls(ctx, travel, tol):
    """A unit mass on a vertical rail, exactly on it, inside its range: lambda = rhs satisfies every row but the pinned
    rail row, which the stopping test leaves out.  The tolerance-terminated solve (the library's default tol among
    them) starts with that row at its bound and returns lambda = 0 on it, as the fixed sweep count does: the piston
    leaves with -g dt along z and nothing else, within dt tol + 4u g dt."""
    sc = sc_.vertical_piston(travel)
    pr = sc_.make_problem(ctx, sc)
    st = pr.step(sc["dt"], sc["erp"], capi.params(method=capi.SOR, max_iters=200, tol=tol, cfm=0.0, omega=1.2), want_stats=True)
    lam, v6 = pr.lambda_(), pr.velocity()
    pr.close()
    want = -sc_.G * sc["dt"]
    b = sc["dt"] * 1e-9 + 4 * 2.0 ** -53 * abs(want)
    print("vertical piston: %d sweeps, lambda %s, v' %s, want %.17g" % (st.iterations, lam, v6[0], want))
    assert st.status == capi.OK and lam[5] == 0.0
    assert abs(v6[0, 2] - want) <= b and np.abs(np.delete(v6[0], 2)).max() <= b


def _run(pr, case):
    st = pr.step(case["dt"], case["erp"], capi.params(**GS3), want_stats=True)
    return [np.asarray(x).tobytes() for x in pr.blocks()] + [pr.lambda_().tobytes(), pr.velocity().tobytes()], (st.schedule, pr.schedule())


def test_table_off_is_the_run_without_the_call(ctx):
    """No call; lim = None; a table without a finite stop on any slider (stops on the other kinds' rows, which are
    ignored); a table set and taken away; a table followed by a new egs_problem_set_constraints: the same bits and the
    same schedule flags."""
    case, motor = sr.generated("n4m8-a")
    runs = []
    for mode in ("none", "null", "infinite", "taken-away", "constraints-again"):
        pr = make_problem(ctx, case)
        pr.set_motors(motor)
        travel = sr.make_travel(case, "upper")
        if mode == "null":
            pr.set_slider_limits(None)
        elif mode == "infinite":
            pr.set_slider_limits(sr.make_travel(case, "all-infinite"))
        elif mode == "taken-away":
            pr.set_slider_limits(travel)
            pr.step(case["dt"], case["erp"], capi.params(**GS3))
            pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
            pr.set_slider_limits(None)
        elif mode == "constraints-again":
            pr.set_slider_limits(travel)
            pr.set_constraints(case["kind"], case["data"])
            pr.set_motors(motor)
        runs.append(_run(pr, case))
        if mode == "none":
            assert_twin(pr.blocks(), sr.twin_assemble(case, motor), capi.F64, what="no table")
        pr.close()
    for r in runs[1:]:
        assert r[1] == runs[0][1]
        for a, b in zip(runs[0][0], r[0]):
            assert a == b


def test_refusals(ctx):
    """EGS_ERR_INVALID for a rail direction that is no unit vector, NaN data, body0 = -1 and every fault of the stop
    table, on a problem whose table is set: the blocks afterwards are those of the table in force."""
    case, motor = sr.generated("n4m8-a")
    travel = sr.make_travel(case, "mixed")
    sl = np.nonzero(case["kind"] == sr.SLIDER)[0]
    slider, world = int(sl[0]), int(sl[case["body1"][sl] < 0][0])
    ball = int(np.nonzero(case["kind"] == jr.BALL)[0][0])
    pr = make_problem(ctx, case)
    pr.set_slider_limits(travel)
    pr.assemble(case["dt"], case["erp"])
    before = pr.blocks()
    for col, val in ((1, case["data"][slider, 1] + 1e-9), (4, np.nan), (6, np.inf), (0, np.nan)):
        bad = case["data"].copy(); bad[slider, col] = val
        with pytest.raises(capi.EgsError) as ei:
            pr.set_constraints(case["kind"], bad)
        assert ei.value.status == capi.ERR_INVALID
    # body0 = -1: the slider's sides swapped on a problem of its own (the topology is the problem's)
    b0, b1 = case["body0"].copy(), case["body1"].copy()
    b0[world], b1[world] = -1, case["body0"][world]
    sw = capi.Problem(ctx, case["p"].shape[0], b0, b1)
    sw.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    with pytest.raises(capi.EgsError) as ei:
        sw.set_constraints(case["kind"], case["data"])
    assert ei.value.status == capi.ERR_INVALID
    sw.close()
    bad = []
    for row, col, val in ((slider, 0, np.nan), (ball, 1, np.nan), (slider, 0, np.inf), (slider, 1, -np.inf)):
        b = travel.copy(); b[row, col] = val; bad.append(b)
    b = travel.copy(); b[slider] = (0.5, 0.25); bad.append(b)      # xlo > xhi
    for b in bad:
        with pytest.raises(capi.EgsError) as ei:
            pr.set_slider_limits(b)
        assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(ValueError):
        pr.set_slider_limits(travel[:-1])
    ok = travel.copy(); ok[slider] = (0.25, 0.25)      # xlo = xhi is a range
    pr.set_slider_limits(ok)
    pr.set_slider_limits(travel)
    pr.assemble(case["dt"], case["erp"])
    for a, c in zip(before, pr.blocks()):
        assert a.tobytes() == c.tobytes()
    assert_twin(before, sr.twin_assemble(case, None, travel), capi.F64, what="after the refusals")
    pr.close()


# ---- 2. the solve against the reference --------------------------------------------------------------------------------------
CLAMP_F, EXCESS, XHI = 5.0, 1e-3, 0.25
assert CLAMP_F < sc_.PISTON_M * sc_.G * sc_.COS_THETA
SCENES = {"free": lambda: sc_.piston(), "motor": lambda: sc_.piston(motor=(0.25, 100.0)), "motor-clamp": lambda: sc_.piston(motor=(0.0, CLAMP_F)),
          "past-stop": lambda: sc_.piston(travel=(-1.0, XHI), x=XHI + EXCESS)}
_solved = {}


def solved(ctx, name):
    """One egs_problem_step (SOR, tol 1e-12, cfm 0) per scene, with the reference's lambda and test_gpu_joints' bound
    |lambda - lambda_ref|_inf <= |A_ff^-1|_1 (residual + 32u max_r mag_r): the device's system is the twin's bit for bit
    (asserted), the reference solves that system exactly with the active set decided in mpmath."""
    if name not in _solved:
        sc = SCENES[name]()
        pr = sc_.make_problem(ctx, sc)
        st = pr.step(sc["dt"], sc["erp"], capi.params(method=capi.SOR, max_iters=20000, tol=1e-12, cfm=0.0, omega=1.2), want_stats=True)
        lam, v6, blocks = pr.lambda_(), pr.velocity(), pr.blocks()
        pr.close()
        tw = sr.twin_assemble(sc, sc["motor"], sc["travel"])
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
        print("%s: %d sweeps, residual %.3g, |A_ff^-1|_1 %.3g, bound %.3g, lambda of the rail row %.9g" %
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


def _along_and_across(r):
    """(v' . s^, the largest component of v' across the rail, s^): s^ is row 2 of the twin's Rn.  A projection sums three
    components, each within _dv_bound, against a unit vector: within |s^|_1 <= sqrt(3) < 2 times it."""
    s = r["tw"]["J0"][1].reshape(3, 6)[2, 0:3]
    v = r["v6"][0, 0:3]
    along = float(v @ s)
    return along, float(np.abs(v - along * s).max()), s


def test_free_piston_starts_at_the_closed_form(ctx):
    """From rest the free piston leaves with dt g cos(theta) along the rail (s^ points down: g cos(theta) = -g s^_z) and
    nothing across it; its rail row is pinned at 0."""
    r = solved(ctx, "free")
    along, across, s = _along_and_across(r)
    want = r["sc"]["dt"] * sc_.G * -s[2]
    b = 2 * _dv_bound(r) + 4 * 2.0 ** -53 * want
    print("free piston: v' . s^ %.17g, closed form %.17g, across %.3g, bound %.3g" % (along, want, across, b))
    assert abs(-s[2] - sc_.COS_THETA) < 1e-15
    assert abs(along - want) <= b and across <= 3 * b
    assert r["lam"][5] == 0.0 and np.abs(r["v6"][0, 3:]).max() <= b


def test_motor_reaches_its_speed_or_its_limit(ctx):
    """Within its force the motor leaves with its speed; clamped at f < m g cos(theta) with speed 0 it gives way and
    leaves with dt (g cos(theta) - f / m), lambda = -f to the bit."""
    r = solved(ctx, "motor")
    along, _, _ = _along_and_across(r)
    assert abs(along - 0.25) <= 2 * _dv_bound(r) + 4 * 2.0 ** -53 * 0.25 and abs(r["lam"][5]) < 100.0
    c = solved(ctx, "motor-clamp")
    along, across, s = _along_and_across(c)
    want = c["sc"]["dt"] * (sc_.G * -s[2] - CLAMP_F / sc_.PISTON_M)
    b = 2 * _dv_bound(c) + 4 * 2.0 ** -53 * (c["sc"]["dt"] * sc_.G)
    print("clamped motor: v' . s^ %.17g, closed form %.17g, bound %.3g, lambda %.17g" % (along, want, b, c["lam"][5]))
    assert c["lam"][5] == -CLAMP_F and c["lam"][5] == float(c["x"][5])
    assert abs(along - want) <= b and across <= 3 * b


def test_a_piston_past_its_stop_is_pushed_back(ctx):
    """1e-3 past the upper stop the rail row is the stop's: the piston leaves with -erp excess / dt along the rail
    against gravity, lambda <= 0."""
    r = solved(ctx, "past-stop")
    sc, tw = r["sc"], r["tw"]
    assert tw["active"][1] == 1 and (tw["lo"][5], tw["hi"][5]) == (-math.inf, 0.0)
    assert abs(tw["err"][5] - EXCESS) < 1e-15
    along, across, _ = _along_and_across(r)
    want = -sc["erp"] * tw["err"][5] / sc["dt"]
    b = 2 * _dv_bound(r) + 4 * 2.0 ** -53 * abs(want)
    print("past the stop: v' . s^ %.17g, want %.17g, bound %.3g, lambda %.9g" % (along, want, b, r["lam"][5]))
    assert abs(along - want) <= b and across <= 3 * b
    assert r["lam"][5] < 0.0 and float(r["x"][5]) < 0.0


# ---- 3. the dense step ---------------------------------------------------------------------------------------------------------
def test_dense_step_against_the_certified_solution(ctx):
    """A motored slider with f > 0: its rail row is a box row (use_bounds bit 0)."""
    from test_gpu_lcp_reference import check_step, device_system
    sc = sc_.piston(motor=(0.25, 100.0))
    pr = sc_.make_problem(ctx, sc)
    prob = device_system(pr, sc["dt"], sc["erp"], 0.0, 1)
    ok, piv = pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=1)
    assert ok
    lam = pr.lambda_()
    pr.close()
    check_step("piston", "step", "single-hard", prob, lam)


def test_dense_step_refuses_a_free_or_stopped_slider(ctx):
    """A free slider, one with f = 0, a motored one with use_bounds = 0, and any slider with a finite stop (even under a
    motor that would make the row a box row): EGS_ERR_UNSUPPORTED naming the constraint; the problem steps on."""
    for motor, travel, ub in ((None, None, 1), ((1.0, 0.0), None, 1), ((1.0, 3.0), None, 0), ((1.0, 3.0), (-1.0, 1.0), 1)):
        sc = sc_.piston(motor=motor, travel=travel)
        pr = sc_.make_problem(ctx, sc)
        with pytest.raises(capi.EgsError) as ei:
            pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=ub)
        assert ei.value.status == capi.ERR_UNSUPPORTED
        if ub == 1:
            assert "slider constraint 1" in str(ei.value)
        st = pr.step(sc["dt"], sc["erp"], capi.params(method=capi.SOR, max_iters=50, tol=0.0, cfm=0.0), want_stats=True)
        assert st.status == capi.OK and np.isfinite(pr.lambda_()).all()
        if travel is not None:
            pr.set_slider_limits(None)
            ok, _ = pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=1)
            assert ok
        pr.close()
