"""GPU (-m gpu): the angular joint blocks (EGS_JOINT_LOCK, EGS_JOINT_HINGE_AXIS) and the hinge motor on a problem.
The assembly against the fp64 twin of tests/joint_reference.py bit for bit; the motor's bounds and target; the schedule
flags; lambda of a step against a 50-digit direct solve of the same bounded system; the dense step and its refusals."""
import math

import mpmath as mp
import numpy as np
import pytest

import joint_cases as jc
import joint_reference as jr
import model_reference as mr
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NAMES = ("J0", "J1", "is_eq", "lo", "hi", "rhs", "err")


def make_problem(ctx, case, precision=capi.F64):
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"], precision)
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    return pr


def assert_twin(got, tw, precision, rows=None, what=""):
    """blocks() against the twin, bit for bit (signs of zero included), in fp32 after the cast; err is fp64 always.
    rows: the constraints compared (default all)."""
    dt = np.float64 if precision == capi.F64 else np.float32
    m = tw["J0"].shape[0]
    sel = np.arange(m) if rows is None else np.asarray(rows)
    r3 = (3 * sel[:, None] + np.arange(3)).reshape(-1)
    for k, name in enumerate(NAMES):
        a, b = np.asarray(got[k]), np.asarray(tw[name])
        if name in ("J0", "J1"):
            ok = jr.bits_equal(a.reshape(m, 18)[sel], b.reshape(m, 18)[sel], dt)
        elif name == "is_eq":
            ok = np.array_equal(a[r3], b[r3])
        else:
            ok = jr.bits_equal(a[r3], b[r3], np.float64 if name == "err" else dt)
        assert ok, (what, name)


# ---- 1. the assembly is the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", jr.IDS)
def test_assembly_is_the_twin(ctx, cid, precision):
    """egs_problem_assemble, then egs_problem_step (whose system is read back after it), then the same list with
    restitution and friction tables set: the joint rows keep their bits."""
    case, motor, _, plain, driven = jr.generated(cid)
    pr = make_problem(ctx, case, precision)
    pr.assemble(case["dt"], case["erp"])
    assert_twin(pr.blocks(), plain, precision, what="assemble")
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=3, tol=0.0, cfm=0.01)
    st = pr.step(case["dt"], case["erp"], prm, want_stats=True)
    assert st.status == capi.OK
    assert_twin(pr.blocks(), plain, precision, what="step")
    m = case["kind"].shape[0]
    pr.set_restitution(np.where(case["kind"] == jr.CONTACT, 0.5, -1.0), 0.0)
    pr.set_friction(np.where(case["kind"] == jr.CONTACT, 0.4, -1.0))
    pr.step(case["dt"], case["erp"], prm)
    assert_twin(pr.blocks(), plain, precision, rows=np.nonzero(case["kind"] != jr.CONTACT)[0], what="tables")
    pr.close()


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", ["n4m8-a", "m259"])
def test_motor_rows_are_the_twin(ctx, cid, precision):
    """Bounds and rhs[2] with the table of the family (tau < 0, 0, +inf, finite; on hinges and on other kinds, where it
    is not applied); motor = NULL afterwards restores the earlier bits."""
    case, motor, _, plain, driven = jr.generated(cid)
    taus = {float(motor[i][1]) for i in range(len(motor)) if case["kind"][i] == jr.HINGE}
    assert {0.0, math.inf} <= taus      # the small family's two hinges: pinned by tau = 0, unlimited
    if cid == "m259":                   # ... and the long list every entry of joint_reference.MOTORS
        assert taus == {t for _, t in jr.MOTORS}
    pr = make_problem(ctx, case, precision)
    pr.assemble(case["dt"], case["erp"])
    before = pr.blocks()
    pr.set_motors(motor)
    pr.assemble(case["dt"], case["erp"])
    assert_twin(pr.blocks(), driven, precision, what="motor")
    st = pr.step(case["dt"], case["erp"], capi.params(method=capi.GAUSS_SEIDEL, max_iters=3, tol=0.0, cfm=0.01), want_stats=True)
    assert_twin(pr.blocks(), driven, precision, what="motor, step")
    pr.set_motors(None)
    pr.assemble(case["dt"], case["erp"])
    after = pr.blocks()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert_twin(after, plain, precision, what="off again")
    pr.close()


def test_refusals(ctx):
    case, motor, _, _, _ = jr.generated("n4m8-a")
    pr = make_problem(ctx, case)
    lock = int(np.nonzero(case["kind"] == jr.LOCK)[0][0]); hinge = int(np.nonzero(case["kind"] == jr.HINGE)[0][0])
    pr.assemble(case["dt"], case["erp"])
    before = pr.blocks()
    for row, col, val in ((lock, 0, case["data"][lock, 0] + 1e-9), (hinge, 1, case["data"][hinge, 1] + 1e-9), (hinge, 4, np.nan),
                          (lock, 6, np.inf)):
        bad = case["data"].copy(); bad[row, col] = val
        with pytest.raises(capi.EgsError) as ei:
            pr.set_constraints(case["kind"], bad)
        assert ei.value.status == capi.ERR_INVALID
    k = case["kind"].copy(); k[0] = 4
    with pytest.raises(capi.EgsError) as ei:
        pr.set_constraints(k, case["data"])
    assert ei.value.status == capi.ERR_INVALID
    for bad in ((np.nan, 1.0), (np.inf, 1.0), (1.0, np.nan)):
        mt = motor.copy(); mt[hinge] = bad
        with pytest.raises(capi.EgsError) as ei:
            pr.set_motors(mt)
        assert ei.value.status == capi.ERR_INVALID
    pr.assemble(case["dt"], case["erp"])
    for a, b in zip(before, pr.blocks()):
        assert a.tobytes() == b.tobytes()
    pr.close()


# ---- 2. schedules ------------------------------------------------------------------------------------------------------------
FORMS = capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_PAIR | capi.SCHED_CHAIN


BASE_ENV = {"EGS_QUAD": "0", "EGS_ISO": "2", "EGS_STEP": "1"}      # the 1-lane isotropic timetable kernel for small piles
FORM_SWITCHES = ("EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY", "EGS_STEP_CHAIN", "EGS_STEP_PAIR", "EGS_STEP_STEADY",
                 "EGS_TILE", "EGS_LANE_ORDER", "EGS_STEP_DEFER_SYSTEM")


def test_a_lock_among_contacts_takes_the_general_schedule(ctx, monkeypatch):
    """The chained piles of tests/step_chain_cases.py ("g32") under the solve of tests/test_gpu_restitution.py's "chain"
    form, which asserts PAIR and CHAIN on them: their contacts alone report LINSYM, FUSED_ASSEMBLY, PAIR and CHAIN, as
    they have since before the angular blocks; with one two-body lock in front of them none of the four is reported,
    and the contacts' rows keep their bits."""
    import bench
    import step_chain_cases as scc
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    for k in FORM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    import step_contact_bounds_cases as sbc
    sc = dict(scc.scene("g32"))
    prm = sbc.params("sor", 5)
    plain, _ = bench.build_problem(ctx, sc, capi.F64)
    plain.step(5e-3, 0.2, prm)
    flags_plain = plain.schedule()      # (egs_problem_get_schedule: the statistics never carry CHAIN)
    blocks_plain = plain.blocks()
    plain.close()
    m = sc["kind"].shape[0]
    with_lock = dict(sc, kind=np.append(jr.LOCK, sc["kind"]).astype(np.int32), body0=np.append(0, sc["body0"]).astype(np.int32),
                     body1=np.append(1, sc["body1"]).astype(np.int32),
                     data=np.vstack([jr.lock_data(sc["R"][0], sc["R"][1]), sc["data"]]))
    pr, _ = bench.build_problem(ctx, with_lock, capi.F64)
    st = pr.step(5e-3, 0.2, prm, want_stats=True)
    flags_lock = pr.schedule() | st.schedule
    got = pr.blocks()
    pr.close()
    print("schedule: contacts alone 0x%x, with a lock 0x%x" % (flags_plain, flags_lock))
    assert st.status == capi.OK and flags_lock & FORMS == 0
    assert flags_plain & FORMS == FORMS
    for a, b in zip(blocks_plain, got):
        a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
        assert a.tobytes() == b[a.size // m:].tobytes()


# ---- 3. the solve against the reference --------------------------------------------------------------------------------------
CLAMP_TAU = 5.0
SOLVES = {"weld": lambda: jc.welded_pair(), "pendulum": lambda: jc.pendulum(), "motor-inf": lambda: jc.pendulum((1.0, math.inf)),
          "motor-clamp": lambda: jc.pendulum((1.0, CLAMP_TAU))}
_solved = {}


def solved(ctx, name):
    """One egs_problem_step per scene (SOR, tol 1e-12, cfm 0), shared by the tests below; with it the reference's lambda,
    the norm of the inverse of the free block and the bound.

    Bound on |lambda - lambda_ref|_inf.  The device's system is the twin's bit for bit (section 1), and the reference
    solves that system exactly, active set included.  At the device's lambda the true residual of the free rows is the
    reported one (their 2-norm, which bounds the largest) plus the rounding of evaluating w = A lambda - rhs through
    J M^-1 J^T: per row at most 32u of the row's magnitude sum (model_reference's factor for a row of this length).  So
        |lambda - lambda_ref|_inf <= |A_ff^-1|_1 (residual + 32u max_r mag_r),
    every term computed here from the reference."""
    if name not in _solved:
        sc = SOLVES[name]()
        pr = jc.make_problem(ctx, sc)
        prm = capi.params(method=capi.SOR, max_iters=20000, tol=1e-12, cfm=0.0, omega=1.2)
        st = pr.step(sc["dt"], sc["erp"], prm, want_stats=True)
        lam, v6, blocks = pr.lambda_(), pr.velocity(), pr.blocks()
        pr.close()
        tw = jr.twin_assemble(sc, sc["motor"])
        assert_twin(blocks, tw, capi.F64, what=name)
        x, norm1, margin = jr.solve_reference(sc, tw, 0.0)
        assert margin > 1e-9, "the scene sits on a tie of its active set: choose another"
        with mp.workdps(mr.DPS):
            N = len(x)
            # row magnitude sums at the reference's lambda, from the dense A of the twin system
            from sweep_reference import system as sweep_system
            s = orc.Sys(sc["Minv"].reshape(-1, 6, 6), sc["body0"], sc["body1"], tw["J0"].reshape(-1, 3, 6), tw["J1"].reshape(-1, 3, 6),
                        tw["is_eq"], tw["lo"], tw["hi"])
            mag = sweep_system(s, 0.0).mag(x, tw["rhs"])
            bound = norm1 * (mp.mpf(st.residual) + 32 * mr.U * max(mag))
        _solved[name] = dict(sc=sc, st=st, lam=lam, v6=v6, x=x, bound=float(bound), norm1=float(norm1), tw=tw)
        print("%s: %d sweeps, residual %.3g, |A_ff^-1|_1 %.3g, bound %.3g" % (name, st.iterations, st.residual, float(norm1), float(bound)))
    return _solved[name]


@pytest.mark.parametrize("name", list(SOLVES))
def test_lambda_against_the_direct_solve(ctx, name):
    r = solved(ctx, name)
    assert r["st"].status == capi.OK and r["st"].iterations < 20000 and r["st"].residual <= 1e-12
    with mp.workdps(mr.DPS):
        worst = max(abs(mp.mpf(float(a)) - b) for a, b in zip(r["lam"], r["x"]))
    print("%s: |lambda - reference|_inf %.3g, bound %.3g" % (name, float(worst), r["bound"]))
    assert worst <= r["bound"]


def _dv_bound(r):
    """What an error of lambda within the bound moves a velocity by, plus the velocity update's own rounding
    (model_reference.velocity_reference's (3 deg + 16) u mag with deg = 2): dt |M^-1 J^T|_inf bound + 22u |v'|."""
    sc, tw = r["sc"], r["tw"]
    W = sc["Minv"].reshape(-1, 6, 6)
    worst = 0.0
    for b in range(W.shape[0]):
        G = np.zeros((6, tw["rhs"].shape[0]))
        for i in range(sc["kind"].shape[0]):
            for Jn, bn in (("J0", "body0"), ("J1", "body1")):
                if sc[bn][i] == b:
                    G[:, 3 * i:3 * i + 3] += np.abs(W[b]) @ np.abs(tw[Jn][i].reshape(3, 6).T)
        worst = max(worst, np.abs(G).sum(axis=1).max())
    return sc["dt"] * worst * r["bound"] * (1 + 1e-9) + 22 * 2.0 ** -53 * max(1.0, np.abs(r["v6"]).max())


def test_welded_pair_leaves_with_one_angular_velocity(ctx):
    r = solved(ctx, "weld")
    d = np.abs(r["v6"][0, 3:] - r["v6"][1, 3:]).max()
    print("weld: |w0' - w1'|_inf %.3g, bound %.3g; w' %s" % (d, 2 * _dv_bound(r), r["v6"][0, 3:]))
    assert d <= 2 * _dv_bound(r)
    # angular momentum about the pair's centre is kept: I w = (2 I + 2 m d^2) w' with I = 0.125, m = 2, d = 0.25, w = 0.5
    assert abs(r["v6"][0, 5] - 0.125) <= 2 * _dv_bound(r)


def test_pendulum_starts_at_the_closed_form(ctx):
    r = solved(ctx, "pendulum")
    sc = r["sc"]
    want = sc["dt"] * jc.PENDULUM_M * jc.G * jc.PENDULUM_R / (jc.PENDULUM_I + jc.PENDULUM_M * jc.PENDULUM_R ** 2)
    w = r["v6"][0, 3:]
    b = _dv_bound(r) + 4 * 2.0 ** -53 * want
    print("pendulum: w' %s, closed form %.17g about y, bound %.3g" % (w, want, b))
    assert abs(w[1] - want) <= b and abs(w[0]) <= b and abs(w[2]) <= b
    assert r["lam"][5] == 0.0      # the pinned axis row


def test_motor_reaches_its_speed_or_its_limit(ctx):
    r = solved(ctx, "motor-inf")
    assert abs(r["v6"][0, 4] - 1.0) <= _dv_bound(r)
    c = solved(ctx, "motor-clamp")
    assert abs(c["lam"][5]) == CLAMP_TAU and c["lam"][5] == float(c["x"][5])
    assert c["v6"][0, 4] < 1.0


# ---- 4. the dense step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ub,cls", [("weld", 0, "single"), ("chain", 0, "single"), ("motors", 1, "single-hard")])
def test_dense_step_against_the_certified_solution(ctx, name, ub, cls):
    from test_gpu_lcp_reference import check_step, device_system
    sc = {"weld": jc.welded_pair, "chain": jc.chain_with_weld, "motors": jc.motored_pair}[name]()
    pr = jc.make_problem(ctx, sc)
    prob = device_system(pr, sc["dt"], sc["erp"], 0.0, ub)
    ok, piv = pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=ub)
    assert ok
    lam = pr.lambda_()
    pr.close()
    check_step(name, "step", cls, prob, lam)


def test_dense_step_refuses_a_pinned_hinge(ctx):
    """A free hinge, a hinge with tau = 0, and any hinge with use_bounds = 0: EGS_ERR_UNSUPPORTED naming the hinge, never
    LCP_FAILED; the problem steps on afterwards."""
    load = capi.load()
    for motor, ub in ((None, 1), ((1.0, 0.0), 1), ((1.0, 3.0), 0)):
        sc = jc.pendulum(motor)
        pr = jc.make_problem(ctx, sc)
        with pytest.raises(capi.EgsError) as ei:
            pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=ub)
        assert ei.value.status == capi.ERR_UNSUPPORTED and "hinge" in str(ei.value)
        st = pr.step(sc["dt"], sc["erp"], capi.params(method=capi.SOR, max_iters=50, tol=0.0, cfm=0.0), want_stats=True)
        assert st.status == capi.OK and np.isfinite(pr.lambda_()).all()
        if motor == (1.0, 3.0):
            ok, _ = pr.step_dense(sc["dt"], sc["erp"], 0.0, use_bounds=1)
            assert ok
        pr.close()
