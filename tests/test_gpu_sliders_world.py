"""GPU (-m gpu): sliders in a world (egs_world_set_joints_kinds with EGS_JOINT_SLIDER_AXIS, egs_world_set_joint_motors,
egs_world_set_slider_limits).  Each ensemble of a batch is its own world bit for bit; the stops push one way only; a
motor between two free bodies keeps their momentum; a platform dropped onto a stop; the stabilise passes; the refusals."""
import math

import numpy as np
import pytest

import joint_reference as jr
import slider_cases as sc_
import slider_reference as sr
from eggshell_amd import capi
from test_gpu_world_step_each import ensemble_view, same_bits

pytestmark = pytest.mark.gpu

PRM = dict(method=capi.SOR, max_iters=20, tol=0.0, cfm=0.01)
U = 2.0 ** -53


def three():
    """A piston 1e-3 past its upper stop (on a rail that points down a ramp), one 1e-3 past its lower stop (on a rail that
    points up one), gravity pressing either into its stop; two free bodies on an off-centre slider whose motor pushes them
    apart."""
    return [sc_.ens_piston(0.101, (-0.5, 0.1), axis=(0.0, 0.6, -0.8)), sc_.ens_piston(-0.201, (-0.2, 0.5), axis=(0.6, 0.0, 0.8), origin=(3.0, 0.0, 2.0)),
            sc_.ens_pushed_pair()]


# ---- 1. each ensemble is its own world ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step", "step_each"])
def test_batched_ensembles_are_their_own_worlds(ctx, entry):
    """E = 3, five steps.  step_each: two rates, and one ensemble sitting each step out.  The stops' multipliers are
    one-signed: an upper stop pushes back only, a lower one forward."""
    ens = three()
    prm = capi.params(**PRM)
    rates = [[2e-3, 4e-3, 0.0], [2e-3, 0.0, 4e-3], [0.0, 2e-3, 4e-3], [4e-3, 2e-3, 0.0], [2e-3, 4e-3, 4e-3]]
    erps = [0.2, 0.1, 0.3] if entry == "step_each" else [0.2] * 3
    bw, off = sc_.make_world(ctx, ens)
    singles = [sc_.make_world(ctx, [e])[0] for e in ens]
    pushed = np.zeros(3, bool)
    try:
        for step in range(5):
            dts = rates[step] if entry == "step_each" else [5e-3] * 3
            if entry == "step":
                bw.step(dts[0], erps[0], prm)
            else:
                bw.step_each(np.array(dts), np.array(erps), prm)
            info = bw.batch_info()
            jo = info["joint_offset"]
            for e, s in enumerate(singles):
                if dts[e] == 0.0:
                    continue
                s.step(dts[e], erps[e], prm)
                body, con, lam = ensemble_view(bw, info, off, e)
                assert con[0].size == 0
                assert same_bits(lam, s.lambda_()), (step, e, "lambda")
                for a, b in zip(body, s.bodies()):
                    assert same_bits(a, b), (step, e, "bodies")
                rail = lam[3 * (jo[e + 1] - jo[e] - 1) + 2]      # the slider is each ensemble's last joint
                if e < 2:
                    pushed[e] = pushed[e] or (rail < 0 if e == 0 else rail > 0)
                    assert rail <= 0 if e == 0 else rail >= 0
                else:
                    pushed[e] = pushed[e] or rail != 0.0
        assert pushed.all()
    finally:
        bw.close()
        for s in singles:
            s.close()


def test_each_rates_reach_the_blocks(ctx):
    """egs_world_step_each on the three ensembles with the middle one sitting out: the system of the step is the twin's,
    the motor target and the stop's row taken with the ensemble's own dt and erp, the sitter's rhs rows exactly 0 with its
    bounds in place."""
    from test_gpu_joints import assert_twin
    ens = three()
    for e in ens:      # something for the rows to differ by
        e["v"] = e["v"] + 0.125
    bw, off = sc_.make_world(ctx, ens)
    dts, erps = np.array([2e-3, 0.0, 4e-3]), np.array([0.2, 0.1, 0.3])
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    b0 = np.concatenate([np.where(e["joints"][0] >= 0, e["joints"][0] + o, -1) for e, o in zip(ens, off)]).astype(np.int32)
    b1 = np.concatenate([np.where(e["joints"][1] >= 0, e["joints"][1] + o, -1) for e, o in zip(ens, off)]).astype(np.int32)
    case = dict(p=cat("p", 3), R=cat("R", 9), v=cat("v", 3), w=cat("w", 3), Minv=cat("Minv", 36), f_ext=cat("f_ext", 6),
                kind=np.concatenate([e["kinds"] for e in ens]), body0=b0, body1=b1, data=np.concatenate([e["joints"][2] for e in ens]))
    none2 = lambda e, row: np.tile(row, (len(e["kinds"]), 1))
    motor = np.concatenate([e["motors"] if e["motors"] is not None else none2(e, [0.0, -1.0]) for e in ens])
    travel = np.concatenate([e["travel"] if e["travel"] is not None else none2(e, [-math.inf, math.inf]) for e in ens])
    which = np.concatenate([[k] * len(e["kinds"]) for k, e in enumerate(ens)])
    tw = sr.twin_assemble(case, motor, travel, dt=dts[which], erp=erps[which])
    try:
        bw.step_each(dts, erps, capi.params(**PRM), detect_contacts=False)
        got = bw.blocks()
    finally:
        bw.close()
    assert_twin(got, tw, capi.F64, what="step_each")
    assert list(tw["active"]) == [0, 1, 0, -1, 0, 0]
    rows = np.repeat(which == 1, 3)
    assert np.all(got[5][rows] == 0.0) and (got[3][3 * 3 + 2], got[4][3 * 3 + 2]) == (0.0, math.inf)
    assert (got[3][3 * 1 + 2], got[4][3 * 1 + 2]) == (-math.inf, 0.0) and (got[3][3 * 5 + 2], got[4][3 * 5 + 2]) == (-3.0, 3.0)


# ---- 2. momentum ---------------------------------------------------------------------------------------------------------------
def test_a_motor_between_two_free_bodies_keeps_their_momentum(ctx):
    """Two free bodies, no gravity, an off-centre slider whose motor pushes them apart: whatever lambda the 20 sweeps
    reach, a velocity update adds dt M^-1 J^T lambda, and the slider's and the lock's J0^T lambda + J1^T lambda carry no
    net force and no net torque about the origin (the lever arm sits on body 0 alone).  Per step, at the pose the step
    assembled at: sum m dv = 0 and sum (p x m dv + I dw) = 0 within 64u times the magnitude sum of the terms, which are
    dt |J_side^T| |lambda| per body side (for the torque also |p| x the force's) and the old momenta they are added to,
    computed here from the step's own blocks."""
    e = sc_.ens_pushed_pair(y=0.0)
    w, _ = sc_.make_world(ctx, [e])
    mass, inertia, dt = 1.0, 0.1, 5e-3
    worst = [0.0, 0.0]
    try:
        for step in range(5):
            pos, _, v0, w0 = w.bodies()
            w.step(dt, 0.2, capi.params(**PRM), detect_contacts=False)
            _, _, v1, w1 = w.bodies()
            J0, J1 = w.blocks()[0].reshape(-1, 3, 6), w.blocks()[1].reshape(-1, 3, 6)
            lam = w.lambda_().reshape(-1, 3)
            dP = mass * (v1 - v0).sum(axis=0)
            dL = (np.cross(pos, mass * (v1 - v0)) + inertia * (w1 - w0)).sum(axis=0)
            # ... and the old momenta the update adds them to, m |v| and |p| x m |v| + I |w| per body
            cross_abs = lambda a, f: np.array([a[1] * f[2] + a[2] * f[1], a[2] * f[0] + a[0] * f[2], a[0] * f[1] + a[1] * f[0]])
            magP = mass * np.abs(v0).sum(axis=0)
            magL = sum(cross_abs(np.abs(pos[b]), mass * np.abs(v0[b])) + inertia * np.abs(w0[b]) for b in range(2))
            for i in range(lam.shape[0]):
                for J, b in ((J0[i], 0), (J1[i], 1)):      # body0 is body 0, body1 is body 1 in both joints
                    f = dt * np.abs(J[:, 0:3]).T @ np.abs(lam[i])
                    t = dt * np.abs(J[:, 3:6]).T @ np.abs(lam[i])
                    magP += f
                    magL += t + cross_abs(np.abs(pos[b]), f)
            assert np.abs(lam[1]).max() > 0 and np.abs(v1 - v0).max() > 1e-4
            for k, (d, mag) in enumerate(((dP, magP), (dL, magL))):
                assert np.all(np.abs(d) <= 64 * U * mag), (step, k, d, 64 * U * mag)
                worst[k] = max(worst[k], float(np.max(np.abs(d) / (64 * U * mag + 1e-300))))
        print("momentum drift / bound: linear %.3g, angular %.3g" % tuple(worst))
        assert (w.bodies()[0][1, 0] - w.bodies()[0][0, 0]) > 0.7      # they do move apart
    finally:
        w.close()


# ---- 3. a platform dropped onto its lower stop ---------------------------------------------------------------------------------
def test_a_dropped_platform_stops_at_its_limit(ctx):
    """A unit mass from rest at x = 0 on a vertical rail under gravity towards lo = -0.02, 60 steps of dt = 5e-3 (erp 0.2,
    SOR to tol 1e-10: a tolerance-terminated solve, whose start holds the pinned rail row at its bound).

    The bound on the largest excess.  The free fall is stepped as v' = v - g dt; x += dt (v + v') / 2, which is exact
    for a constant acceleration: after k steps v = -g k dt and x = -g (k dt)^2 / 2.  The stop acts in the first step that
    is assembled with x < lo, step K = the least k with g (k dt)^2 / 2 > |lo|; the platform arrives there with the speed
    v = g K dt, and the step before ended at most v dt past the stop.  The step in which the row first acts still moves
    by dt (v_old + v') / 2 with v_old the arrival speed, which no row of that step can change, and v' = -erp excess / dt:
    v dt / 2 - erp excess / 2 further, so the largest excess is at most (1 + (1 - erp) / 2) v dt.  From the pose that step
    leaves both velocities of every update are the row's, excess_k+1 = excess_k - erp (excess_k-1 + excess_k) / 2: the
    excess shrinks every step.  One per cent on top covers the lock and the two rail equality rows solved with it and the
    solve's tolerance."""
    dt, erp, lo, g = 5e-3, 0.2, -0.02, 9.8
    rail, origin = np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, 2.0])
    e = sc_.ens_piston(0.0, (lo, math.inf))
    K = next(k for k in range(1, 1000) if g * (k * dt) ** 2 / 2 > -lo)
    v = g * K * dt
    bound = 1.01 * (1 + (1 - erp) / 2) * v * dt
    w, _ = sc_.make_world(ctx, [e])
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-10, cfm=0.0, omega=1.2)
    xs, lams = [], []
    try:
        for _ in range(60):
            w.step(dt, erp, prm, detect_contacts=False)
            xs.append(float(rail @ (w.bodies()[0][0] - origin)))      # the travel, from the body's centre
            lams.append(w.lambda_()[5])
    finally:
        w.close()
    under = [k for k, x in enumerate(xs) if x < lo]
    assert under and under[0] == K - 1, "the platform reaches its stop after the free fall of the closed form"
    first = under[0]
    excess = [lo - x for x in xs]
    print("first step under the stop %d, excess %.3g, after the first active step %.3g, largest %.3g, bound %.3g (v %.4g); last %.3g" %
          (first, excess[first], excess[first + 1], max(excess), bound, v, excess[-1]))
    assert all(x == 0.0 for x in lams[:first + 1]) and lams[first + 1] > 0.0      # a lower stop pushes forward only
    assert abs(xs[first] + g * (K * dt) ** 2 / 2) < 1e-9
    assert max(excess) <= bound
    for k in range(first + 1, len(xs) - 1):      # from the pose the first active step (first + 1) leaves
        assert excess[k + 1] < excess[k], (k, excess[k], excess[k + 1])
    assert 0.0 < excess[-1] < excess[first + 1] * (1 - erp / 2) ** 20


# ---- 4. the stabilise passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["sweeps", "direct"])
def test_stabilize_brings_a_slider_back(ctx, entry):
    """PostStabilize on a piston displaced 1e-3 across its rail and 1e-3 past its upper stop (err_sq = 2e-6: the lock is
    exact), beside one inside its range and on its rail and one past its lower stop: err_sq falls with every pass, and
    each ensemble of the batch ends with the bits of its own world."""
    ens = [sc_.ens_piston(0.101, (-0.5, 0.1), across=1e-3), sc_.ens_piston(0.05, (-0.5, 0.1), origin=(0.0, 6.0, 2.0)),
           sc_.ens_piston(-0.201, (-0.2, 0.5), origin=(0.0, 9.0, 2.0), across=-1e-3)]
    before = 2e-6
    run = (lambda w, k: w.stabilize(capi.STABILIZE_POST, max_steps=k, detect_contacts=False)) if entry == "sweeps" else \
          (lambda w, k: w.stabilize_direct(capi.STABILIZE_POST, max_steps=k, detect_contacts=False))
    one, _ = sc_.make_world(ctx, [ens[0]])
    every = [before]
    for _ in range(400):      # one world relaxed a pass at a time (a pass starts from the bodies the one before left)
        run(one, 1)
        info = one.stabilize_info()
        if info["steps"][0] == 0:
            break
        every.append(float(info["err_sq"][0]))
    one.close()
    print("%s: %d passes one at a time, err_sq %.6g -> %.6g; the first three %s" % (entry, len(every) - 1, every[0], every[-1], every[1:4]))
    assert len(every) >= 2 and every[-1] <= 1e-9
    assert all(b < a for a, b in zip(every, every[1:]))
    bw, off = sc_.make_world(ctx, ens)
    singles = [sc_.make_world(ctx, [e])[0] for e in ens]
    left = run(bw, 0)
    info = bw.stabilize_info()
    print("%s: passes %s, final err_sq %s" % (entry, info["steps"], info["err_sq"]))
    assert left == 0 and info["err_sq"][0] <= 1e-9 and info["steps"][0] >= 1 and info["steps"][1] == 0 and info["steps"][2] >= 1
    for e, s in enumerate(singles):
        run(s, 0)
        si = s.stabilize_info()
        assert si["steps"][0] == info["steps"][e] and same_bits(si["err_sq"][:1], info["err_sq"][e:e + 1])
        pos, R, v, wv = bw.bodies()
        sl = slice(off[e], off[e + 1])
        for a, b in zip((pos[sl], R[sl], v[sl], wv[sl]), s.bodies()):
            assert same_bits(a, b), (entry, e)
        s.close()
    bw.close()


@pytest.mark.parametrize("entry", ["sweeps", "direct", "step"])
def test_a_door_and_a_drawer_in_one_world(ctx, entry):
    """A batch that holds a limited hinge and a slider with a stop, so both tables are set on one list: the stabilise
    routes and a step treat each ensemble as its own world does, bit for bit (a door 0.05 rad past its stop, a piston
    1e-3 across its rail and 1e-3 past its stop, and one ensemble with both a limited hinge and a slider)."""
    from test_gpu_limits_world import door
    both = door(0.35, -0.5, 0.3, y=9.0)      # the door's body, hinged to the world, and a second body on a slider to the world
    pist = sc_.ens_piston(0.101, (-0.5, 0.1), origin=(0.0, 12.0, 2.0), across=1e-3)
    both = dict(both, **{k: np.concatenate([both[k].reshape(1, -1), pist[k].reshape(1, -1)]) for k in ("p", "R", "v", "w", "Minv", "f_ext")})
    both["joints"] = (np.concatenate([both["joints"][0], pist["joints"][0] + 1]).astype(np.int32),
                      np.concatenate([both["joints"][1], pist["joints"][1]]).astype(np.int32), np.vstack([both["joints"][2], pist["joints"][2]]))
    both["kinds"] = np.concatenate([both["kinds"], pist["kinds"]]).astype(np.int32)
    both["limits"] = np.vstack([both["limits"], np.zeros((2, 8))])
    both["travel"] = np.vstack([np.tile([-math.inf, math.inf], (2, 1)), pist["travel"]])
    ens = [door(0.35, -0.5, 0.3), sc_.ens_piston(0.101, (-0.5, 0.1), origin=(0.0, 6.0, 2.0), across=1e-3), both]
    run = {"sweeps": lambda w: w.stabilize(capi.STABILIZE_POST, max_steps=0, detect_contacts=False),
           "direct": lambda w: w.stabilize_direct(capi.STABILIZE_POST, max_steps=0, detect_contacts=False),
           "step": lambda w: w.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False)}[entry]
    bw, off = sc_.make_world(ctx, ens)
    singles = [sc_.make_world(ctx, [e])[0] for e in ens]
    run(bw)
    if entry != "step":
        info = bw.stabilize_info()
        print("%s: passes %s, final err_sq %s" % (entry, info["steps"], info["err_sq"]))
        assert np.all(info["err_sq"] <= 1e-9) and np.all(info["steps"] >= 1)
    for e, s in enumerate(singles):
        run(s)
        if entry != "step":
            si = s.stabilize_info()
            assert si["steps"][0] == info["steps"][e] and same_bits(si["err_sq"][:1], info["err_sq"][e:e + 1])
        pos, R, v, wv = bw.bodies()
        sl = slice(off[e], off[e + 1])
        for a, b in zip((pos[sl], R[sl], v[sl], wv[sl]), s.bodies()):
            assert same_bits(a, b), (entry, e)
        s.close()
    bw.close()


def test_a_vertical_free_piston_falls_in_a_world(ctx):
    """egs_world_step with the library's default parameters (tol 1e-9 > 0) on a unit mass on a vertical rail, alone and
    in a batch beside a cairn-free second piston with a stop: five steps of free fall, v = -g k dt to dt tol + rounding,
    the rail row's multiplier exactly 0."""
    import ctypes
    prm = capi.SolveParams()
    capi.load().egs_default_params(ctypes.byref(prm))
    assert prm.tol > 0
    dt = 5e-3
    ens = [sc_.ens_piston(0.0, None), sc_.ens_piston(0.0, (-0.5, 0.1), origin=(0.0, 6.0, 2.0))]
    for group in ([ens[0]], ens):
        w, off = sc_.make_world(ctx, group)
        try:
            for k in range(1, 6):
                w.step(dt, 0.2, prm, detect_contacts=False)
                v, lam = w.bodies()[2], w.lambda_().reshape(-1, 3)
                assert np.all(lam[1::2, 2] == 0.0)
                assert np.abs(v[:, 2] + 9.8 * k * dt).max() <= k * (dt * prm.tol + 8 * U * 9.8 * dt), (k, v)
                assert np.abs(v[:, :2]).max() <= k * dt * prm.tol
        finally:
            w.close()


def test_err_sq_of_the_displaced_piston_is_the_twins(ctx):
    """... and the err the passes start from is the twin's: (1e-3 across)^2 + (1e-3 past the stop)^2."""
    e = sc_.ens_piston(0.101, (-0.5, 0.1), across=1e-3)
    case = dict(p=e["p"], R=e["R"], v=e["v"], w=e["w"], Minv=e["Minv"], f_ext=e["f_ext"], kind=e["kinds"], body0=e["joints"][0],
                body1=e["joints"][1], data=e["joints"][2], dt=1.0, erp=0.2)
    tw = sr.twin_assemble(case, None, e["travel"])
    assert tw["active"][1] == 1 and abs(float(np.sum(tw["err"] ** 2)) - 2e-6) < 1e-12
    w, _ = sc_.make_world(ctx, [e])
    w.stabilize_direct(capi.STABILIZE_POST, max_steps=1, detect_contacts=False)
    after = float(w.stabilize_info()["err_sq"][0])
    w.close()
    assert after < float(np.sum(tw["err"] ** 2))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_a_new_joint_list(ctx):
    e = sc_.ens_piston(0.05, (-0.5, 0.1))
    w, _ = sc_.make_world(ctx, [e])
    b0, b1, data = e["joints"]
    for row, col, val in ((1, 0, math.nan), (0, 1, math.nan), (1, 0, math.inf), (1, 1, -math.inf), (1, 0, 0.2)):
        bad = e["travel"].copy(); bad[row, col] = val
        with pytest.raises(capi.EgsError) as ei:
            w.set_slider_limits(bad)
        assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(ValueError):
        w.set_slider_limits(e["travel"][:1])
    for d in (np.vstack([data[0], data[1] * 1.001]), np.vstack([data[0], np.where(np.arange(7) == 4, math.nan, data[1])])):
        with pytest.raises(capi.EgsError) as ei:
            w.set_joints_kinds(e["kinds"], b0, b1, d)
        assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(capi.EgsError) as ei:      # body0 = -1
        w.set_joints_kinds(e["kinds"], b1, b0, data)
    assert ei.value.status == capi.ERR_INVALID
    w.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False)
    free, _ = sc_.make_world(ctx, [dict(e, travel=None)])
    w.set_joints_kinds(e["kinds"], b0, b1, data)      # drops the table
    for x in (w, free):
        x.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
        x.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False)
    for a, b in zip(w.blocks() + w.bodies(), free.blocks() + free.bodies()):
        assert same_bits(a, b)
    w.close(); free.close()


def test_dense_steps_refuse_a_free_or_stopped_slider(ctx):
    """EGS_ERR_UNSUPPORTED from both dense entries, naming the slider joint, with nothing moved; the world steps on; with
    the table taken away and a motor with f > 0 the dense step runs."""
    ens = [sc_.ens_pushed_pair(), sc_.ens_piston(0.05, (-0.5, 0.1), motor=(0.25, 30.0))]
    bw, off = sc_.make_world(ctx, ens)
    before = bw.bodies()
    for call in (lambda: bw.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False),
                 lambda: bw.step_dense_each([5e-3, 2e-3], [0.2, 0.2], 0.0, use_bounds=1, detect_contacts=False)):
        with pytest.raises(capi.EgsError) as ei:
            call()
        assert ei.value.status == capi.ERR_UNSUPPORTED and "slider joint 3" in str(ei.value)
    for a, b in zip(before, bw.bodies()):
        assert same_bits(a, b)
    st = bw.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False, want_stats=True)
    assert st.status == capi.OK and np.isfinite(bw.lambda_()).all()
    bw.set_slider_limits(None)
    assert bw.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False) == 0
    bw.set_joint_motors(None)      # free sliders: pinned rail rows
    with pytest.raises(capi.EgsError) as ei:
        bw.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "slider joint 1" in str(ei.value)
    bw.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False)
    bw.close()
