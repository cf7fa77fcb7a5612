"""GPU (-m gpu): hinge angle limits in a world (egs_world_set_joint_limits).  Each ensemble of a batch is its own world
bit for bit; the dense steps refuse; a door released under gravity stops at its limit; the stabilise passes take an
active stop as a row of their system."""
import math

import mpmath as mp
import numpy as np
import pytest

import joint_cases as jc
import joint_reference as jr
import limit_reference as lr
import model_reference as mr
from eggshell_amd import capi
from test_gpu_joints_world import make_world as make_joint_world
from test_gpu_world_step_each import ensemble, ensemble_view, same_bits, spaced_chain

pytestmark = pytest.mark.gpu

PRM = dict(method=capi.SOR, max_iters=20, tol=0.0, cfm=0.01)
Y_AXIS = [0.0, 1.0, 0.0]


def door(theta, lo, hi, y=3.0):
    """joint_cases' box hinged to the world about y (its centre 0.5 along x: gravity turns it towards +theta), without
    the motor, standing at `theta` of a range (lo, hi)."""
    e = jc.ens_motored_hinge(y=y)
    e["motors"] = None
    e["limits"] = np.zeros((2, 8))
    e["limits"][1] = lr.limit_row(jc.EYE, Y_AXIS, None, theta, lo, hi)
    return e


def chain_with_limited_hinge():
    """Three spaced links, ball joints link to link and link 0 to the world; links 0 and 1 hinged about y, that hinge
    0.02 rad into a range that ends at 0.01."""
    e = ensemble(spaced_chain(3), joints=True)
    b0, b1, data = e["joints"]
    hd = np.zeros(7); hd[0:6] = Y_AXIS + Y_AXIS
    e["joints"] = (np.append(b0, 0).astype(np.int32), np.append(b1, 1).astype(np.int32), np.vstack([data, hd]))
    e["kinds"] = np.array([jr.BALL] * 3 + [jr.HINGE], np.int32)
    e["motors"] = None
    e["limits"] = np.zeros((4, 8))
    e["limits"][3] = lr.limit_row(jc.EYE, Y_AXIS, jc.EYE, 0.02, -0.5, 0.01)
    return e


def make_world(ctx, ens, precision=capi.F64):
    """test_gpu_joints_world's world, then the ensembles' limit rows (zeros where an ensemble has none)."""
    w, off = make_joint_world(ctx, ens, precision)
    rows = [e["limits"] if e.get("limits") is not None else np.zeros((len(e["joints"][0]), 8)) for e in ens if e["joints"] is not None]
    if any(e.get("limits") is not None for e in ens):
        w.set_joint_limits(np.concatenate(rows))
    return w, off


def three():
    return [door(0.31, -0.5, 0.3), door(-0.31, -0.3, 0.5, y=6.0), chain_with_limited_hinge()]


# ---- 1. each ensemble is its own world ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step", "step_each"])
def test_batched_ensembles_are_their_own_worlds(ctx, entry):
    """E = 3: a door past its upper stop, a door past its lower stop, a chain with one limited hinge; five steps.
    step_each: two rates, and one ensemble sitting each step out."""
    ens = three()
    prm = capi.params(**PRM)
    rates = [[2e-3, 4e-3, 0.0], [2e-3, 0.0, 4e-3], [0.0, 2e-3, 4e-3], [4e-3, 2e-3, 0.0], [2e-3, 4e-3, 4e-3]]
    erps = [0.2, 0.1, 0.3] if entry == "step_each" else [0.2] * 3
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens]
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
                axis = lam[3 * (jo[e + 1] - jo[e] - 1) + 2]      # the hinge is each ensemble's last joint
                pushed[e] = pushed[e] or (axis > 0 if e == 1 else axis < 0)
                assert axis <= 0 if e != 1 else axis >= 0      # one-sided: an upper stop pushes back only, a lower one forward
        assert pushed.all()
    finally:
        bw.close()
        for s in singles:
            s.close()


def test_dense_steps_refuse_a_limited_hinge(ctx):
    """EGS_ERR_UNSUPPORTED from both dense entries, naming the hinge joint, with nothing moved; the world steps on, and
    with the table taken away the refusal is the one of a free hinge."""
    ens = [jc.ens_chain_with_weld(), door(0.1, -0.3, 0.5)]
    ens[1]["motors"] = np.array([[0.0, -1.0], [1.0, 2.0]])      # a motor that would make the axis row a box row
    bw, off = make_world(ctx, ens)
    before = bw.bodies()
    for call in (lambda: bw.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False),
                 lambda: bw.step_dense_each([5e-3, 2e-3], [0.2, 0.2], 0.0, use_bounds=1, detect_contacts=False)):
        with pytest.raises(capi.EgsError) as ei:
            call()
        assert ei.value.status == capi.ERR_UNSUPPORTED and "hinge joint 6" in str(ei.value)
    for a, b in zip(before, bw.bodies()):
        assert same_bits(a, b)
    st = bw.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False, want_stats=True)
    assert st.status == capi.OK and np.isfinite(bw.lambda_()).all()
    bw.set_joint_limits(None)
    assert bw.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False) == 0
    bw.close()


def test_refusals_and_a_new_joint_list(ctx):
    e = door(0.1, -0.3, 0.5)
    w, _ = make_world(ctx, [e])
    for col, val in ((0, np.nan), (1, 0.5), (6, 0.9)):
        bad = e["limits"].copy(); bad[1, col] = val
        with pytest.raises(capi.EgsError) as ei:
            w.set_joint_limits(bad)
        assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(ValueError):
        w.set_joint_limits(e["limits"][:1])
    w.step(5e-3, 0.2, capi.params(**PRM))
    free, _ = make_joint_world(ctx, [e])
    w.set_joints_kinds(e["kinds"], *e["joints"])      # drops the table
    for x in (w, free):
        x.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
        x.step(5e-3, 0.2, capi.params(**PRM))
    for a, b in zip(w.blocks() + w.bodies(), free.blocks() + free.bodies()):
        assert same_bits(a, b)
    w.close(); free.close()


# ---- 2. a door released towards its stop -------------------------------------------------------------------------------------
def _theta(R_row, q):
    """The hinge angle of the world-side door from its R, at 50 digits."""
    sn, cs, _, _ = lr.angle_reference(mr._m3(R_row), None, mr._v(Y_AXIS), mr._v(q))
    return mp.atan2(sn, cs)


def test_a_released_door_stops_at_its_limit(ctx):
    """From rest at theta = 0 towards hi = 0.1 under gravity, 70 steps of dt = 5e-3 (erp 0.2, SOR to 1e-10).

    The bound on the overshoot.  About its hinge the door is a pendulum: theta'' = a cos(theta), a = m g r / (I + m r^2)
    (m = 1, I = 0.1, r = 0.5, g = 9.8), which the world steps as w' = w + a cos(theta) dt; theta += dt (w + w') / 2
    (StepPositions_ODE moves by the mean of the old and the new velocity).  With H = w^2 / 2 - a sin(theta) (H = 0 at the
    release), one such step changes w^2 / 2 by exactly a cos(theta_k) (theta_k+1 - theta_k), and sin is concave on
    [0, pi/2], so H grows by at most a (cos(theta_k) - cos(theta_k+1)) (theta_k+1 - theta_k) <= a sin(theta_k+1)
    (theta_k+1 - theta_k)^2; summed up to an angle theta with steps of at most W dt each, H <= a sin(theta) theta W dt.
    So while the stop has not acted, w^2 / 2 <= a sin(theta) (1 + theta W dt), and the step that first crosses hi starts
    at theta <= hi and ends at theta <= hi + W dt, where W is the least fixed point of
    W = sqrt(2 a sin(hi + W dt) (1 + (hi + W dt) W dt)) -- the energy-bound speed; W dt is one step's travel at it.  The
    door's ball joint is solved with the hinge (its erp term acts along the arm, across the motion), which the 1 per cent
    on top allows for.

    Once the stop is active the solve asks for s^ . w' = -erp sin(excess) / dt.  The step in which the row first acts
    still moves the door by dt (w + w') / 2 with w the speed it arrived with, which no row of that step can change: the
    pose that step leaves may lie past the pose it started from, by dt w / 2 - erp sin(excess) / 2 with w <= W (so over
    every phase of the crossing the largest excess is at most (1 + (1 - erp) / 2) W dt, reached when the crossing step
    itself ends W dt past the stop; on this scene it stays within the one step's travel asserted below).  From that pose
    on both velocities of every update are the row's: excess_k+1 = excess_k - erp (sin(excess_k-1) + sin(excess_k)) / 2,
    so the excess does not grow again."""
    dt, erp, hi = 5e-3, 0.2, 0.1
    e = door(0.0, None, hi)
    q = e["limits"][1, 0:4]
    a = 1.0 * 9.8 * 0.5 / (0.1 + 1.0 * 0.5 ** 2)
    W = math.sqrt(2 * a * math.sin(hi))
    for _ in range(50):
        W = math.sqrt(2 * a * math.sin(hi + W * dt) * (1 + (hi + W * dt) * W * dt))
    bound = 1.01 * W * dt
    w, _ = make_world(ctx, [e])
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-10, cfm=0.0, omega=1.2)
    thetas, lams = [], []
    with mp.workdps(mr.DPS):
        for _ in range(70):
            w.step(dt, erp, prm)
            thetas.append(_theta(w.bodies()[1][0], q))
            lams.append(w.lambda_()[5])
        w.close()
        over = [k for k, t in enumerate(thetas) if t > hi]
        assert over and over[0] > 10, "the door reaches its stop after a free swing"
        first = over[0]
        excess = [float(t - mp.mpf(hi)) for t in thetas]
        print("first step over the stop %d, excess %.3g, after the first active step %.3g, bound %.3g (W %.4g); last excess %.3g" %
              (first, excess[first], excess[first + 1], bound, W, excess[-1]))
        assert all(x == 0.0 for x in lams[:first]) and lams[first + 1] < 0.0
        assert max(excess) <= bound
        # the first active step moves by dt (w + w') / 2: half the arrival speed w <= W, and half the row's own
        # w' = -erp sin(excess) / dt
        assert excess[first + 1] <= excess[first] + 1.01 * W * dt / 2 - erp * math.sin(excess[first]) / 2
        for k in range(first + 1, len(thetas) - 1):      # from the pose the first active step (first + 1) leaves
            assert thetas[k + 1] <= thetas[k], (k, excess[k], excess[k + 1])
        assert excess[-1] < excess[first + 1] * (1 - erp / 2) ** 20


# ---- 3. the stabilise passes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["sweeps", "direct"])
def test_stabilize_brings_a_hinge_back_to_its_stop(ctx, entry):
    """PostStabilize on a door 0.05 rad past its upper stop (err_sq = sin(0.05)^2: the ball joint and the axes are
    exact), beside a door inside its range and one past its lower stop: err_sq falls with every pass, and each ensemble
    of the batch ends with the bits of its own world."""
    ens = [door(0.35, -0.5, 0.3), door(0.1, -0.3, 0.5, y=6.0), door(-0.33, -0.3, 0.5, y=9.0)]
    before = math.sin(0.05) ** 2
    run = (lambda w, k: w.stabilize(capi.STABILIZE_POST, max_steps=k, detect_contacts=False)) if entry == "sweeps" else \
          (lambda w, k: w.stabilize_direct(capi.STABILIZE_POST, max_steps=k, detect_contacts=False))
    seq = [before]
    for k in (1, 2, 3):
        one, _ = make_world(ctx, [ens[0]])
        run(one, k)
        info = one.stabilize_info()
        one.close()
        if info["steps"][0] < k:      # settled before the cap: the passes are over
            break
        seq.append(float(info["err_sq"][0]))
    print("%s: err_sq by pass %s" % (entry, seq))
    assert len(seq) >= 2 and abs(seq[0] - before) < 1e-15
    assert all(b < a for a, b in zip(seq, seq[1:]))
    # every pass: one world relaxed a pass at a time (a pass starts from the bodies the one before left) until it settles
    one, _ = make_world(ctx, [ens[0]])
    every = [before]
    for _ in range(1000):
        run(one, 1)
        info = one.stabilize_info()
        if info["steps"][0] == 0:
            break
        every.append(float(info["err_sq"][0]))
    one.close()
    print("%s: %d passes one at a time, err_sq %.6g -> %.6g; the first three %s" % (entry, len(every) - 1, every[0], every[-1], every[1:4]))
    assert len(every) > 100 and every[-1] <= 1e-9
    assert all(b < a for a, b in zip(every, every[1:]))
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens]
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
