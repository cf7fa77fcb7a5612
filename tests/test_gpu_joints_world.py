"""GPU (-m gpu): welds and hinges in a world (egs_world_set_joints_kinds, egs_world_set_joint_motors).  Each ensemble
of a batch is its own world bit for bit; the per-ensemble rates reach the motor's target; all-ball kinds are
egs_world_set_joints; the collider prunes against the ball joints only; the stabilise passes take the new kinds."""
import numpy as np
import pytest

import joint_cases as jc
import joint_reference as jr
from eggshell_amd import capi, scenes
from test_gpu_world_step_each import bodies, ensemble, ensemble_view, same_bits, spaced_chain

pytestmark = pytest.mark.gpu

PRM = dict(method=capi.SOR, max_iters=20, tol=0.0, cfm=0.01)


def set_joints(w, ens, off):
    """The ensembles' joints with global body indices, their kinds and their motors (rows (0, -1) where an ensemble has
    none)."""
    b0, b1, data, kind, motor, any_motor = [], [], [], [], [], False
    for e, o in zip(ens, off):
        if e["joints"] is None:
            continue
        j0, j1, jd = e["joints"]
        b0.append(np.where(j0 >= 0, j0 + o, -1)); b1.append(np.where(j1 >= 0, j1 + o, -1)); data.append(jd)
        kind.append(e["kinds"] if e.get("kinds") is not None else np.zeros(len(j0), np.int32))
        motor.append(e["motors"] if e.get("motors") is not None else np.tile([0.0, -1.0], (len(j0), 1)))
        any_motor = any_motor or e.get("motors") is not None
    if not b0:
        return
    w.set_joints_kinds(np.concatenate(kind), np.concatenate(b0), np.concatenate(b1), np.concatenate(data))
    if any_motor:
        w.set_joint_motors(np.concatenate(motor))


def make_world(ctx, ens, precision=capi.F64):
    """A plain world for one ensemble, a batched one for several: (world, body offsets)."""
    if len(ens) == 1:
        w, off = capi.World(ctx, ens[0]["p"].shape[0], precision), np.array([0, ens[0]["p"].shape[0]])
    else:
        w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens], precision)
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6))
    set_joints(w, ens, off)
    return w, off


def three():
    return [jc.ens_chain_with_weld(), jc.ens_motored_hinge(), jc.ens_cairn()]


# ---- 1. each ensemble is its own world ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step", "step_each"])
def test_batched_ensembles_are_their_own_worlds(ctx, entry):
    """E = 3: a chain with a weld, a motored hinge whose motor clamps, a cairn without joints; five steps."""
    ens = three()
    prm = capi.params(**PRM)
    dts, erps = ([2e-3, 5e-3, 4e-3], [0.2, 0.1, 0.3]) if entry == "step_each" else ([5e-3] * 3, [0.2] * 3)
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens]
    try:
        for step in range(5):
            if entry == "step":
                bw.step(dts[0], erps[0], prm)
            else:
                bw.step_each(np.array(dts), np.array(erps), prm)
            info = bw.batch_info()
            for e, s in enumerate(singles):
                s.step(dts[e], erps[e], prm)
                body, con, lam = ensemble_view(bw, info, off, e)
                for a, b in zip(con, s.contacts()):
                    assert np.array_equal(a, b), (step, e, "contacts")
                assert same_bits(lam, s.lambda_()), (step, e, "lambda")
                for a, b in zip(body, s.bodies()):
                    assert same_bits(a, b), (step, e, "bodies")
        lam = bw.lambda_()
        jo = bw.batch_info()["joint_offset"]
        assert abs(lam[3 * (jo[1] + 1) + 2]) == 2.0      # the motor of ensemble 1 sits on its torque limit
        assert np.any(lam[3 * jo[0] + 12:3 * jo[0] + 15] != 0.0)      # the weld's lock carries load
    finally:
        bw.close()
        for s in singles:
            s.close()


def test_each_rates_reach_the_blocks(ctx):
    """egs_world_step_each on joints only (no detection), two ensembles with different dt and one sitting out: the
    system of the step is the twin's, the motor target taken with the ensemble's own dt, the rows of the ensemble that
    sits out exactly 0 with its bounds in place."""
    ens = [jc.ens_chain_with_weld(), jc.ens_motored_hinge(), jc.ens_motored_hinge(y=6.0)]
    ens[2]["motors"] = np.array([[0.0, -1.0], [-0.5, np.inf]])
    for e in ens:      # something for the target to differ from
        e["w"] = e["w"] + 0.25
    bw, off = make_world(ctx, ens)
    dts, erps = np.array([2e-3, 0.0, 4e-3]), np.array([0.2, 0.1, 0.3])
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    b0 = np.concatenate([np.where(e["joints"][0] >= 0, e["joints"][0] + o, -1) for e, o in zip(ens, off)]).astype(np.int32)
    b1 = np.concatenate([np.where(e["joints"][1] >= 0, e["joints"][1] + o, -1) for e, o in zip(ens, off)]).astype(np.int32)
    case = dict(p=cat("p", 3), R=cat("R", 9), v=cat("v", 3), w=cat("w", 3), Minv=cat("Minv", 36), f_ext=cat("f_ext", 6),
                kind=np.concatenate([e["kinds"] for e in ens]), body0=b0, body1=b1, data=np.concatenate([e["joints"][2] for e in ens]))
    motor = np.concatenate([e["motors"] if e["motors"] is not None else np.tile([0.0, -1.0], (len(e["kinds"]), 1)) for e in ens])
    which = np.concatenate([[k] * len(e["kinds"]) for k, e in enumerate(ens)])
    tw = jr.twin_assemble(case, motor, dt=dts[which], erp=erps[which])
    try:
        bw.step_each(dts, erps, capi.params(**PRM), detect_contacts=False)
        got = bw.blocks()
    finally:
        bw.close()
    from test_gpu_joints import assert_twin
    assert_twin(got, tw, capi.F64, what="step_each")
    out = which == 1
    rows = np.repeat(out, 3)
    assert np.all(got[5][rows] == 0.0) and got[4][3 * 6 + 2] == 2.0 and got[3][3 * 6 + 2] == -2.0
    assert got[5][3 * 8 + 2] != got[5][3 * 6 + 2]


def test_all_ball_kinds_are_set_joints(ctx):
    sc = spaced_chain(4)
    e = ensemble(sc, joints=True)
    out = []
    for kinds in ("set_joints", "null", "zeros"):
        w = capi.World(ctx, 4)
        w.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
        if kinds == "set_joints":
            w.set_joints(*e["joints"])
        else:
            w.set_joints_kinds(None if kinds == "null" else np.zeros(4, np.int32), *e["joints"])
        for _ in range(3):
            st = w.step(5e-3, 0.2, capi.params(**PRM), want_stats=True)
        out.append(list(w.bodies()) + [w.lambda_(), np.array([st.schedule, st.iterations]), np.array([st.residual])] + list(w.blocks()))
        w.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert same_bits(a, b)


def test_refusals(ctx):
    e = jc.ens_chain_with_weld()
    w = capi.World(ctx, 4)
    w.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
    b0, b1, data = e["joints"]
    for kinds, d in ((np.array([0, 0, 0, 0, 1], np.int32), data), (np.array([0, 0, 0, 0, 7], np.int32), data),
                     (e["kinds"], np.vstack([data[:4], data[4] * 1.001]))):
        with pytest.raises(capi.EgsError) as ei:
            w.set_joints_kinds(kinds, b0, b1, d)
        assert ei.value.status == capi.ERR_INVALID
    w.set_joints_kinds(e["kinds"], b0, b1, data)
    with pytest.raises(capi.EgsError) as ei:
        w.set_joint_motors(np.tile([np.nan, 1.0], (5, 1)))
    assert ei.value.status == capi.ERR_INVALID
    w.step(5e-3, 0.2, capi.params(**PRM))
    w.close()
    # across two ensembles
    bw, off = capi.World.batch(ctx, [2, 2])
    with pytest.raises(capi.EgsError) as ei:
        bw.set_joints_kinds(np.array([jr.LOCK], np.int32), np.array([0], np.int32), np.array([2], np.int32), jr.lock_data(jc.EYE, jc.EYE)[None])
    assert ei.value.status == capi.ERR_INVALID
    bw.close()


# ---- 2. the dense steps --------------------------------------------------------------------------------------------------------
def test_world_dense_step_and_its_refusal(ctx):
    """A free hinge in a batch: egs_world_step_dense returns EGS_ERR_UNSUPPORTED naming the hinge and moves nothing; with
    a motor (0 < tau) on every hinge it solves, each ensemble as its own world."""
    ens = [jc.ens_chain_with_weld(), jc.ens_motored_hinge()]
    free = [jc.ens_chain_with_weld(), dict(jc.ens_motored_hinge(), motors=None)]
    bw, off = make_world(ctx, free)
    before = bw.bodies()
    for ub in (0, 1):
        with pytest.raises(capi.EgsError) as ei:
            bw.step_dense(5e-3, 0.2, 0.0, use_bounds=ub, detect_contacts=False)
        assert ei.value.status == capi.ERR_UNSUPPORTED and "hinge" in str(ei.value)
    for a, b in zip(before, bw.bodies()):
        assert same_bits(a, b)
    bw.step(5e-3, 0.2, capi.params(**PRM), detect_contacts=False)      # still usable
    bw.close()
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens]
    with pytest.raises(capi.EgsError) as ei:
        bw.step_dense(5e-3, 0.2, 0.0, use_bounds=0, detect_contacts=False)
    assert ei.value.status == capi.ERR_UNSUPPORTED
    assert bw.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False) == 0
    info = bw.batch_info()
    for e, s in enumerate(singles):
        assert s.step_dense(5e-3, 0.2, 0.0, use_bounds=1, detect_contacts=False) == 0
        body, _, lam = ensemble_view(bw, info, off, e)
        assert same_bits(lam, s.lambda_())
        for a, b in zip(body, s.bodies()):
            assert same_bits(a, b)
        s.close()
    bw.close()


# ---- 3. the collider sees the ball joints only ---------------------------------------------------------------------------------
def test_pruning_takes_the_ball_joints_only(ctx):
    """Two stacked boxes welded at a point within 1e-6 of one of their contact points: that contact is pruned, and the
    list is the one of a world that holds the weld's ball joint alone."""
    sc = scenes.box_stack(1, 1, 2)
    e = ensemble(sc)
    free = ctx.update_contacts(e["p"], e["R"])
    pair = np.nonzero((free[0] == 0) & (free[1] == 1))[0]
    assert pair.size >= 1
    x = free[2][pair[0], 0:3] + np.array([3e-7, 0.0, 0.0])
    R0, R1 = e["R"][0].reshape(3, 3), e["R"][1].reshape(3, 3)
    ball = np.concatenate([R0.T @ (x - e["p"][0]), R1.T @ (x - e["p"][1]), [0.0]])
    lists = []
    for with_lock in (True, False):
        w = capi.World(ctx, 2)
        w.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
        if with_lock:
            w.set_joints_kinds(np.array([jr.BALL, jr.LOCK], np.int32), np.zeros(2, np.int32), np.ones(2, np.int32),
                               np.vstack([ball, jr.lock_data(R0, R1)]))
        else:
            w.set_joints(np.zeros(1, np.int32), np.ones(1, np.int32), ball[None])
        w.step(5e-3, 0.2, capi.params(**PRM))
        lists.append(w.contacts())
        w.close()
    for a, b in zip(*lists):
        assert same_bits(a, b)
    assert lists[0][0].shape[0] == free[0].shape[0] - 1
    assert not np.any(np.all(np.abs(lists[0][2][:, 0:3] - free[2][pair[0], 0:3]) < 1e-12, axis=1))


# ---- 4. the stabilise passes -----------------------------------------------------------------------------------------------------
def bent_weld(angle=0.05, y=0.0):
    """Two boxes 0.6 apart welded as they stand, then body 1 turned by `angle` about z: the lock's error is sin(angle)
    about z and the ball anchor is off by the turn of its arm."""
    sc = bodies([[0.0, y, 1.0], [0.6, y, 1.0]])
    e = ensemble(sc)
    data = np.zeros((2, 7))
    data[0, 0:6] = [0.3, 0.0, 0.0, -0.3, 0.0, 0.0]
    data[1] = jr.lock_data(jc.EYE, jc.EYE)
    c, s = np.cos(angle), np.sin(angle)
    e["R"][1] = np.array([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0])
    e["joints"] = (np.zeros(2, np.int32), np.ones(2, np.int32), data)
    e["kinds"], e["motors"] = np.array([jr.BALL, jr.LOCK], np.int32), None
    return e


@pytest.mark.parametrize("entry", ["sweeps", "direct"])
def test_stabilize_straightens_a_bent_weld(ctx, entry):
    """PostStabilize on a weld bent by 0.05 rad beside a hinged chain: err_sq after one pass is below err_sq before (the
    twin's err at the initial pose), it converges, and each ensemble of the batch ends with the bits of its own world."""
    hinge = jc.ens_motored_hinge()
    ens = [bent_weld(), hinge, bent_weld(0.03, y=4.0)]
    tw = jr.twin_assemble(dict(p=ens[0]["p"], R=ens[0]["R"], v=ens[0]["v"], w=ens[0]["w"], Minv=ens[0]["Minv"], f_ext=ens[0]["f_ext"],
                               kind=ens[0]["kinds"], body0=ens[0]["joints"][0], body1=ens[0]["joints"][1], data=ens[0]["joints"][2],
                               dt=1.0, erp=0.2))
    before = float(np.sum(tw["err"] ** 2))
    assert abs(tw["err"][5] - (-np.sin(0.05))) < 1e-15 and before > 1e-3
    run = (lambda w, k: w.stabilize(capi.STABILIZE_POST, max_steps=k, detect_contacts=False)) if entry == "sweeps" else \
          (lambda w, k: w.stabilize_direct(capi.STABILIZE_POST, max_steps=k, detect_contacts=False))
    one, _ = make_world(ctx, [ens[0]])
    run(one, 1)
    after1 = one.stabilize_info()["err_sq"][0]
    one.close()
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens]
    left = run(bw, 0)
    info = bw.stabilize_info()
    print("%s: err_sq before %.3g, after one pass %.3g; passes to converge %s, final err_sq %s" %
          (entry, before, after1, info["steps"], info["err_sq"]))
    assert after1 < before
    assert left == 0 and info["err_sq"][0] <= 1e-9 < before
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
