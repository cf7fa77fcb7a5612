"""GPU (-m gpu): spheres through the world -- every entry that detects contacts sees egs_world_set_shapes."""
import mpmath as mp
import numpy as np
import pytest

import sphere_twin as twin
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, G, RAD = 0.005, 0.2, 9.8, 0.15


def bodies(sc):
    """A scene's bodies as World.set_bodies takes them; boxes get the 0.3 cube and shape 0."""
    n = sc["p"].shape[0]
    return dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy(),
                Minv=orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36),
                f_ext=orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6),
                side=sc.get("side", np.full((n, 3), 0.3)), shape=sc.get("shape", np.zeros(n, np.int32)))


def ball(z=RAD, vx=0.0):
    e = bodies(scenes.ball_pile(1, 1, 1, radius=RAD, sink=0.0))
    e["p"][0, 2] = z
    e["v"][0, 0] = vx
    return e


def make_world(ctx, ens, shapes=True):
    if len(ens) == 1:
        w, off = capi.World(ctx, ens[0]["p"].shape[0]), np.array([0, ens[0]["p"].shape[0]])
    else:
        w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens])
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6), side=cat("side", 3))
    if shapes:
        w.set_shapes(np.concatenate([e["shape"] for e in ens]))
    return w, off


def test_resting_ball_stays_put(ctx):
    """r = 0.15, m = 1, started at z = r, 50 steps of dt = 0.005 with SOR at its defaults.  Nothing acts sideways, so
    x, y, v_x, v_y and w stay exactly 0.  Bound on |z - r|, from erp, dt and g alone: at z = r the ball is not in
    contact (z < 0 strictly), so step 1 is free fall, g dt^2 / 2 down, leaving v_z = -g dt.  A step in contact at depth
    d solves the normal row for v_z' = erp d / dt >= 0 (rhs = -erp err / dt^2 - J u, err = -d), so the midpoint rule
    moves the ball by dt (v_z + v_z') / 2 >= -g dt^2 / 2 in step 2 and upwards (both velocities >= 0) afterwards,
    d' = d - erp (d_prev + d) / 2 < d: the depth never exceeds g dt^2 and never becomes a height.  Hence
    |z - r| <= g dt^2 = 2.45e-4."""
    w, _ = make_world(ctx, [ball()])
    prm = capi.params(method=capi.SOR)
    bound = G * DT * DT
    worst = 0.0
    for _ in range(50):
        assert w.step(DT, ERP, prm, want_stats=True).status == capi.OK
        p, R, v, wv = w.bodies()
        assert p[0, 0] == 0 and p[0, 1] == 0 and v[0, 0] == 0 and v[0, 1] == 0 and (wv == 0).all()
        worst = max(worst, abs(p[0, 2] - RAD))
    print("resting ball: max |z - r| = %.6g, bound g dt^2 = %.6g" % (worst, bound))
    assert worst <= bound
    w.close()


def test_rolling_ball_reaches_five_sevenths(ctx):
    """The same ball with v_x = 0.7 and no spin under the friction box (|lambda_t| <= 1): it slides for 40 steps,
    then rolls.  m v r + I w about the contact point is conserved by any contact impulse with lever arm r, so
    v_x -> (5/7) 0.7 = 0.5 and w_y = v_x / r.  Tolerance, from the CPU alone: the restatement of this step loop
    (sphere_twin.ball_steps) is E_57 = |v - 5/7 v0| and E_roll = |v - w r| away from the two statements at 50 digits,
    and its fp64 run differs from its 50-digit run by D; the device gets E + 16 D.  Measured on the CPU: E_57 = 2e-51,
    E_roll = 0, D = 9.8e-17 (so the bound is 1.6e-15).  The rows are solved to convergence as in the restatement
    (SOR, tol = 0, 100 sweeps: the row matrix is diagonal, the error halves per sweep); the default tol = 1e-9
    would leave dt 1e-9 = 5e-12 of slip at the contact point."""
    steps, v0 = 80, 0.7
    x, z, vx, vz, wy = twin.ball_steps(RAD, 1.0, v0, steps, DT, ERP, g=G)
    with mp.workdps(50):
        X, Z, VX, VZ, WY = twin.ball_steps(RAD, 1.0, v0, steps, DT, ERP, g=G, num=mp.mpf)
        D = float(max(abs(mp.mpf(vx) - VX), abs(mp.mpf(wy) - WY) * mp.mpf(RAD)))
        E57, Eroll = float(abs(VX - mp.mpf(5) / 7 * mp.mpf(v0))), float(abs(VX - WY * mp.mpf(RAD)))
    w, _ = make_world(ctx, [ball(vx=v0)])
    prm = capi.params(method=capi.SOR, max_iters=100, tol=0.0)
    for _ in range(steps):
        assert w.step(DT, ERP, prm, want_stats=True).status == capi.OK
    p, R, v, wv = w.bodies()
    w.close()
    d57, droll = abs(v[0, 0] - 5.0 / 7.0 * v0), abs(v[0, 0] - wv[0, 1] * RAD)
    print("rolling ball: device |v - 5/7 v0| = %.3g (bound %.3g), |v - w r| = %.3g (bound %.3g); restatement fp64 v = %.17g, "
          "device v = %.17g" % (d57, E57 + 16 * D, droll, Eroll + 16 * D, vx, v[0, 0]))
    assert v[0, 1] == 0 and wv[0, 0] == 0 and wv[0, 2] == 0
    assert d57 <= E57 + 16 * D
    assert droll <= Eroll + 16 * D


def mixed():
    """Two cubes and two balls in a row, each 1 mm into its neighbour and into the ground."""
    b = bodies(scenes.box_stack(2, 1, 1, gap=-1e-3))
    s = bodies(scenes.ball_pile(2, 1, 1, gap=-1e-3, origin=(0.598, 0.0)))
    return {k: np.concatenate([b[k], s[k]]) for k in b}


def ensembles():
    empty = {k: v[:0] for k, v in ball().items()}
    return [bodies(scenes.ball_pile(2, 2, 2)), bodies(scenes.box_stack(2, 1, 2)), mixed(), empty]


def test_batched_world_ensembles_match_their_own_worlds(ctx):
    """Balls only, boxes only, mixed, empty: after each of 10 steps every ensemble is the world that holds it alone,
    bit for bit -- bodies, contact list, lambda, sweep count."""
    ens = ensembles()
    prm = capi.params(method=capi.SOR, max_iters=40, tol=1e-7, cfm=0.01)
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens[:3]]
    kinds = set()
    for step in range(10):
        bw.step(DT, ERP, prm)
        sst = [s.step(DT, ERP, prm, want_stats=True) for s in singles]
        info = bw.batch_info()
        co = info["contact_offset"]
        assert co[3] == co[4]                                      # the empty ensemble has no contacts
        B, C, lam = bw.bodies(), bw.contacts(), bw.lambda_()
        for k, s in enumerate(singles):
            sl = slice(off[k], off[k + 1])
            for a, b in zip(B, s.bodies()):
                assert np.array_equal(a[sl], b), (step, k, "bodies")
            cs = slice(co[k], co[k + 1])
            s0, s1, sd = s.contacts()
            assert np.array_equal(np.where(C[0][cs] >= 0, C[0][cs] - off[k], -1), s0) and np.array_equal(C[1][cs] - off[k], s1)
            assert C[2][cs].tobytes() == sd.tobytes(), (step, k, "contacts")
            assert lam[3 * co[k]:3 * co[k + 1]].tobytes() == s.lambda_().tobytes(), (step, k, "lambda")
            assert info["iterations"][k] == sst[k].iterations, (step, k)
            if k == 2:
                shape = ens[2]["shape"]
                kinds |= {(int(shape[i]), int(shape[j])) if i >= 0 else (-1, int(shape[j])) for i, j in zip(s0, s1)}
    assert kinds >= {(-1, 0), (-1, 1), (0, 0), (0, 1), (1, 1)}         # the mixed ensemble met every pairing
    for w in [bw] + singles:
        w.close()


def test_dense_step_and_direct_stabilize_see_the_ball(ctx):
    """One egs_world_step_dense of a ball 1 mm in the ground: the LCP is solved directly, so v_z is the erp form's
    erp d / dt to rounding (1e-12, the project's bound for a short fp64 chain).  egs_world_stabilize_direct (INIT,
    detection on) of a ball 0.05 deep: no ensemble left unsettled, i.e. err_sq = depth^2 <= 1e-9, its own tolerance."""
    d = 1e-3
    w, _ = make_world(ctx, [ball(z=RAD - d)])
    assert w.step_dense(DT, ERP) == 0
    p, R, v, wv = w.bodies()
    assert len(w.contacts()[0]) == 1
    assert abs(v[0, 2] - ERP * d / DT) <= 1e-12 and v[0, 0] == 0 and v[0, 1] == 0 and (wv == 0).all()
    w.close()
    w, _ = make_world(ctx, [ball(z=RAD - 0.05)])
    assert w.stabilize_direct(capi.STABILIZE_INIT, detect_contacts=True) == 0
    p, R, v, wv = w.bodies()
    info = w.stabilize_info()
    print("stabilize_direct: z - r = %.3g after %d passes, err_sq %.3g" % (p[0, 2] - RAD, info["steps"][0], info["err_sq"][0]))
    assert info["err_sq"][0] <= 1e-9
    assert -np.sqrt(1e-9) <= p[0, 2] - RAD <= 0.05 and p[0, 0] == 0 and p[0, 1] == 0
    w.close()
    # without the shapes the same body is a 0.3 cube 0.05 deep: four contacts, not one
    w, _ = make_world(ctx, [ball(z=RAD - 0.05)], shapes=False)
    w.step_dense(DT, ERP)
    assert len(w.contacts()[0]) == 4
    w.close()


def test_set_shapes_null_returns_to_boxes(ctx):
    """After a sphere run, set_shapes(None) + the same bodies again is a fresh box world, bit for bit, warm start on."""
    e = mixed()
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=30, tol=0.0, cfm=0.01)
    w, _ = make_world(ctx, [e])
    fresh, _ = make_world(ctx, [e], shapes=False)
    for x in (w, fresh):
        x.set_warm_start(True)
    for _ in range(3):
        w.step(DT, ERP, prm)
    as_spheres = w.contacts()
    w.set_shapes(None)
    w.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"], side=e["side"])
    for step in range(3):
        w.step(DT, ERP, prm)
        fresh.step(DT, ERP, prm)
        for a, b in zip(w.bodies() + w.contacts() + (w.lambda_(),), fresh.bodies() + fresh.contacts() + (fresh.lambda_(),)):
            assert a.tobytes() == b.tobytes(), step
        if step == 0:
            assert len(w.contacts()[0]) != len(as_spheres[0])   # (and no history survived: fresh has none)
    w.close(); fresh.close()
