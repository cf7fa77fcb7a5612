"""GPU (-m gpu): capsules through the world -- every entry that detects contacts sees egs_world_set_shapes with
EGS_SHAPE_CAPSULE."""
import numpy as np
import pytest

import capsule_twin as twin
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, G, RAD, LEN = 0.005, 0.2, 9.8, 0.1, 0.6
CAPSULE = capi.SHAPE_CAPSULE


def bodies(sc):
    """A scene's bodies as World.set_bodies takes them; boxes get the 0.3 cube and shape 0."""
    n = sc["p"].shape[0]
    return dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy(),
                Minv=orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36),
                f_ext=orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6),
                side=sc.get("side", np.full((n, 3), 0.3)), shape=sc.get("shape", np.zeros(n, np.int32)))


def join(*ens):
    return {k: np.concatenate([e[k] for e in ens]) for k in ens[0]}


def log(x=0.0, y=0.0, z=RAD - 1e-3, length=LEN):
    """One log along x, by default 1 mm in the ground."""
    e = bodies(scenes.log_pile(1, 1, 1, radius=RAD, length=length, sink=0.0))
    e["p"][0] = [x, y, z]
    return e


def make_world(ctx, ens):
    if len(ens) == 1:
        w, off = capi.World(ctx, ens[0]["p"].shape[0]), np.array([0, ens[0]["p"].shape[0]])
    else:
        w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens])
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6), side=cat("side", 3))
    w.set_shapes(np.concatenate([e["shape"] for e in ens]))
    return w, off


def test_log_laid_in_the_ground_comes_to_rest(ctx):
    """r = 0.1, length 0.6, m = 1, lying along x 1 mm in the ground, 200 steps of dt = 0.005.  Two ground contacts (end 0,
    end 1) at every step.  A step in contact at depth d leaves v_z' = erp d / dt >= 0, so the depth shrinks by at least
    the factor 1 - erp a step until the log is out of contact (z >= r), falls g dt^2 / 2 and is in contact again: as for
    the resting ball, |z - r| <= g dt^2 = 2.45e-4 from then on, and 1e-3 * 0.8^200 is far below that.  In fp64 the log
    never gets out: once the depth is an ulp of r the step's rise, dt erp d / dt = erp d, is below half an ulp and z
    stays where it is, one ulp in the ground, so every one of the 200 steps has both contacts.  The two contacts
    mirror each other in x, so the rows solved to convergence (SOR, tol = 0, 100 sweeps: the 2 x 2 normal system's
    coupling is -1/3, an error factor of 1/9 a sweep) leave no torque: the axis stays horizontal to rounding, |u_z| <=
    1e-12 (the project's bound for a short fp64 chain)."""
    w, _ = make_world(ctx, [log()])
    prm = capi.params(method=capi.SOR, max_iters=100, tol=0.0)
    worst_uz = 0.0
    for step in range(200):
        assert w.step(DT, ERP, prm, want_stats=True).status == capi.OK
        b0, b1, data = w.contacts()
        p, R, v, wv = w.bodies()
        assert len(b0) == 2 and (b0 == -1).all() and data[0, 0] < 0 < data[1, 0], step
        worst_uz = max(worst_uz, abs(R[0, 8]))
    print("lying log: z - r = %.6g (bound g dt^2 = %.6g), max |u_z| = %.3g" % (p[0, 2] - RAD, G * DT * DT, worst_uz))
    assert abs(p[0, 2] - RAD) <= G * DT * DT
    assert worst_uz <= 1e-12
    w.close()


def test_log_bridging_two_cubes(ctx):
    """Two 0.3 cubes 0.6 apart, 1 mm in the ground, and a log of length 0.9 across them, 1 mm in their top faces: one
    contact per cube at every step (each end ball over a face; the flat stretches above the cubes give no third), and
    after 200 steps the log rests at cube height + r within the erp residue of the cube and of the log, 2 g dt^2, and
    so does each of its end balls, which bounds the tilt: e |u_z| <= 2 g dt^2 with e = 0.35.  The scene mirrors itself
    in x, so the log does not slide: |x| <= 1e-6."""
    cubes = bodies(scenes.box_stack(2, 1, 1, gap=0.3))
    cubes["p"][:, 0] -= cubes["p"][:, 0].mean()
    cubes["p"][:, 2] = 0.149
    e = join(cubes, log(z=0.299 + RAD - 1e-3, length=0.9))
    w, _ = make_world(ctx, [e])
    prm = capi.params(method=capi.SOR, max_iters=100, tol=0.0)
    for step in range(200):
        assert w.step(DT, ERP, prm, want_stats=True).status == capi.OK
        b0, b1, _ = w.contacts()
        on = [int(((b0 == k) & (b1 == 2)).sum()) for k in (0, 1)]
        assert on == [1, 1], (step, on)
    p, R, v, wv = w.bodies()
    print("bridge: log z - (0.3 + r) = %.6g, cubes z - 0.15 = %s, bound %.6g" % (p[2, 2] - 0.3 - RAD, p[:2, 2] - 0.15, 2 * G * DT * DT))
    assert abs(p[2, 2] - 0.3 - RAD) <= 2 * G * DT * DT
    assert abs(p[2, 0]) <= 1e-6 and 0.35 * abs(R[2, 8]) <= 2 * G * DT * DT
    w.close()


def test_ball_on_a_logs_side_is_pushed_along_the_twins_normal(ctx):
    """A ball 1 mm in the side of a lying log, off its crest: the pair's contact is the twin's row, bit for bit, its
    normal multiplier is positive and the step separates the two along that normal."""
    ball = bodies(scenes.ball_pile(1, 1, 1, radius=0.1, sink=0.0))
    n_dir = np.array([0.0, 0.6, 0.8])
    ball["p"][0] = np.array([0.05, 0.0, RAD - 1e-3]) + n_dir * (0.2 - 1e-3)
    e = join(log(), ball)
    want = twin.pair(e["p"], e["R"], e["side"], e["shape"], 0, 1)
    assert len(want) == 1
    w, _ = make_world(ctx, [e])
    w.step(DT, ERP, capi.params(method=capi.SOR, max_iters=100, tol=0.0))
    b0, b1, data = w.contacts()
    k = np.flatnonzero((b0 == 0) & (b1 == 1))
    assert len(k) == 1 and data[k[0]].tobytes() == want[0].tobytes()
    n = data[k[0], 3:6]
    assert np.abs(n - n_dir).max() <= 1e-12
    p, R, v, wv = w.bodies()
    lam = w.lambda_().reshape(-1, 3)[k[0]]
    print("ball on log: lambda %s, separating speed %.6g" % (lam, (v[1] - v[0]) @ n))
    assert lam[2] > 0 and (v[1] - v[0]) @ n > 0 and v[1, 1] > 0
    w.close()


def ensembles():
    crib = bodies(scenes.log_pile(1, 3, 2, radius=RAD, length=LEN))
    cube = bodies(scenes.box_stack(1, 1, 1))
    cube["p"][0] = [0.0, 0.5, 0.149]
    ball = bodies(scenes.ball_pile(1, 1, 1, radius=0.1))
    ball["p"][0] = [0.0, 0.0, 3 * RAD - 2e-3]
    mixed = join(log(), cube, ball, log(y=0.5, z=0.299 + RAD - 1e-3))     # a ball on a log, a log across a cube
    pair = bodies(scenes.log_pile(1, 2, 1, radius=RAD, length=LEN, gap=-1e-3))   # two logs side by side, touching
    return [crib, mixed, pair]


def test_batched_world_ensembles_match_their_own_worlds(ctx):
    """A crib, a mixed scene and two logs side by side: after each of 10 steps every ensemble is the world that holds
    it alone, bit for bit -- bodies, contact list, lambda, sweep count."""
    ens = ensembles()
    prm = capi.params(method=capi.SOR, max_iters=40, tol=1e-7, cfm=0.01)
    bw, off = make_world(ctx, ens)
    singles = [make_world(ctx, [e])[0] for e in ens]
    kinds = set()
    for step in range(10):
        bw.step(DT, ERP, prm)
        sst = [s.step(DT, ERP, prm, want_stats=True) for s in singles]
        info = bw.batch_info()
        co = info["contact_offset"]
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
            shape = ens[k]["shape"]
            kinds |= {(int(shape[i]), int(shape[j])) if i >= 0 else (-1, int(shape[j])) for i, j in zip(s0, s1)}
    assert kinds >= {(-1, 0), (-1, 2), (2, 2), (0, 2), (2, 1)}      # ground, log on log, log across the cube, ball on a log
    for w in [bw] + singles:
        w.close()


def test_a_far_capsule_changes_nothing_for_the_others(ctx):
    """Cubes and balls with shapes set and no capsule: the world's first contact list is the context call's (the
    launches of a scene without capsules).  The same bodies with one log added 50 m away, which switches every launch to
    the capsule instantiations: the others' contacts are the same bits and the log has its two."""
    b = bodies(scenes.box_stack(2, 1, 1, gap=-1e-3))
    s = bodies(scenes.ball_pile(2, 1, 1, gap=-1e-3, origin=(0.598, 0.0)))
    e = join(b, s)
    prm = capi.params(method=capi.SOR, max_iters=20, tol=0.0)
    w, _ = make_world(ctx, [e])
    w.step(DT, ERP, prm)
    base = w.contacts()
    direct = ctx.update_contacts_shapes(e["p"], e["R"], e["side"], e["shape"])
    assert len(base[0]) > 8 and all(x.tobytes() == y.tobytes() for x, y in zip(base, direct))
    e2 = join(e, log(x=50.0))
    w2, _ = make_world(ctx, [e2])
    w2.step(DT, ERP, prm)
    c0, c1, cd = w2.contacts()
    mine = c1 == 4
    assert mine.sum() == 2 and (c0[mine] == -1).all()
    # ground contacts come first, by body: the log's two sit between the others' ground contacts and their pairs
    assert all(x.tobytes() == y.tobytes() for x, y in zip((c0[~mine], c1[~mine], cd[~mine]), base))
    w.close(); w2.close()
