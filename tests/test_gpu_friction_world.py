"""GPU (-m gpu): the friction pyramid in the world (egs_world_set_friction): a world's friction step is Problem.step on
its state and contact list with mu on every contact; in a batched world every ensemble is bit-identical to a world of
its own with its own coefficient, an ensemble with mu < 0 to a world that never heard of friction -- also with warm
start and through egs_world_step_each; the dense steps refuse; and a cube dropped under tilted gravity ends slower with
the larger coefficient."""
import numpy as np
import pytest

import friction_reference as fr
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP = 0.005, 0.2


def pile(nx=2, ny=2, nz=2, push=0.0):
    """A box pile as one ensemble's bodies, with a sideways force on every box so that friction has something to do."""
    sc = scenes.box_stack(nx, ny, nz)
    n = sc["p"].shape[0]
    f = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6).copy()
    f[:, 0] += push
    return dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy(),
                Minv=orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36), f_ext=f)


def make_world(ctx, ens, precision=capi.F64):
    if len(ens) == 1:
        e = ens[0]
        w = capi.World(ctx, e["p"].shape[0], precision)
        off = np.array([0, e["p"].shape[0]])
    else:
        w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens], precision)
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6))
    return w, off


def view(w, off, e):
    """Ensemble e's bodies and lambda rows of a batched world (contacts only: no joints here)."""
    pos, R, v, wv = w.bodies()
    s = slice(off[e], off[e + 1])
    co = w.batch_info()["contact_offset"] if w.n_ensembles > 1 else np.array([0, len(w.contacts()[0])])
    lam = w.lambda_()
    return (pos[s], R[s], v[s], wv[s]), lam[3 * co[e]:3 * co[e + 1]]


@pytest.mark.parametrize("method", [capi.GAUSS_SEIDEL, capi.SOR, capi.JACOBI], ids=["gs", "sor", "jacobi"])
def test_world_step_is_problem_step_with_mu_on_every_contact(ctx, method):
    e = pile(2, 2, 2, push=3.0)
    prm = capi.params(method=method, max_iters=20, tol=0.0, cfm=0.01)
    w, _ = make_world(ctx, [e])
    w.set_friction(0.4)
    st = w.step(DT, ERP, prm, want_stats=True)
    assert st.status == capi.OK and st.schedule & capi.SCHED_FRICTION
    b0, b1, data = w.contacts()
    lam = w.lambda_()
    _, _, v, wv = w.bodies()
    w.close()
    n, m = e["p"].shape[0], b0.shape[0]
    assert m > 0
    pr = capi.Problem(ctx, n, b0, b1)
    pr.set_state(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
    pr.set_constraints(np.full(m, scenes.CONTACT_BOX, np.int32), data)
    pr.set_friction(np.full(m, 0.4))
    ps = pr.step(DT, ERP, prm, want_stats=True)
    assert ps.schedule & capi.SCHED_FRICTION
    assert pr.lambda_().tobytes() == lam.tobytes()
    v6 = pr.velocity()
    assert np.array_equal(v6[:, :3], v) and np.array_equal(v6[:, 3:], wv)
    pr.set_friction(None)
    pr.step(DT, ERP, prm)
    assert pr.lambda_().tobytes() != lam.tobytes()      # the box is another problem
    pr.close()


@pytest.mark.parametrize("mode", ["fixed", "tol", "warm", "each"])
def test_batched_world_ensembles_match_their_own_worlds(ctx, mode):
    """E = 3 piles of 2 x 2 x 2 with mu = (0.3, -1, 0.8): each ensemble is its own world bit for bit over three steps
    (bodies, lambda, sweep count, residual), ensemble 1 a world that never heard of friction."""
    mus = (0.3, -1.0, 0.8)
    ens = [pile(2, 2, 2, push=p) for p in (3.0, 2.0, 4.0)]
    tol = 1e-6 if mode == "tol" else 0.0
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=30, tol=tol, cfm=0.01)
    bw, off = make_world(ctx, ens)
    bw.set_friction(np.array(mus))
    singles = []
    for e, mu in zip(ens, mus):
        s, _ = make_world(ctx, [e])
        if mu >= 0:
            s.set_friction(mu)
        singles.append(s)
    worlds = [bw] + singles
    if mode == "warm":
        for w in worlds:
            w.set_warm_start(True)
    dts = np.array([DT, 0.5 * DT, 2 * DT])
    try:
        for step in range(3):
            if mode == "each":
                bst = bw.step_each(dts, ERP, prm, want_stats=True)
                sst = [s.step_each(dts[k:k + 1], ERP, prm, want_stats=True) for k, s in enumerate(singles)]
            else:
                bst = bw.step(DT, ERP, prm, want_stats=True)
                sst = [s.step(DT, ERP, prm, want_stats=True) for s in singles]
            assert bst.schedule & capi.SCHED_FRICTION
            assert bool(sst[0].schedule & capi.SCHED_FRICTION) and not sst[1].schedule & capi.SCHED_FRICTION
            info = bw.batch_info()
            for k, s in enumerate(singles):
                body, lam = view(bw, off, k)
                for a, b in zip(body, s.bodies()):
                    assert np.array_equal(a, b), (step, k, "bodies")
                assert lam.tobytes() == s.lambda_().tobytes(), (step, k, "lambda")
                assert info["iterations"][k] == sst[k].iterations, (step, k)
                assert np.array_equal(info["residual"][k], sst[k].residual), (step, k)
    finally:
        for w in worlds:
            w.close()


def test_dense_steps_refuse_while_friction_is_on(ctx):
    w, _ = make_world(ctx, [pile(1, 1, 2)])
    w.set_friction(0.5)
    for call in (lambda: w.step_dense(DT, ERP), lambda: w.step_dense_each([DT], ERP)):
        with pytest.raises(capi.EgsError) as e:
            call()
        assert e.value.status == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.EgsError) as e:
        w.set_friction(np.nan)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.EgsError) as e:
        w.set_friction([0.5, 0.5])      # not the world's ensemble count
    assert e.value.status == capi.ERR_INVALID
    w.set_friction(-1.0)
    w.step_dense(DT, ERP, use_bounds=1)      # off: the dense step is taken again (whatever its own outcome)
    w.close()


def test_dropped_cube_under_tilted_gravity_ends_slower_with_more_friction(ctx):
    """Qualitative: 50 steps of a cube dropped from just above the ground under gravity tilted by atan 0.5; the
    one-step test (test_gpu_friction.py) is the quantitative one."""
    case = fr.cube_case()
    vx = {}
    for mu in (0.2, 0.8):
        w = capi.World(ctx, 1)
        p = case["p"].copy(); p[0, 2] += 0.01
        w.set_bodies(p, case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
        w.set_friction(mu)
        prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=50, tol=0.0, cfm=0.0)
        for _ in range(50):
            st = w.step(DT, ERP, prm, want_stats=True)
            assert st.status == capi.OK
        _, _, v, _ = w.bodies()
        assert len(w.contacts()[0]) > 0
        w.close()
        vx[mu] = v[0, 0]
    print("v_x after 50 steps: mu 0.2 -> %.4g, mu 0.8 -> %.4g" % (vx[0.2], vx[0.8]))
    assert vx[0.8] < vx[0.2] and vx[0.2] > 0
