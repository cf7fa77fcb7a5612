"""GPU (-m gpu): live inertia (egs_problem_set_live_inertia / egs_world_set_live_inertia).  With it on, every stepping
entry first recomputes on the device, from the R and w it holds, what Ensemble::Init would compute at that state for
every body whose inertia_body is not a multiple of the identity: the bits of the CPU oracle's minv_blocks /
external_force (certified against 40 digits in test_inertia_reference_cpu.py).  Checked here: those bits; the defining
equivalence -- a live world is bit for bit the frozen world whose host re-uploads the oracle's values before every
step; the oracle's own step; worlds of cubes untouched; the physics it is for; the refusals."""
import numpy as np
import pytest

import live_inertia_cases as lic
from eggshell_amd import capi, scenes
from helpers import ode_step
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP = lic.DT, 0.2


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_bodies(n, seed):
    """n bodies with random R and w and full symmetric positive definite I_b; every third body exactly isotropic; an
    applied torque on every other body (zero rows elsewhere)."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    R = np.array([scenes._quat_to_R(*qq) for qq in q])
    I = np.zeros((n, 9))
    for b in range(n):
        if b % 3 == 2:
            I[b] = (np.eye(3) * rng.uniform(0.01, 0.2)).reshape(9)
        else:
            A = rng.uniform(-1, 1, (3, 3))
            S = A @ A.T + 0.05 * np.eye(3)
            I[b] = (0.1 * (S + S.T) / 2.0).reshape(9)
    torque = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(-1, 1, (n, 3)), 0.0)
    return dict(p=rng.uniform(-1, 1, (n, 3)) + [0, 0, 5], R=R, v=rng.uniform(-1, 1, (n, 3)), w=rng.uniform(-3, 3, (n, 3)),
                mass=rng.uniform(0.5, 2.0, n), I_body=I, torque=torque)


def chain_topology(n):
    """a ball joint between neighbours, the first held to the world: n constraints"""
    b0 = np.arange(n, dtype=np.int32)
    b1 = np.append(np.arange(1, n, dtype=np.int32), -1).astype(np.int32)
    b0[n - 1] = 0
    data = np.zeros((n, 7))
    data[:, 0:3] = [0.15, -0.15, 0.15]
    data[:, 3:6] = [-0.15, 0.15, -0.15]
    return np.zeros(n, np.int32), b0, b1, data


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_refresh_bits(ctx, n):
    sc = random_bodies(n, 100 + n)
    rng = np.random.default_rng(n)
    # what the caller uploads: its own linear rows, and angular parts that only the skipped bodies keep
    Minv_up = rng.uniform(0.5, 2.0, (n, 36))
    f_up = rng.uniform(-1, 1, (n, 6))
    kind, b0, b1, data = chain_topology(n)
    pr = capi.Problem(ctx, n, b0, b1)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv_up, f_up)
    pr.set_constraints(kind, data)
    pr.set_live_inertia(sc["I_body"], sc["torque"])
    pr.assemble(DT, ERP)
    Minv, f_ext = pr.mass()
    want_M, want_f = lic.host_mass(sc["R"], sc["w"], sc["mass"], sc["I_body"], Minv_up, f_up, sc["torque"])
    skipped = lic.is_skipped(sc["I_body"])
    assert skipped.sum() == n // 3
    assert same_bits(Minv, want_M) and same_bits(f_ext, want_f)
    # said again, part by part: the angular 3x3 and the torque rows of the live bodies are the oracle's ...
    oM = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 6, 6)
    oF = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    assert same_bits(Minv.reshape(n, 6, 6)[~skipped][:, 3:, 3:], oM[~skipped][:, 3:, 3:])
    assert same_bits(f_ext[~skipped][:, 3:], sc["torque"][~skipped] + oF[~skipped][:, 3:])
    # ... and every linear row, every off-diagonal 3x3 and every skipped body is what was uploaded
    keep = np.ones((n, 6, 6), bool)
    keep[~skipped, 3:, 3:] = False
    assert same_bits(Minv.reshape(n, 6, 6)[keep], Minv_up.reshape(n, 6, 6)[keep])
    assert same_bits(f_ext[:, :3], f_up[:, :3]) and same_bits(f_ext[skipped], f_up[skipped])
    # the assembly that followed read the refreshed Wf: its rhs is the oracle's with these arrays
    J0, J1, is_eq, lo, hi, rhs, err = pr.blocks()
    want_rhs = orc.ode_rhs(sc["v"], sc["w"], want_M, want_f, b0, b1, J0, J1, err, DT, ERP)
    assert same_bits(rhs, want_rhs)
    pr.close()


def test_refresh_without_a_torque_and_idempotent(ctx):
    n = 257
    sc = random_bodies(n, 7)
    Minv_up = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_up = np.zeros((n, 6))
    kind, b0, b1, data = chain_topology(n)
    pr = capi.Problem(ctx, n, b0, b1)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv_up, f_up)
    pr.set_constraints(kind, data)
    pr.set_live_inertia(sc["I_body"])
    pr.assemble(DT, ERP)
    first = pr.mass()
    want = lic.host_mass(sc["R"], sc["w"], sc["mass"], sc["I_body"], Minv_up, f_up)
    assert same_bits(first[0], want[0]) and same_bits(first[1], want[1])      # (-0.0 rows included: no 0 + t)
    pr.assemble(DT, ERP)
    again = pr.mass()
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
    pr.close()


@pytest.mark.parametrize("method", [capi.GAUSS_SEIDEL, capi.SOR])
def test_fp32_problem_solves_with_the_rounded_blocks(ctx, method):
    """The working-precision copy the refresh writes is (float) of the fp64 value: the fp32 solve it feeds is the fp32
    oracle's on float32(Minv), as the fp32 parity tests compare."""
    n = 64
    sc = random_bodies(n, 11)
    sc["v"] *= 0.0
    Minv_up = orc.minv_blocks(sc["R"], sc["mass"], np.tile((np.eye(3) * 0.1).reshape(9), (n, 1)))
    f_up = np.zeros((n, 6)); f_up[:, 2] = -9.8 * sc["mass"]
    kind, b0, b1, data = chain_topology(n)
    pr = capi.Problem(ctx, n, b0, b1, precision=capi.F32)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv_up, f_up)
    pr.set_constraints(kind, data)
    pr.set_live_inertia(sc["I_body"], sc["torque"])
    pr.assemble(DT, ERP)
    Minv, f_ext = pr.mass()
    want_M, want_f = lic.host_mass(sc["R"], sc["w"], sc["mass"], sc["I_body"], Minv_up, f_up, sc["torque"])
    assert same_bits(Minv, want_M) and same_bits(f_ext, want_f)
    J0, J1, is_eq, lo, hi, rhs, err = pr.blocks()
    pr.solve(capi.params(method=method, max_iters=20, tol=0.0, cfm=0.02))
    x32, a32 = pr.lambda_().astype(np.float32), pr.accumulators().astype(np.float32)
    s = orc.Sys(want_M, b0, b1, J0, J1, is_eq, lo, hi)
    xo, ao = orc.fast_iterate_f32(s, rhs, 0.02, method, max_iters=20)[:2]
    assert same_bits(x32, xo.reshape(x32.shape)) and same_bits(a32, ao.reshape(a32.shape))
    pr.close()


# ---- the defining equivalence ---------------------------------------------------------------------------------------
def make_world(ctx, sc, joints, live):
    n = sc["p"].shape[0]
    w = capi.World(ctx, n)
    w.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], sc["Minv"], sc["f_ext"])
    if joints:
        w.set_joints(sc["body0"], sc["body1"], sc["data"])
    if live:
        w.set_live_inertia(sc["I_body"])
    return w


def host_refresh(w, sc, Minv, f_ext):
    """The route a caller had to take before: read the bodies back, the oracle's values with the skip rule, upload."""
    _, R, _, wv = w.bodies()
    Minv, f_ext = lic.host_mass(R, wv, sc["mass"], sc["I_body"], Minv, f_ext)
    w.set_bodies(None, None, None, None, Minv, f_ext)
    return Minv, f_ext


def assert_same_world(a, b, what):
    for x, y, name in zip(a.bodies(), b.bodies(), ("pos", "R", "v", "w")):
        assert same_bits(x, y), (what, name)
    ia, ib = a.info(), b.info()
    assert ia["n_constraints"] == ib["n_constraints"] and ia["n_contacts"] == ib["n_contacts"], what
    for x, y, name in zip(a.contacts(), b.contacts(), ("body0", "body1", "data")):
        assert same_bits(x, y), (what, "contact " + name)
    assert same_bits(a.lambda_(), b.lambda_()), (what, "lambda")


def equivalence(ctx, sc, joints, step, steps=30):
    live, frozen = make_world(ctx, sc, joints, True), make_world(ctx, sc, joints, False)
    Minv, f_ext = sc["Minv"], sc["f_ext"]
    for k in range(steps):
        Minv, f_ext = host_refresh(frozen, sc, Minv, f_ext)
        step(live); step(frozen)
        assert_same_world(live, frozen, k)
    Ml, fl = live.mass()
    _, R, _, wv = live.bodies()
    want = lic.host_mass(R, wv, sc["mass"], sc["I_body"], Minv, f_ext)
    assert same_bits(Ml, want[0]) and same_bits(fl, want[1])      # get_mass: the arrays of the state the device holds now
    moved = np.abs(live.bodies()[1] - sc["R"]).max()
    live.close(); frozen.close()
    return moved


def test_equivalence_free_brick(ctx):
    sc = lic.free_brick_bodies("random")
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20, tol=0.0, cfm=0.01)
    moved = equivalence(ctx, sc, False, lambda w: w.step(DT, ERP, prm, detect_contacts=False))
    assert moved > 1e-2      # it did tumble


@pytest.mark.parametrize("route", ["gs", "sor", "dense"])
def test_equivalence_chain_of_bricks(ctx, route):
    sc = lic.brick_chain(4)
    assert np.allclose(np.diag(lic.BRICK), [0.0375, 0.0308333333, 0.0083333333])
    if route == "dense":
        step = lambda w: w.step_dense(DT, ERP, 0.01, 0, detect_contacts=False)
    else:
        prm = capi.params(method=capi.GAUSS_SEIDEL if route == "gs" else capi.SOR, max_iters=50, tol=1e-9, cfm=0.01)
        step = lambda w: w.step(DT, ERP, prm, detect_contacts=False)
    assert equivalence(ctx, sc, True, step) > 1e-4


def dropped_bricks():
    rng = np.random.default_rng(3)
    n = 3
    sc = dict(p=np.array([[0.0, 0.0, 0.152 + 0.31 * k] for k in range(n)]), R=np.tile(np.eye(3).reshape(9), (n, 1)),
              v=np.zeros((n, 3)), w=rng.uniform(-2, 2, (n, 3)), mass=np.ones(n), I_body=np.tile(lic.BRICK.reshape(9), (n, 1)))
    sc["Minv"] = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    sc["f_ext"] = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    return sc


def test_equivalence_dropped_bricks_with_contacts(ctx):
    """Three spinning bricks a little above the ground and each other: contacts come and go over the 30 steps."""
    sc = dropped_bricks()
    prm = capi.params(method=capi.SOR, max_iters=60, tol=1e-9, cfm=0.01)
    live, frozen = make_world(ctx, sc, False, True), make_world(ctx, sc, False, False)
    Minv, f_ext = sc["Minv"], sc["f_ext"]
    counts = []
    for k in range(30):
        Minv, f_ext = host_refresh(frozen, sc, Minv, f_ext)
        live.step(5e-3, ERP, prm, detect_contacts=True); frozen.step(5e-3, ERP, prm, detect_contacts=True)
        assert_same_world(live, frozen, k)
        counts.append(live.info()["n_contacts"])
    print("contacts per step:", counts)
    assert len(set(counts)) > 1 and max(counts) > 0
    live.close(); frozen.close()


# ---- against the oracle's step --------------------------------------------------------------------------------------
def test_chain_of_bricks_against_the_oracle_step(ctx):
    """20 dense steps of the brick chain; each is compared with the oracle's step (helpers.ode_step) restarted from the
    device's own state with Minv0 / f_ext0 recomputed there, so nothing accumulates.  Tolerance: the 1e-9 that
    test_gpu_adapter2.py holds the frozen dense step to."""
    sc = lic.brick_chain(4)
    w = make_world(ctx, sc, True, True)
    for k in range(20):
        p, R, v, wv = w.bodies()
        st = dict(sc, p=p, R=R, v=v, w=wv)
        st["Minv0"] = orc.minv_blocks(R, sc["mass"], sc["I_body"])
        st["f_ext0"] = orc.external_force(R, wv, sc["mass"], sc["I_body"])
        lam = ode_step(st, DT, ERP)
        assert w.step_dense(DT, ERP, 0.01, 0, detect_contacts=False) == 0
        for got, want, name in zip(w.bodies(), (st["p"], st["R"], st["v"], st["w"]), ("pos", "R", "v", "w")):
            assert np.abs(got - want).max() < 1e-9, (k, name)
        assert np.abs(w.lambda_() - lam).max() < 1e-9 * max(1.0, np.abs(lam).max()), k
    w.close()


# ---- cubes are untouched ----------------------------------------------------------------------------------------------
def test_cubes_are_untouched(ctx):
    sc = scenes.box_stack(2, 2, 2)
    n = sc["p"].shape[0]
    assert lic.is_skipped(sc["I_body"]).all() and np.array_equal(sc["I_body"][0], (0.1 * np.eye(3)).reshape(9))
    Minv = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=30, tol=0.0, cfm=0.01)
    out = []
    for live in (True, False):
        w = capi.World(ctx, n)
        w.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
        if live:
            w.set_live_inertia(sc["I_body"])
        sched = [w.step(5e-3, ERP, prm, detect_contacts=True, want_stats=True).schedule for _ in range(5)]
        out.append((sched, w.bodies(), w.lambda_(), w.mass()))
        w.close()
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert same_bits(x, y)
    assert same_bits(out[0][2], out[1][2])
    assert same_bits(out[0][3][0], Minv) and same_bits(out[0][3][1], f_ext)
    # the problem entries: the same schedule bits from egs_problem_get_schedule, SCHED_ISO among them where it applies
    res = []
    for live in (True, False):
        pr = capi.Problem(ctx, n, sc["body0"], sc["body1"])
        pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
        pr.set_constraints(sc["kind"], sc["data"])
        if live:
            pr.set_live_inertia(sc["I_body"])
        st = pr.step(5e-3, ERP, prm, want_stats=True)
        res.append((st.schedule, pr.schedule(), pr.lambda_(), pr.velocity()))
        pr.close()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert same_bits(res[0][2], res[1][2]) and same_bits(res[0][3], res[1][3])


# ---- physics on the device ------------------------------------------------------------------------------------------
def device_run(ctx, start, steps, live):
    sc = lic.free_brick_bodies(start)
    w = make_world(ctx, sc, False, live)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20, tol=0.0)
    t = lic.Tumble(sc["R"], sc["w"])
    for _ in range(steps):
        w.step(DT, ERP, prm, detect_contacts=False)
        _, R, _, wv = w.bodies()
        t.see(R, wv)
    state = w.bodies()
    w.close()
    return t, state


def test_device_brick_keeps_its_angular_momentum_live_only(ctx):
    live, state = device_run(ctx, "random", 1000, True)
    frozen, _ = device_run(ctx, "random", 1000, False)
    print("L drift: live %.3e, frozen %.3e; energy change: live %.3e, frozen %.3e" %
          (live.drift, frozen.drift, live.energy_change, frozen.energy_change))
    assert live.drift <= 1e-2
    assert frozen.drift >= 0.5
    twin, tstate = lic.twin_run("random", 1000, True)
    assert np.abs(state[1] - tstate["R"]).max() < 1e-9 and np.abs(state[3] - tstate["w"]).max() < 1e-9      # the oracle twin


def test_device_brick_flips_about_its_intermediate_axis_live_only(ctx):
    live, _ = device_run(ctx, "intermediate", 4000, True)
    frozen, _ = device_run(ctx, "intermediate", 4000, False)
    print("flips: live", live.flips, "frozen", frozen.flips)
    assert live.flips and 1000 < live.flips[0] < 2000
    assert frozen.flips == []


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_null_turns_it_off(ctx):
    sc = lic.brick_chain(4)
    w = make_world(ctx, sc, True, True)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20, tol=0.0, cfm=0.01)
    w.step(DT, ERP, prm, detect_contacts=False)
    before = w.mass()
    nan = sc["I_body"].copy(); nan[2, 4] = np.nan
    inf_torque = np.zeros((4, 3)); inf_torque[1, 0] = np.inf
    skew = sc["I_body"].copy(); skew[1, 1] = 1e-5          # I[0][1] != I[1][0]
    indefinite = sc["I_body"].copy(); indefinite[3] = np.diag([0.03, -0.01, 0.02]).reshape(9)
    semi = sc["I_body"].copy(); semi[0] = np.array([[1.0, 1.0, 0], [1.0, 1.0, 0], [0, 0, 1.0]]).reshape(9)
    for bad, torque in ((nan, None), (sc["I_body"], inf_torque), (skew, None), (indefinite, None), (semi, None)):
        with pytest.raises(capi.EgsError) as e:
            w.set_live_inertia(bad, torque)
        assert e.value.status == capi.ERR_INVALID
        after = w.mass()
        assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    # still on: a step moves the arrays with the bodies
    w.step(DT, ERP, prm, detect_contacts=False)
    moved = w.mass()
    assert not same_bits(before[0], moved[0])
    # NULL turns it off: steps leave them alone from here on
    w.set_live_inertia(None)
    held = w.mass()
    for _ in range(3):
        w.step(DT, ERP, prm, detect_contacts=False)
    off = w.mass()
    assert same_bits(held[0], off[0]) and same_bits(held[1], off[1])
    w.close()
