"""GPU (-m gpu): egs_problem_step with the assembly in the prologue of the LINSYM timetable launch
(step_solve_kernel's ASSEMBLE form).  Over consecutive step + advance calls lambda, v6 and every get_blocks output
must keep the bits of the two-launch path (EGS_FUSED_ASSEMBLY=0) and of the oracle; scenes outside the form's
preconditions (unequal masses, a ball joint between two bodies, tol > 0) must fall back with unchanged results, and a
free body (no constraint) must not disturb it."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import bench
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

STEPS = 3


@contextmanager
def fused_env(value):
    old = os.environ.get("EGS_FUSED_ASSEMBLY")
    if value is None:
        os.environ.pop("EGS_FUSED_ASSEMBLY", None)
    else:
        os.environ["EGS_FUSED_ASSEMBLY"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("EGS_FUSED_ASSEMBLY", None)
        else:
            os.environ["EGS_FUSED_ASSEMBLY"] = old


def c3_piles(batch, heavy=False, joint=False, free=False):
    """`batch` C3 piles (the bench's piles and seeds), optionally with one heavier box, a jointed chain or a free body."""
    nx, ny, nz, _, _, _ = bench.WORKLOADS["c3"]
    piles = [scenes.box_stack(nx, ny, nz, jitter=1e-3, seed=k + 1, origin=(0.0, 100.0 * k)) for k in range(batch)]
    extra = []
    if joint:   # two-body ball joints: J1_lin holds +0 where J0_lin holds +0, not -0
        extra.append(scenes.chain(8, anchor=(0.0, -100.0, 2.0)))
    if free:    # a body without constraints
        one = piles[0]
        extra.append(dict(p=np.array([[0.0, -200.0, 5.0]]), R=one["R"][:1].copy(), v=np.array([[0.1, 0.0, 0.0]]),
                          w=np.zeros((1, 3)), mass=one["mass"][:1].copy(), I_body=one["I_body"][:1].copy(),
                          kind=np.zeros(0, np.int32), body0=np.zeros(0, np.int32), body1=np.zeros(0, np.int32),
                          data=np.zeros((0, 7))))
    sc = scenes.concat(piles + extra)
    if heavy:   # one box of the last pile twice as heavy: unequal linear weights on its contacts
        sc["mass"] = sc["mass"].copy()
        sc["mass"][piles[0]["p"].shape[0] * batch - 1] *= 2.0
    return sc, piles


def run(ctx, sc, prm, env, steps=STEPS):
    """`steps` x (step, advance) with EGS_FUSED_ASSEMBLY = env: per step the state it started from, the stats and the
    outputs as bytes-comparable copies."""
    _, _, _, _, _, dt = bench.WORKLOADS["c3"]
    out = []
    with fused_env(env):
        pr, _ = bench.build_problem(ctx, sc, capi.F64)
        for _ in range(steps):
            state = pr.state()
            st = pr.step(dt, 0.2, prm, want_stats=True)
            out.append(dict(state=state, st=st, lam=pr.lambda_(), v6=pr.velocity(), acc=pr.accumulators(),
                            wres=pr.wres(), blocks=pr.blocks()))
            pr.advance(dt)
        pr.close()
    return out


def assert_same_bytes(new, old):
    assert len(new) == len(old)
    for s, (a, b) in enumerate(zip(new, old)):
        assert a["st"].status == capi.OK and b["st"].status == capi.OK
        assert a["st"].iterations == b["st"].iterations and a["st"].residual == b["st"].residual, "step %d" % s
        for k in ("lam", "v6", "acc", "wres"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), "step %d: %s" % (s, k)
        for k, (x, y) in enumerate(zip(a["blocks"], b["blocks"])):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "step %d: get_blocks output %d" % (s, k)


def oracle_check(sc, piles, out, method, sweeps, omega, which):
    """Every step of piles `which`: the blocks from the oracle's assembly of the state the step started from, lambda and
    the accumulators from its sweep, v6 from its velocity update."""
    _, _, _, _, _, dt = bench.WORKLOADS["c3"]
    Minv, f_ext = bench.host_mass_and_force(sc)
    m1, n1 = piles[0]["kind"].shape[0], piles[0]["p"].shape[0]
    for s, o in enumerate(out):
        pos, R, v, w = o["state"]
        J0g, J1g, is_eqg, log, hig, rhsg, errg = o["blocks"]
        for k in which:
            cons, rows, bod = slice(k * m1, (k + 1) * m1), slice(3 * k * m1, 3 * (k + 1) * m1), slice(k * n1, (k + 1) * n1)
            b0 = np.where(sc["body0"][cons] >= 0, sc["body0"][cons] - k * n1, -1)
            b1 = sc["body1"][cons] - k * n1
            J0, J1, is_eq, lo, hi, err = orc.assemble(pos[bod], R[bod], sc["kind"][cons], b0, b1, sc["data"][cons])
            for name, g, ref in (("J0", J0g[cons], J0), ("J1", J1g[cons], J1), ("is_eq", is_eqg[rows], is_eq),
                                 ("lo", log[rows], lo), ("hi", hig[rows], hi), ("err", errg[rows], err)):
                assert np.array_equal(g.reshape(ref.shape), ref), "step %d pile %d: %s" % (s, k, name)
            sysk = orc.Sys(Minv[bod], b0, b1, J0, J1, is_eq, lo, hi)
            rhs = orc.ode_rhs(v[bod], w[bod], Minv[bod], f_ext[bod], sysk.body0, sysk.body1, J0, J1, err, dt, 0.2)
            assert np.array_equal(rhsg[rows], rhs), "step %d pile %d: rhs" % (s, k)
            xf, af, _, _ = orc.fast_iterate(sysk, rhs, 0.01, method, max_iters=sweeps, tol=0.0, omega=omega)
            assert np.array_equal(o["lam"][rows], xf), "step %d pile %d: lambda" % (s, k)
            assert np.array_equal(o["acc"][bod], af), "step %d pile %d: accumulators" % (s, k)
            v6o = orc.velocity_update(v[bod], w[bod], Minv[bod], f_ext[bod], sysk.body0, sysk.body1, J0, J1, xf, dt)
            assert np.abs(o["v6"][bod] - v6o).max() <= 1e-12 * max(1.0, np.abs(v6o).max()), "step %d pile %d: v6" % (s, k)


def params(method, sweeps, tol=0.0):
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    return capi.params(method=meth, max_iters=sweeps, tol=tol, cfm=0.01, omega=omega), meth, omega


@pytest.mark.parametrize("method", ["gs", "sor"])
def test_fused_bits_c3x24(ctx, method):
    sweeps = bench.WORKLOADS["c3"][3]
    prm, meth, omega = params(method, sweeps)
    sc, piles = c3_piles(24)
    new = run(ctx, sc, prm, None)
    old = run(ctx, sc, prm, "0")
    for o in new:
        assert o["st"].schedule & capi.SCHED_LINSYM and o["st"].schedule & capi.SCHED_FUSED_ASSEMBLY
    for o in old:
        assert o["st"].schedule & capi.SCHED_LINSYM and not o["st"].schedule & capi.SCHED_FUSED_ASSEMBLY
    assert_same_bytes(new, old)
    oracle_check(sc, piles, new, meth, sweeps, omega, which=(0, 23))


@pytest.mark.parametrize("case", ["mixed_mass", "ball_joint", "tol"])
def test_fused_falls_back(ctx, case):
    sweeps = bench.WORKLOADS["c3"][3]
    if case == "tol":
        prm, _, _ = params("gs", 300, tol=1e-7)
    else:
        prm, _, _ = params("gs", sweeps)
    sc, _ = c3_piles(24, heavy=case == "mixed_mass", joint=case == "ball_joint")
    new = run(ctx, sc, prm, None, steps=2)
    old = run(ctx, sc, prm, "0", steps=2)
    for o in new:
        assert not o["st"].schedule & capi.SCHED_FUSED_ASSEMBLY
    assert_same_bytes(new, old)


def test_fused_free_body(ctx):
    """A body without constraints has no tile: the velocity launch covers it, the fused assembly still applies."""
    sweeps = bench.WORKLOADS["c3"][3]
    prm, _, _ = params("gs", sweeps)
    sc, _ = c3_piles(24, free=True)
    new = run(ctx, sc, prm, None, steps=2)
    old = run(ctx, sc, prm, "0", steps=2)
    for o in new:
        assert o["st"].schedule & capi.SCHED_FUSED_ASSEMBLY
    assert_same_bytes(new, old)
