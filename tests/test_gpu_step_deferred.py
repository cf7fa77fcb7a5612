"""GPU (-m gpu): egs_problem_step on the store-free fused launch (step_solve_kernel's ASSEMBLE form with
STORE_SYSTEM = false).  The launch leaves J0, J1, rhs, lo, hi, err and is_eq unwritten, the problem makes them on demand
(ensure_system) from the state the step read.  Whatever is read after
whatever sequence of calls must keep the bits of the eager path (EGS_STEP_DEFER_SYSTEM=0): GS and backward SOR, on three
small piles in one partly filled 256-lane tile (inactive lanes, ground contacts with a body on side 1 only)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import bench
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, SWEEPS = 5e-3, 0.2, 20


@contextmanager
def env(**values):
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def small_piles(free=False):
    piles = [scenes.box_stack(2, 2, 3, jitter=1e-3, seed=k, origin=(0.0, 100.0 * k)) for k in range(3)]
    if free:    # a body without constraints: no slot in any tile
        one = piles[0]
        piles.append(dict(p=np.array([[0.0, -200.0, 5.0]]), R=one["R"][:1].copy(), v=np.array([[0.1, 0.0, 0.0]]),
                          w=np.zeros((1, 3)), mass=one["mass"][:1].copy(), I_body=one["I_body"][:1].copy(),
                          kind=np.zeros(0, np.int32), body0=np.zeros(0, np.int32), body1=np.zeros(0, np.int32),
                          data=np.zeros((0, 7))))
    return scenes.concat(piles)


def params(method, sweeps=SWEEPS, tol=0.0):
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    return capi.params(method=meth, max_iters=sweeps, tol=tol, cfm=0.01, omega=omega)


def run(ctx, sc, sequence, defer, fused=None):
    """`sequence(pr)` -> dict of arrays on a fresh problem of the scene, on the 1-lane isotropic timetable schedule
    (EGS_QUAD=0 EGS_ISO=2), deferred (defer=None: the default) or eager (defer="0"); fused="0": assemble_kernel, the
    sweep launch and velocity_kernel, three launches."""
    with env(EGS_QUAD="0", EGS_ISO="2", EGS_STEP_DEFER_SYSTEM=defer, EGS_FUSED_ASSEMBLY=fused):
        pr, _ = bench.build_problem(ctx, sc, capi.F64)
        try:
            return sequence(pr)
        finally:
            pr.close()


def both(ctx, sc, sequence):
    """The sequence deferred and eager; everything it returned compared byte for byte.  Returns the deferred run."""
    new, old = run(ctx, sc, sequence, None), run(ctx, sc, sequence, "0")
    assert_same(new, old)
    return new


def assert_same(new, old):
    assert new.keys() == old.keys()
    for k in new:
        a, b = new[k], old[k]
        if isinstance(a, capi.SolveStats):
            assert a.status == capi.OK and b.status == capi.OK, k
            assert a.iterations == b.iterations and a.residual == b.residual, k
            continue
        for i, (x, y) in enumerate(zip(a, b) if isinstance(a, tuple) else [(a, b)]):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), "%s[%d]" % (k, i)


DEFERRED = capi.SCHED_STATIC | capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_DEFERRED_SYSTEM


def check_schedule(schedule):
    assert schedule & capi.SCHED_FUSED_ASSEMBLY, "the fused launch did not run"
    if os.environ.get("EGS_STEP_DEFER_SYSTEM") == "0":
        assert not schedule & capi.SCHED_DEFERRED_SYSTEM
    else:
        assert schedule & DEFERRED == DEFERRED, "silent fall-back: the store-free launch did not run"


def deferred_step(pr, prm, want_stats=False):
    """One step.  Asking for statistics reduces the residual, which reads the bounds and so materialises the system:
    the sequences that test the deferral step without them and end with check_form."""
    st = pr.step(DT, ERP, prm, want_stats=want_stats)
    if want_stats:
        check_schedule(st.schedule)
    return st


def check_form(pr, prm):
    """After a sequence has collected its outputs: one more step of the same kind, whose schedule bits are read
    (egs_problem_get_stats).  The schedule is a function of the problem, the parameters and the switches, which the
    sequence's steps share."""
    pr.step(DT, ERP, prm)
    check_schedule(pr.stats().schedule)


def outputs(pr):
    return dict(lam=pr.lambda_(), v6=pr.velocity(), acc=pr.accumulators(), wres=pr.wres())


def oracle_system(sc, state):
    """The oracle's assembly and rhs of the scene in `state`: J0, J1, is_eq, lo, hi, rhs, err as get_blocks orders them."""
    pos, R, v, w = state
    Minv, f_ext = bench.host_mass_and_force(sc)
    J0, J1, is_eq, lo, hi, err = orc.assemble(pos, R, sc["kind"], sc["body0"], sc["body1"], sc["data"])
    s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
    rhs = orc.ode_rhs(v, w, Minv, f_ext, s.body0, s.body1, J0, J1, err, DT, ERP)
    return J0, J1, is_eq, lo, hi, rhs, err


def assert_blocks_equal_oracle(blocks, ref):
    for name, g, r in zip(("J0", "J1", "is_eq", "lo", "hi", "rhs", "err"), blocks, ref):
        assert np.array_equal(np.asarray(g).reshape(np.asarray(r).shape), r), name


METHODS = ["gs", "sor"]


@pytest.mark.parametrize("method", METHODS)
def test_step_blocks(ctx, method):
    """step, blocks; then step, step, blocks: the second record overwrites the first with no read in between."""
    prm, sc = params(method), small_piles()

    def seq(pr):
        deferred_step(pr, prm)
        out = dict(b1=pr.blocks(), **outputs(pr))
        deferred_step(pr, prm)
        deferred_step(pr, prm)
        out["b2"] = pr.blocks()
        check_form(pr, prm)
        return out
    both(ctx, sc, seq)


@pytest.mark.parametrize("method", METHODS)
def test_step_advance_blocks(ctx, method):
    """step, advance, blocks: the blocks of the state the step started from, also against the oracle's assembly."""
    prm, sc = params(method), small_piles()
    kept = {}

    def seq(pr):
        kept["state"] = pr.state()
        deferred_step(pr, prm)
        pr.advance(DT)
        out = dict(blocks=pr.blocks(), state=pr.state())
        check_form(pr, prm)
        return out
    new = both(ctx, sc, seq)
    assert_blocks_equal_oracle(new["blocks"], oracle_system(sc, kept["state"]))
    assert not np.array_equal(new["state"][0], kept["state"][0])   # the advance did move the bodies


@pytest.mark.parametrize("method", METHODS)
def test_step_advance_advance_blocks(ctx, method):
    """Only one old state set is kept: the second advance materialises the system first."""
    prm, sc = params(method), small_piles()
    kept = {}

    def seq(pr):
        kept["state"] = pr.state()
        deferred_step(pr, prm)
        pr.advance(DT)
        pr.advance(DT)
        out = dict(blocks=pr.blocks(), state=pr.state())
        check_form(pr, prm)
        return out
    new = both(ctx, sc, seq)
    assert_blocks_equal_oracle(new["blocks"], oracle_system(sc, kept["state"]))


@pytest.mark.parametrize("method", METHODS)
def test_inputs_change_while_deferred(ctx, method):
    """step, set_state(other), blocks: the blocks are the step's; step, set_constraints(other), step: the new ones."""
    prm, sc = params(method), small_piles()
    other = scenes.concat([scenes.box_stack(2, 2, 3, jitter=1e-3, seed=k + 7, origin=(0.0, 100.0 * k)) for k in range(3)])
    deeper = sc["data"].copy()
    deeper[:, 6] *= 1.5

    def seq(pr):
        deferred_step(pr, prm)
        pr.set_state(other["p"], other["R"], other["v"] + 0.01, other["w"])
        out = dict(b_state=pr.blocks())
        deferred_step(pr, prm)
        pr.set_constraints(sc["kind"], deeper)
        out["b_cons"] = pr.blocks()
        deferred_step(pr, prm)
        out.update(outputs(pr))
        out["b_after"] = pr.blocks()
        check_form(pr, prm)
        return out
    new = both(ctx, sc, seq)
    assert not np.array_equal(new["b_cons"][5], new["b_after"][5])   # the rhs follows the new penetration depths


@pytest.mark.parametrize("method", METHODS)
def test_readers_of_the_system(ctx, method):
    """step, matvec; step, solve (a fresh fixed-count solve on the materialised system); a tol > 0 step right after a
    deferred one (not fused: results unchanged)."""
    prm, sc = params(method), small_piles()
    prm_tol = params(method, sweeps=60, tol=1e-7)

    def seq(pr):
        deferred_step(pr, prm)
        out = dict(mv=pr.matvec(None, capi.MV_FULL, 0.01, 1.0))
        deferred_step(pr, prm)
        out["st_solve"] = pr.solve(params(method, sweeps=7))
        out["lam_solve"] = pr.lambda_()
        deferred_step(pr, prm)
        st = pr.step(DT, ERP, prm_tol, want_stats=True)
        assert not st.schedule & capi.SCHED_FUSED_ASSEMBLY
        out["st_tol"] = st
        out.update(outputs(pr))
        out["b_tol"] = pr.blocks()
        check_form(pr, prm)
        return out
    both(ctx, sc, seq)


@pytest.mark.parametrize("method", METHODS)
def test_free_body(ctx, method):
    """One body without a constraint (no lane, no slot): the deferred form still runs, and the velocity launch gives the
    free body its v + dt W f."""
    prm, sc = params(method), small_piles(free=True)

    def seq(pr):
        deferred_step(pr, prm)
        out = outputs(pr)
        pr.advance(DT)
        deferred_step(pr, prm)
        out["v6_second"] = pr.velocity()
        out["blocks"] = pr.blocks()
        check_form(pr, prm)
        return out
    new = both(ctx, sc, seq)
    Minv, f_ext = bench.host_mass_and_force(sc)
    b = sc["p"].shape[0] - 1
    want = np.concatenate([sc["v"][b], sc["w"][b]]) + DT * (Minv[b].reshape(6, 6) @ f_ext[b])
    assert np.abs(new["v6"][b] - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()


@pytest.mark.parametrize("method", METHODS)
def test_step_advance_rounds(ctx, method):
    """Three step + advance rounds with statistics: lambda, v6, the accumulators, w and the stats."""
    prm, sc = params(method), small_piles()

    def seq(pr):
        out = {}
        for k in range(3):
            out["st%d" % k] = deferred_step(pr, prm, want_stats=True)
            for name, a in outputs(pr).items():
                out["%s%d" % (name, k)] = a
            pr.advance(DT)
        out["state"] = pr.state()
        return out
    both(ctx, sc, seq)


@pytest.mark.parametrize("method", METHODS)
def test_hot_loop_without_reads(ctx, method):
    """The loop the deferral is for: step, advance, step, .. with nothing read in between, so every advance writes the
    second state set and swaps, and every step overwrites the record.  The last step's schedule is asserted directly
    (its statistics materialise the system only then), and its outputs are also those of the three-launch path
    (assemble_kernel, sweep, velocity_kernel)."""
    prm, sc = params(method), small_piles()

    def seq(pr):
        for _ in range(3):
            pr.step(DT, ERP, prm)
            pr.advance(DT)
        start = pr.state()
        pr.step(DT, ERP, prm)
        st = pr.stats()
        if os.environ.get("EGS_FUSED_ASSEMBLY") != "0":
            check_schedule(st.schedule)
        out = dict(st=st, start=start, blocks=pr.blocks(), **outputs(pr))
        pr.advance(DT)
        out["end"] = pr.state()
        return out
    new = both(ctx, sc, seq)
    assert_same(new, run(ctx, sc, seq, None, fused="0"))
    assert_blocks_equal_oracle(new["blocks"], oracle_system(sc, new["start"]))
