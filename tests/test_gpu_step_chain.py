"""GPU (-m gpu): the CHAIN form of the lane-pair launch (EGS_STEP_CHAIN; step_pair.hip).  In the
steady part of the timetable a thread pair keeps its two bodies' accumulators in registers from the first of its two
updates to the second: the same doubles travel by register instead of through LDS, so lambda, w, the accumulators and
the velocities of a step must keep every bit of

  * the same step with EGS_STEP_CHAIN=0 in the same process (the pair form with its LDS round trip),
  * the same step with EGS_STEP_PAIR=0 (one lane per constraint),
  * the sequential CPU oracle (the velocity update as the other step tests compare it: its sums are ordered otherwise),

on the chained scenes of step_chain_cases.py: the smallest pile that takes the form (no lane with a body on side 0, two
idle wavefronts), the same with twelve pairs that hold an A and no B (forward they load and store in the first step of
an iteration, backward in the second), piles over two tiles of different depth and period, a tile of period 8 with
bodies on side 0; at 1, 2, 9 and 10 sweeps, GS and backward SOR, the store-free launch and the storing one
(EGS_STEP_DEFER_SYSTEM=0, whose blocks are read back), and with EGS_STEP_STEADY=0.  Pairable lists whose plan is not
chained must not report the form and must keep their bits whatever the switch says.  EGS_SCHED_CHAIN is read from
egs_problem_get_schedule: egs_solve_stats.schedule keeps the bits of the pair launch, with the form on or off.

The window: the form walks the steady window [t_s, t_e) two steps per iteration from an even step.  Every chained pile
here has an even depth and an even period, so the forward window starts even and has an even length at every sweep
count, and the backward window starts at 2 depth - 1, odd, and has an odd length: there the fill takes one more step.
Both window parities and the odd entry occur (test_plan_chained.py asserts it without a GPU); after the entry is trimmed
the rest is even in all of them -- an odd rest, which leaves one more step to the drain, needs a tile of odd depth, and
no sweep count gives one on these piles."""
import numpy as np
import pytest

import bench
import step_chain_cases as scc
from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, CFM = 5e-3, 0.2, 0.01
# every switch that puts these small scenes on the 1-lane isotropic timetable kernel
BASE_ENV = {"EGS_QUAD": "0", "EGS_ISO": "2", "EGS_STEP": "1"}
FUSED = capi.SCHED_STATIC | capi.SCHED_ISO | capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY


def params(method, sweeps):
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    return capi.params(method=meth, max_iters=sweeps, tol=0.0, cfm=CFM, omega=omega)


def step(ctx, monkeypatch, sc, method, sweeps, form, store, steady=True):
    """One egs_problem_step under the switches; every output, the blocks of a storing launch, and the schedule bits
    of egs_problem_get_schedule (checked to be those of the statistics plus, at most, EGS_SCHED_CHAIN).  form: "chain"
    (the default launch), "pair" (EGS_STEP_CHAIN=0) or "lane" (EGS_STEP_PAIR=0)."""
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    for k in ("EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY"):
        monkeypatch.delenv(k, raising=False)
    for k, off in (("EGS_STEP_CHAIN", form == "pair"), ("EGS_STEP_PAIR", form == "lane"), ("EGS_STEP_DEFER_SYSTEM", store),
                   ("EGS_STEP_STEADY", not steady)):
        if off:
            monkeypatch.setenv(k, "0")
        else:
            monkeypatch.delenv(k, raising=False)
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    try:
        pr.step(DT, ERP, params(method, sweeps))
        st = pr.stats()
        assert st.status == capi.OK
        out = dict(lam=pr.lambda_(), acc=pr.accumulators(), wres=pr.wres(), v6=pr.velocity())
        if store:
            assert not st.schedule & capi.SCHED_DEFERRED_SYSTEM
            for name, a in zip(("J0", "J1", "is_eq", "lo", "hi", "rhs", "err"), pr.blocks()):
                out[name] = a
        sched = pr.schedule()
        assert sched & ~capi.SCHED_CHAIN == int(st.schedule) and not st.schedule & capi.SCHED_CHAIN
        return out, sched
    finally:
        pr.close()


def assert_same(new, old, what):
    assert new.keys() == old.keys()
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (what, k)


_scenes, _oracle = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = scc.scene(name)
    return _scenes[name]


def oracle(name, method, sweeps):
    """The blocks, lambda, accumulators, w and v6 of one step of the scene from the sequential oracle (once per case)."""
    ident = (name, method, sweeps)
    if ident not in _oracle:
        sc = scene(name)
        meth, omega = (orc.GAUSS_SEIDEL, 1.0) if method == "gs" else (orc.SOR, 1.5)
        Minv, f_ext = bench.host_mass_and_force(sc)
        J0, J1, is_eq, lo, hi, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
        s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
        rhs = orc.ode_rhs(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, err, DT, ERP)
        xf, af, _, _ = orc.fast_iterate(s, rhs, CFM, meth, max_iters=sweeps, tol=0.0, omega=omega)
        v6 = orc.velocity_update(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, xf, DT)
        _oracle[ident] = dict(lam=xf, acc=af, wres=orc.fast_wres(s, rhs, CFM, xf, af), v6=v6, J0=J0, J1=J1, rhs=rhs)
    return _oracle[ident]


def assert_oracle(got, ref, what):
    for name in ("lam", "acc", "wres"):
        assert np.array_equal(got[name].reshape(ref[name].shape), ref[name]), (what, name)
    assert np.abs(got["v6"] - ref["v6"]).max() <= 1e-12 * max(1.0, np.abs(ref["v6"]).max()), what
    for name in ("J0", "J1", "rhs"):
        if name in got:
            assert np.array_equal(got[name].reshape(ref[name].shape), ref[name]), (what, name)


@pytest.mark.parametrize("method", ["gs", "sor"])
@pytest.mark.parametrize("name", scc.CHAINED)
def test_chain_keeps_every_bit(ctx, monkeypatch, name, method):
    sc = scene(name)
    for sweeps in scc.SWEEPS:
        for store in (False, True):
            what = (name, method, sweeps, "storing" if store else "store-free")
            on, s_on = step(ctx, monkeypatch, sc, method, sweeps, "chain", store)
            pair, s_pair = step(ctx, monkeypatch, sc, method, sweeps, "pair", store)
            lane, s_lane = step(ctx, monkeypatch, sc, method, sweeps, "lane", store)
            assert s_on & FUSED == FUSED and s_on & capi.SCHED_PAIR and s_on & capi.SCHED_CHAIN, what
            assert s_pair == s_on & ~capi.SCHED_CHAIN, what
            assert s_lane == s_on & ~(capi.SCHED_CHAIN | capi.SCHED_PAIR), what
            assert bool(s_on & capi.SCHED_DEFERRED_SYSTEM) == (not store), what
            assert_same(on, pair, what)
            assert_same(on, lane, what)
            assert_oracle(on, oracle(name, method, sweeps), what)


@pytest.mark.parametrize("method", ["gs", "sor"])
@pytest.mark.parametrize("name", scc.PAIRABLE_NOT_CHAINED)
def test_other_pairable_lists_keep_their_launch(ctx, monkeypatch, name, method):
    sc = scene(name)
    for sweeps in (2, 9):
        what = (name, method, sweeps)
        on, s_on = step(ctx, monkeypatch, sc, method, sweeps, "chain", False)
        off, s_off = step(ctx, monkeypatch, sc, method, sweeps, "pair", False)
        assert s_on & FUSED == FUSED and s_on & capi.SCHED_PAIR, what
        assert not s_on & capi.SCHED_CHAIN and s_on == s_off, what
        assert_same(on, off, what)
        assert_oracle(on, oracle(name, method, sweeps), what)


@pytest.mark.parametrize("name", ["two", "g32p"])
def test_the_steady_loop_switch_takes_the_form_away(ctx, monkeypatch, name):
    """EGS_STEP_STEADY=0: the form is the steady loop's, so the pair launch's general loop alone walks the timetable."""
    sc = scene(name)
    for method in ("gs", "sor"):
        on, s_on = step(ctx, monkeypatch, sc, method, 9, "chain", False)
        single, s_single = step(ctx, monkeypatch, sc, method, 9, "chain", False, steady=False)
        assert s_on & capi.SCHED_CHAIN and s_single == s_on & ~capi.SCHED_CHAIN, (name, method)
        assert_same(on, single, (name, method))
