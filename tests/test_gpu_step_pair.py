"""GPU (-m gpu): the PAIR form of the fused step launch (one update on a lane pair, EGS_STEP_PAIR; step_pair.hip).  It changes
which thread forms which product and no rounding, so lambda, w, the accumulators and the velocities of a step must keep
every bit of

  * the same step with EGS_STEP_PAIR=0 in the same process (one lane per constraint),
  * the sequential CPU oracle (the velocity update as the other step tests compare it: its sums are ordered otherwise),

on the scenes of step_pair_cases.py: the smallest pile that takes the form (ground contacts only: no lane with a body
on side 0, two idle wavefronts), a tile whose last pairs hold an A and no B, piles over two tiles of different depth
and period; at 1, 2 and 9 sweeps (an empty, a short and a long steady window), GS and backward SOR, the store-free
launch and the storing one (EGS_STEP_DEFER_SYSTEM=0, whose blocks are read back).  Lists whose plan is not pairable
must not report the form and must keep their bits whatever the switch says."""
import numpy as np
import pytest

import bench
import step_pair_cases as spc
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


def step(ctx, monkeypatch, sc, method, sweeps, pair, store):
    """One egs_problem_step under the switches; every output, and the blocks of a storing launch."""
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    for k in ("EGS_STEP_STEADY", "EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY"):
        monkeypatch.delenv(k, raising=False)
    if pair:
        monkeypatch.delenv("EGS_STEP_PAIR", raising=False)
    else:
        monkeypatch.setenv("EGS_STEP_PAIR", "0")
    if store:
        monkeypatch.setenv("EGS_STEP_DEFER_SYSTEM", "0")
    else:
        monkeypatch.delenv("EGS_STEP_DEFER_SYSTEM", raising=False)
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
        return out, int(st.schedule)
    finally:
        pr.close()


def assert_same(new, old, what):
    assert new.keys() == old.keys()
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (what, k)


_scenes, _oracle = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = spc.scene(name)
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
@pytest.mark.parametrize("name", spc.PAIRABLE)
def test_pair_keeps_every_bit(ctx, monkeypatch, name, method):
    sc = scene(name)
    for sweeps in spc.SWEEPS:
        for store in (False, True):
            what = (name, method, sweeps, "storing" if store else "store-free")
            on, s_on = step(ctx, monkeypatch, sc, method, sweeps, True, store)
            off, s_off = step(ctx, monkeypatch, sc, method, sweeps, False, store)
            assert s_on & FUSED == FUSED and s_on & capi.SCHED_PAIR, what
            assert s_off == s_on & ~capi.SCHED_PAIR, what
            assert bool(s_on & capi.SCHED_DEFERRED_SYSTEM) == (not store), what
            assert_same(on, off, what)
            assert_oracle(on, oracle(name, method, sweeps), what)


@pytest.mark.parametrize("method", ["gs", "sor"])
@pytest.mark.parametrize("name", spc.NOT_PAIRABLE)
def test_other_lists_keep_their_launch(ctx, monkeypatch, name, method):
    sc = scene(name)
    for sweeps in (2, 9):
        what = (name, method, sweeps)
        on, s_on = step(ctx, monkeypatch, sc, method, sweeps, True, False)
        off, s_off = step(ctx, monkeypatch, sc, method, sweeps, False, False)
        assert not s_on & capi.SCHED_PAIR and s_on == s_off, what
        assert bool(s_on & capi.SCHED_FUSED_ASSEMBLY) == (name != "chain"), what
        assert_same(on, off, what)
        assert_oracle(on, oracle(name, method, sweeps), what)


def test_the_steady_loop_switch_changes_nothing(ctx, monkeypatch):
    """EGS_STEP_STEADY=0: the form's general loop alone walks the whole timetable."""
    sc = scene("two")
    for method in ("gs", "sor"):
        on, s_on = step(ctx, monkeypatch, sc, method, 9, True, False)
        monkeypatch.setenv("EGS_STEP_STEADY", "0")
        pr, _ = bench.build_problem(ctx, sc, capi.F64)
        try:
            pr.step(DT, ERP, params(method, 9))
            st = pr.stats()
            single = dict(lam=pr.lambda_(), acc=pr.accumulators(), wres=pr.wres(), v6=pr.velocity())
        finally:
            pr.close()
        monkeypatch.delenv("EGS_STEP_STEADY")
        assert st.status == capi.OK and st.schedule == s_on
        assert_same(on, single, method)
