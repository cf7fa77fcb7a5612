"""GPU (-m gpu): the SHARE form of the CHAIN launch (EGS_STEP_SHARE; step_pair.hip).  Where the two
contacts of every thread pair carry one normal, a thread keeps the linear Jacobian block, the weights and the linear
products of its side once for both constraints: the same doubles in fewer registers, the same multiplies, so lambda, w,
the accumulators and the velocities of a step must keep every bit of

  * the same step with EGS_STEP_SHARE=0 in the same process (the CHAIN form with both copies),
  * the same step with EGS_STEP_PAIR=0 (one lane per constraint),
  * the sequential CPU oracle (the velocity update as the other step tests compare it: its sums are ordered otherwise),

on the smallest chained scenes of test_gpu_step_chain.py (step_share_cases.py: the 32-box pile, the same with twelve
pairs that hold an A and no B, 8 x 4 x 2, two tiles of depth 16 and 64), at 1, 2, 9 and 10 sweeps, GS and backward SOR,
the store-free launch and the storing one (EGS_STEP_DEFER_SYSTEM=0, whose blocks are read back), with EGS_STEP_STEADY=0,
and with restitution (an instantiation of its own).  A pile whose contacts all carry one tilted normal runs the form on
a linear block without a zero entry.  A pile in which one pair's normals differ only in the sign of a zero,
or by a tilt, must not report the form and must still match the references; an A without a B may carry any normal.
egs_problem_set_constraints decides again: the form follows the normals from one step to the next.

EGS_SCHED_SHARE is read from egs_problem_get_schedule_full: egs_problem_get_schedule and egs_solve_stats.schedule keep
the bits they had, with the form on or off."""
import numpy as np
import pytest

import bench
import restitution_reference as rr
import step_share_cases as ssc
from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, CFM = 5e-3, 0.2, 0.01
# every switch that puts these small scenes on the 1-lane isotropic timetable kernel
BASE_ENV = {"EGS_QUAD": "0", "EGS_ISO": "2", "EGS_STEP": "1"}
FUSED = capi.SCHED_STATIC | capi.SCHED_ISO | capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_PAIR
SWEEPS = (1, 2, 9, 10)


def params(method, sweeps):
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    return capi.params(method=meth, max_iters=sweeps, tol=0.0, cfm=CFM, omega=omega)


def set_env(monkeypatch, form, store, steady=True):
    """form: "share" (the default launch), "chain" (EGS_STEP_SHARE=0) or "lane" (EGS_STEP_PAIR=0)."""
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    for k in ("EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY", "EGS_STEP_CHAIN", "EGS_TILE", "EGS_LANE_ORDER"):
        monkeypatch.delenv(k, raising=False)
    for k, off in (("EGS_STEP_SHARE", form == "chain"), ("EGS_STEP_PAIR", form == "lane"), ("EGS_STEP_DEFER_SYSTEM", store),
                   ("EGS_STEP_STEADY", not steady)):
        if off:
            monkeypatch.setenv(k, "0")
        else:
            monkeypatch.delenv(k, raising=False)


def outputs(pr, store):
    """Every output of the step pr has just run, the blocks of a storing launch, and the schedule bits of
    egs_problem_get_schedule_full (checked: egs_problem_get_schedule is those without EGS_SCHED_SHARE, the statistics
    those without EGS_SCHED_CHAIN as well)."""
    st = pr.stats()
    assert st.status == capi.OK
    out = dict(lam=pr.lambda_(), acc=pr.accumulators(), wres=pr.wres(), v6=pr.velocity())
    if store:
        assert not st.schedule & capi.SCHED_DEFERRED_SYSTEM
        for name, a in zip(("J0", "J1", "is_eq", "lo", "hi", "rhs", "err"), pr.blocks()):
            out[name] = a
    full = pr.schedule_full()
    assert pr.schedule() == full & ~capi.SCHED_SHARE
    assert int(st.schedule) == full & ~(capi.SCHED_SHARE | capi.SCHED_CHAIN)
    return out, full


def step(ctx, monkeypatch, sc, method, sweeps, form, store, steady=True, rest=None):
    set_env(monkeypatch, form, store, steady)
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    try:
        if rest is not None:
            pr.set_restitution(*rest)
        pr.step(DT, ERP, params(method, sweeps))
        return outputs(pr, store)
    finally:
        pr.close()


def assert_same(new, old, what):
    assert new.keys() == old.keys()
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (what, k)


_scenes, _oracle = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = ssc.scene(name)
    return _scenes[name]


def oracle(name, method, sweeps, rest=None):
    """The blocks, lambda, accumulators, w and v6 of one step of the scene from the sequential oracle (once per case);
    rest = (coefficients, threshold): the rhs is the restitution twin's (restitution_reference.py)."""
    ident = (name, method, sweeps, rest is not None)
    if ident not in _oracle:
        sc = scene(name)
        meth, omega = (orc.GAUSS_SEIDEL, 1.0) if method == "gs" else (orc.SOR, 1.5)
        Minv, f_ext = bench.host_mass_and_force(sc)
        J0, J1, is_eq, lo, hi, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
        s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
        if rest is None:
            rhs = orc.ode_rhs(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, err, DT, ERP)
        else:
            rhs, what, _ = rr.twin_rhs(dict(sc, Minv=Minv, f_ext=f_ext, dt=DT, erp=ERP), J0, J1, err, rest[0], rest[1])
            assert "bounce" in what
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


def check_forms(ctx, monkeypatch, name, method, sweeps, store, shares, rest=None):
    """The default launch against EGS_STEP_SHARE=0, EGS_STEP_PAIR=0 and the oracle; shares: must it report the form?"""
    sc = scene(name)
    what = (name, method, sweeps, "storing" if store else "store-free")
    on, s_on = step(ctx, monkeypatch, sc, method, sweeps, "share", store, rest=rest)
    chain, s_chain = step(ctx, monkeypatch, sc, method, sweeps, "chain", store, rest=rest)
    lane, s_lane = step(ctx, monkeypatch, sc, method, sweeps, "lane", store, rest=rest)
    assert s_on & FUSED == FUSED and s_on & capi.SCHED_CHAIN, what
    assert bool(s_on & capi.SCHED_SHARE) == shares, what
    assert s_chain == s_on & ~capi.SCHED_SHARE, what
    assert s_lane == s_on & ~(capi.SCHED_SHARE | capi.SCHED_CHAIN | capi.SCHED_PAIR), what
    assert bool(s_on & capi.SCHED_DEFERRED_SYSTEM) == (not store), what
    assert_same(on, chain, what)
    assert_same(on, lane, what)
    assert_oracle(on, oracle(name, method, sweeps, rest), what)
    return on


@pytest.mark.parametrize("method", ["gs", "sor"])
@pytest.mark.parametrize("name", ssc.SCENES + ("h2:tilt", "g32p:tilt", "g32p:alone"))
def test_share_keeps_every_bit(ctx, monkeypatch, name, method):
    for sweeps in SWEEPS:
        for store in (False, True):
            check_forms(ctx, monkeypatch, name, method, sweeps, store, shares=True)


def test_the_tilted_block_has_no_zero_entry(ctx, monkeypatch):
    """What the tilted pile is for: Rn, the same in every contact, without a zero, and with eight distinct values among
    its nine entries (the rotation that takes the normal to z turns about an axis in the xy plane, so Rn[0][1] =
    Rn[1][0]; every other entry differs from the rest)."""
    out, sched = step(ctx, monkeypatch, scene("h2:tilt"), "gs", 2, "share", True)
    assert sched & capi.SCHED_SHARE
    lin = out["J1"].reshape(-1, 3, 6)[:, :, :3].reshape(-1, 9)
    assert (lin == lin[0]).all() and (lin[0] != 0).all() and np.unique(lin[0]).shape == (8,)


@pytest.mark.parametrize("method", ["gs", "sor"])
@pytest.mark.parametrize("name", ["g32:zero", "h2:zero", "two:tiltB"])
def test_two_normals_in_a_pair_keep_the_chain_form(ctx, monkeypatch, name, method):
    for sweeps in (2, 9):
        for store in (False, True):
            check_forms(ctx, monkeypatch, name, method, sweeps, store, shares=False)


@pytest.mark.parametrize("name", ["two", "g32p"])
def test_the_steady_loop_switch_takes_the_form_away(ctx, monkeypatch, name):
    """EGS_STEP_STEADY=0: no CHAIN form, so no SHARE form either; the general loop alone walks the timetable."""
    sc = scene(name)
    for method in ("gs", "sor"):
        on, s_on = step(ctx, monkeypatch, sc, method, 9, "share", False)
        single, s_single = step(ctx, monkeypatch, sc, method, 9, "share", False, steady=False)
        assert s_on & capi.SCHED_SHARE and s_single == s_on & ~(capi.SCHED_SHARE | capi.SCHED_CHAIN), (name, method)
        assert_same(on, single, (name, method))
        assert_oracle(on, oracle(name, method, 9), (name, method))


@pytest.mark.parametrize("store", [False, True], ids=["deferred", "storing"])
@pytest.mark.parametrize("method", ["gs", "sor"])
def test_share_with_restitution(ctx, monkeypatch, method, store):
    """The REST instantiations: every body of the 8 x 4 x 2 pile approaches the one below it."""
    name = "h2:falling"
    if name not in _scenes:
        sc = dict(ssc.scene("h2"))
        sc["v"] = sc["v"].copy()
        sc["v"][:, 2] -= np.random.default_rng(11).uniform(0.05, 2.0, sc["v"].shape[0])
        _scenes[name] = sc
    m = scene(name)["body0"].shape[0]
    rest = (np.array([rr.COEFFICIENTS[i % 5] for i in range(m)]), 0.5)
    for sweeps in (2, 9):
        on = check_forms(ctx, monkeypatch, name, method, sweeps, store, shares=True, rest=rest)
        off, _ = step(ctx, monkeypatch, scene(name), method, sweeps, "share", store)
        assert on["lam"].tobytes() != off["lam"].tobytes()


@pytest.mark.parametrize("method", ["gs", "sor"])
def test_set_constraints_decides_again(ctx, monkeypatch, method):
    """One problem, three steps from the same state: one normal per face, then a pair whose normals differ in the sign of
    a zero, then one normal per face again.  The form is on, off, on, and every step is the fresh problem's."""
    plain, zero = scene("h2"), scene("h2:zero")
    set_env(monkeypatch, "share", False)
    pr, _ = bench.build_problem(ctx, plain, capi.F64)
    try:
        for sc, name, shares in ((plain, "h2", True), (zero, "h2:zero", False), (plain, "h2", True)):
            pr.set_constraints(sc["kind"], sc["data"])
            pr.step(DT, ERP, params(method, 9))
            got, sched = outputs(pr, False)
            assert bool(sched & capi.SCHED_SHARE) == shares and sched & capi.SCHED_CHAIN, (name, method)
            fresh, s_fresh = step(ctx, monkeypatch, sc, method, 9, "share", False)
            assert s_fresh == sched
            assert_same(got, fresh, (name, method))
            assert_oracle(got, oracle(name, method, 9), (name, method))
    finally:
        pr.close()
