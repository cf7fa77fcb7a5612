"""GPU (-m gpu): the FACE launch writes the step's velocities in its epilogue (EGS_STEP_FACE_VELOCITY; step_face.hip),
and egs_problem_step then runs no velocity_kernel.  The expression is velocity_kernel's, v + dt (W f + a), on the
accumulator the epilogue has just stored, so velocity(), lambda, w and the accumulators of a step must keep every bit of

  * the same step with EGS_STEP_FACE_VELOCITY=0 (the launch followed by velocity_kernel: the step as it was),
  * the sequential CPU oracle (as test_gpu_step_face.py compares it).

Every input that enters the expression is non-trivial here: random v and w, a random force and torque on every body, an
inertia of its own per body (isotropic, and one mass: what the FACE form asks), dt = 3.7e-3, erp = 0.35.  The scenes are
the small faced piles of step_face_cases.py and three 8 x 4 x 2 piles side by side, at 1, 2, 9 and 10 sweeps; unsplit,
and split by force at s1 = 1, the middle and S - 1 on all tiles and on one of three (a first part must leave the
velocities to its second part); five steps in a row on one problem with advance and set_state between them.

A body in no constraint is in no tile, and still moves by dt W f: such a problem keeps velocity_kernel.  A step whose
launch is not the FACE form (two contact points per face, backward SOR, restitution) is what it was."""
import numpy as np
import pytest

import restitution_reference as rr
import test_gpu_step_face as tsf
import test_gpu_step_face_split as tsp
import test_gpu_step_share as tss
from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, CFM = 3.7e-3, 0.35, tss.CFM
SCENES = ("g32", "g32p", "two", "mixed", "h2", "h2x3")
SWEEPS = (1, 2, 9, 10)

_inputs, _oracle = {}, {}


def inputs(name, extra=None):
    """The scene with random v, w, force and torque and an inertia per body; extra: None, or where one more body that no
    constraint touches goes ("last": behind the others, "first": before them, every body number moving up by one)."""
    key = (name, extra)
    if key not in _inputs:
        sc = dict(tsp.scene(name))
        rng = np.random.default_rng(len(name) + 17)
        if extra:
            at = 0 if extra == "first" else sc["p"].shape[0]
            for k, row in (("p", [50.0, -50.0, 7.0]), ("R", np.eye(3).reshape(9)), ("v", np.zeros(3)), ("w", np.zeros(3)),
                           ("mass", sc["mass"][0]), ("I_body", sc["I_body"][0])):
                sc[k] = np.insert(sc[k], at, row, axis=0)
            if extra == "first":
                sc["body0"] = np.where(sc["body0"] >= 0, sc["body0"] + 1, -1).astype(np.int32)
                sc["body1"] = np.where(sc["body1"] >= 0, sc["body1"] + 1, -1).astype(np.int32)
        n = sc["p"].shape[0]
        sc["v"] = rng.uniform(-0.5, 0.5, (n, 3))
        sc["w"] = rng.uniform(-0.5, 0.5, (n, 3))
        assert np.all(sc["mass"] == sc["mass"][0])
        Minv = np.zeros((n, 6, 6))
        inv_inertia = rng.uniform(4.0, 16.0, n)
        for k in range(3):
            Minv[:, k, k] = 1.0 / sc["mass"]
            Minv[:, 3 + k, 3 + k] = inv_inertia
        f_ext = rng.uniform(-3.0, 3.0, (n, 6))
        f_ext[:, 2] -= 9.8 * sc["mass"]
        assert np.all(sc["v"] != 0) and np.all(sc["w"] != 0) and np.all(f_ext != 0)
        _inputs[key] = (sc, Minv.reshape(n, 36), f_ext)
    return _inputs[key]


def problem(ctx, name, extra=None):
    sc, Minv, f_ext = inputs(name, extra)
    pr = capi.Problem(ctx, sc["p"].shape[0], sc["body0"], sc["body1"], capi.F64)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
    pr.set_constraints(sc["kind"], sc["data"])
    return pr


def params(sweeps, method="gs"):
    return tss.params(method, sweeps)


def set_env(monkeypatch, velocity, split=0, form="face"):
    """velocity: the epilogue writes (True: the default) or EGS_STEP_FACE_VELOCITY=0; split as test_gpu_step_face_split"""
    tsp.set_env(monkeypatch, split, form=form)
    if velocity:
        monkeypatch.delenv("EGS_STEP_FACE_VELOCITY", raising=False)
    else:
        monkeypatch.setenv("EGS_STEP_FACE_VELOCITY", "0")


def outputs(pr):
    out, full = tss.outputs(pr, False)
    return out, pr.schedule_forms()


def step(ctx, monkeypatch, name, sweeps, velocity, split=0, extra=None, method="gs", rest=None, form="face"):
    set_env(monkeypatch, velocity, split, form)
    pr = problem(ctx, name, extra)
    try:
        if rest is not None:
            pr.set_restitution(*rest)
        pr.step(DT, ERP, params(sweeps, method))
        return outputs(pr)
    finally:
        pr.close()


def oracle(name, sweeps, extra=None):
    key = (name, sweeps, extra)
    if key not in _oracle:
        sc, Minv, f_ext = inputs(name, extra)
        J0, J1, is_eq, lo, hi, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
        s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
        rhs = orc.ode_rhs(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, err, DT, ERP)
        xf, af, _, _ = orc.fast_iterate(s, rhs, CFM, orc.GAUSS_SEIDEL, max_iters=sweeps, tol=0.0, omega=1.0)
        v6 = orc.velocity_update(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, xf, DT)
        _oracle[key] = dict(lam=xf, acc=af, wres=orc.fast_wres(s, rhs, CFM, xf, af), v6=v6)
    return _oracle[key]


_kernel = {}


def with_velocity_kernel(ctx, monkeypatch, name, sweeps):
    """The unsplit step with EGS_STEP_FACE_VELOCITY=0, once per case, checked against the oracle."""
    if (name, sweeps) not in _kernel:
        got, forms = step(ctx, monkeypatch, name, sweeps, False)
        assert forms & capi.SCHED_FACE and not forms & capi.SCHED_FACE_SPLIT, (name, sweeps)
        tss.assert_oracle(got, oracle(name, sweeps), (name, sweeps))
        _kernel[(name, sweeps)] = (got, forms)
    return _kernel[(name, sweeps)]


@pytest.mark.parametrize("name", SCENES)
def test_the_epilogue_writes_velocity_kernels_bits(ctx, monkeypatch, name):
    for sweeps in SWEEPS:
        ref, f_ref = with_velocity_kernel(ctx, monkeypatch, name, sweeps)
        got, forms = step(ctx, monkeypatch, name, sweeps, True)
        assert forms == f_ref, (name, sweeps)
        tss.assert_same(got, ref, (name, sweeps))
        tss.assert_oracle(got, oracle(name, sweeps), (name, sweeps))
        assert np.all(got["v6"] != 0), (name, sweeps)     # every body was written


@pytest.mark.parametrize("name", SCENES)
def test_split_tiles_leave_the_velocity_to_the_second_part(ctx, monkeypatch, name):
    """All tiles split, and one of three: at s1 = 1, the middle and S - 1.  A first part that wrote a velocity which its
    second part then failed to overwrite would leave that of s1 sweeps."""
    tiles = tsp.n_tiles(name)
    for sweeps in (2, 9, 10):
        ref, f_ref = with_velocity_kernel(ctx, monkeypatch, name, sweeps)
        for h in sorted({tiles, 1}):
            for s1 in tsp.cuts(sweeps):
                what = (name, sweeps, h, s1)
                got, forms = step(ctx, monkeypatch, name, sweeps, True, split=(h, s1))
                assert forms == f_ref | capi.SCHED_FACE_SPLIT, what
                tss.assert_same(got, ref, what)
                off, f_off = step(ctx, monkeypatch, name, sweeps, False, split=(h, s1))
                assert f_off == forms, what
                tss.assert_same(off, ref, what)


def test_one_of_three_tiles_is_a_strict_subset():
    assert tsp.n_tiles("h2x3") == 3


def run_steps(ctx, monkeypatch, name, velocity, split, n_steps=5, sweeps=9):
    set_env(monkeypatch, velocity, split)
    sc, Minv, f_ext = inputs(name)
    pr, outs = problem(ctx, name), []
    try:
        for k in range(n_steps):
            pr.step(DT, ERP, params(sweeps))
            outs.append(outputs(pr))
            if k % 2 == 0:
                pr.advance(DT)      # the next step reads the velocities this one wrote
            else:
                pr.set_state(sc["p"], sc["R"], sc["w"], sc["v"], Minv, f_ext)     # v and w change places
        return outs
    finally:
        pr.close()


@pytest.mark.parametrize("split", [0, (3, 4), (1, 8)], ids=["unsplit", "all-split", "one-split"])
def test_five_steps_in_a_row(ctx, monkeypatch, split):
    ref = run_steps(ctx, monkeypatch, "h2x3", False, 0)
    got = run_steps(ctx, monkeypatch, "h2x3", True, split)
    assert len(got) == len(ref) == 5
    for k, ((g, fg), (r, fr)) in enumerate(zip(got, ref)):
        assert fg & ~capi.SCHED_FACE_SPLIT == fr and fr & capi.SCHED_FACE, (split, k)
        tss.assert_same(g, r, (split, k))
    assert ref[1][0]["v6"].tobytes() != ref[0][0]["v6"].tobytes()      # the steps differ: advance moved the state
    tss.assert_same(ref[0][0], with_velocity_kernel(ctx, monkeypatch, "h2x3", 9)[0], "first step")


@pytest.mark.parametrize("extra", ["last", "first"])
@pytest.mark.parametrize("name", ["h2", "h2x3"])
def test_a_body_in_no_tile_keeps_velocity_kernel(ctx, monkeypatch, name, extra):
    """One body that no constraint touches: it is a slot of no tile, so no epilogue writes it, and it moves by dt W f."""
    sc, Minv, f_ext = inputs(name, extra)
    free = 0 if extra == "first" else sc["p"].shape[0] - 1
    assert not np.any(sc["body0"] == free) and not np.any(sc["body1"] == free)
    W = Minv.reshape(-1, 6, 6)[free]
    moved = np.concatenate([sc["v"][free], sc["w"][free]]) + DT * (W @ f_ext[free])
    for sweeps in (2, 9):
        for split in (0, (1, 1)):
            what = (name, extra, sweeps, split)
            got, forms = step(ctx, monkeypatch, name, sweeps, True, split=split, extra=extra)
            off, f_off = step(ctx, monkeypatch, name, sweeps, False, split=split, extra=extra)
            assert forms == f_off and forms & capi.SCHED_FACE, what
            tss.assert_same(got, off, what)
            tss.assert_oracle(got, oracle(name, sweeps, extra), what)
            assert np.abs(got["v6"].reshape(-1, 6)[free] - moved).max() <= 1e-15 * np.abs(moved).max(), what
            assert np.all(got["acc"].reshape(-1, 6)[free] == 0), what


@pytest.mark.parametrize("case", ["h2half", "sor", "restitution"])
def test_a_launch_that_is_not_face_is_unchanged(ctx, monkeypatch, case):
    name, method, rest = ("h2half" if case == "h2half" else "h2"), ("sor" if case == "sor" else "gs"), None
    if case == "restitution":
        rest = (np.array([rr.COEFFICIENTS[i % 5] for i in range(inputs(name)[0]["body0"].shape[0])]), 0.05)
    for sweeps in (2, 9):
        on, f_on = step(ctx, monkeypatch, name, sweeps, True, method=method, rest=rest)
        off, f_off = step(ctx, monkeypatch, name, sweeps, False, method=method, rest=rest)
        assert f_on == f_off and not f_on & capi.SCHED_FACE, (case, sweeps)
        tss.assert_same(on, off, (case, sweeps))
        share, f_share = step(ctx, monkeypatch, name, sweeps, True, method=method, rest=rest, form="share")
        assert f_share == f_on, (case, sweeps)
        tss.assert_same(on, share, (case, sweeps))
        if case == "h2half":
            tss.assert_oracle(on, oracle(name, sweeps), (case, sweeps))
