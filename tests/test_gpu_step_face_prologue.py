"""GPU (-m gpu): the staged prologue of the FACE form (step_face.hip: step_solve_face_kernel).  The kernel loads the
four members' descriptors, then data[7] of both owned constraints with the group's two body numbers, then the two
bodies' state ONCE per lane, and assembles both constraints from those values (assemble_device.h: contact_blocks,
side_u) where it used to run the one-lane assembly twice behind its own loads.  Nothing it computes may move by a bit.

The stock scenes are at rest, which hides u = v/dt + W f and its divisions, and give every body the same weights.  Here
every body gets a random non-zero v and w, a random f_ext on all six components and an inertia of its own (the angular
weights differ across every face); dt and erp are not the benchmark's.  The linear masses stay equal: unequal ones take
the whole fused launch away (its LINSYM precondition), which one case asserts -- the form is then off and the step is
the other kernels'.

On g32, g32p (groups of three, ground contacts), two (a deep tile plus a partly filled one), mixed, h2 and g32:tilt, at
1, 2 and 9 sweeps:
  * lambda, wres, the accumulators and velocity() byte for byte against the same step with EGS_STEP_FACE=0;
  * blocks() read after the step (the deferred assemble_kernel) byte for byte against blocks() after that step;
  * the step against the sequential CPU oracle as test_gpu_step_face.py compares it (lambda, accumulators and w exactly,
    the velocities to 1e-12, the blocks and rhs exactly);
  * the form is reported where expected and is off on h2half;
  * a second step after advance (the state buffer sets swap) and a third after set_state read the current state;
  * a body without contacts beside the tiles gets v + dt W f.
"""
import numpy as np
import pytest

import step_face_cases as sfc
import test_gpu_step_face as tsf
import test_gpu_step_share as tss
from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, CFM = 3.7e-3, 0.35, tss.CFM        # the benchmark and the other step tests run 5e-3 and 0.2
SCENES = ("g32", "g32p", "two", "mixed", "h2", "g32:tilt")
SWEEPS = (1, 2, 9)
BLOCKS = ("J0", "J1", "is_eq", "lo", "hi", "rhs", "err")

_cases, _oracle = {}, {}


def moving(name, unequal_mass=False, free_body=False):
    """step_face_cases.py's scene in motion: (scene, Minv [n][6][6], f_ext [n][6])."""
    key = (name, unequal_mass, free_body)
    if key not in _cases:
        sc = dict(sfc.scene(name))
        rng = np.random.default_rng(sum(map(ord, name)) + 7)
        if free_body:                           # one more body, far from the pile, in no constraint
            far = np.array([[50.0, -30.0, 20.0]])
            sc["p"] = np.concatenate([sc["p"], far])
            sc["R"] = np.concatenate([sc["R"], np.eye(3).reshape(1, 9)])
        n = sc["p"].shape[0]
        sc["v"] = rng.uniform(0.05, 0.8, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
        sc["w"] = rng.uniform(0.05, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
        mass = rng.uniform(0.5, 2.0, n) if unequal_mass else np.full(n, 1.25)
        inertia = rng.uniform(0.05, 0.3, n)     # I = inertia * I3: isotropic, another weight on every body
        Minv = np.zeros((n, 6, 6))
        for k in range(3):
            Minv[:, k, k] = 1.0 / mass
            Minv[:, 3 + k, 3 + k] = 1.0 / inertia
        f_ext = rng.uniform(0.2, 3.0, (n, 6)) * rng.choice([-1.0, 1.0], (n, 6))
        f_ext[:, 2] -= 9.8 * mass
        _cases[key] = (sc, Minv, f_ext)
    return _cases[key]


def build(ctx, case):
    sc, Minv, f_ext = case
    pr = capi.Problem(ctx, sc["p"].shape[0], sc["body0"], sc["body1"], capi.F64)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
    pr.set_constraints(sc["kind"], sc["data"])
    return pr


def read(pr):
    """the step's outputs and forms (test_gpu_step_face.outputs asserts what the other reports say), then the blocks:
    the deferred assemble_kernel runs for them"""
    out, forms = tsf.outputs(pr, False)
    for k, a in zip(BLOCKS, pr.blocks()):
        out[k] = a
    return out, forms


def step(ctx, monkeypatch, case, sweeps, form):
    tsf.set_env(monkeypatch, form)
    pr = build(ctx, case)
    try:
        pr.step(DT, ERP, tss.params("gs", sweeps))
        return read(pr)
    finally:
        pr.close()


def oracle_step(state, case, sweeps):
    """One step of the case from (p, R, v, w) on the sequential oracle: what test_gpu_step_share.oracle computes, at this
    file's dt, erp, weights and forces."""
    sc, Minv, f_ext = case
    p, R, v, w = state
    J0, J1, is_eq, lo, hi, err = orc.assemble(p, R, sc["kind"], sc["body0"], sc["body1"], sc["data"])
    s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
    rhs = orc.ode_rhs(v, w, Minv, f_ext, s.body0, s.body1, J0, J1, err, DT, ERP)
    xf, af, _, _ = orc.fast_iterate(s, rhs, CFM, orc.GAUSS_SEIDEL, max_iters=sweeps, tol=0.0, omega=1.0)
    v6 = orc.velocity_update(v, w, Minv, f_ext, s.body0, s.body1, J0, J1, xf, DT)
    return dict(lam=xf, acc=af, wres=orc.fast_wres(s, rhs, CFM, xf, af), v6=v6, J0=J0, J1=J1, rhs=rhs)


def oracle(name, sweeps):
    if (name, sweeps) not in _oracle:
        sc = moving(name)[0]
        _oracle[name, sweeps] = oracle_step((sc["p"], sc["R"], sc["v"], sc["w"]), moving(name), sweeps)
    return _oracle[name, sweeps]


@pytest.mark.parametrize("name", SCENES)
def test_the_staged_prologue_keeps_every_bit(ctx, monkeypatch, name):
    case = moving(name)
    for sweeps in SWEEPS:
        what = (name, sweeps)
        on, f_on = step(ctx, monkeypatch, case, sweeps, "face")
        off, f_off = step(ctx, monkeypatch, case, sweeps, "share")
        assert f_on & capi.SCHED_FACE and f_on & capi.SCHED_DEFERRED_SYSTEM, what
        assert f_off == f_on & ~capi.SCHED_FACE, what
        tss.assert_same(on, off, what)
        tss.assert_oracle(on, oracle(name, sweeps), what)
    # the scene does what it is for: the two sides of a face between boxes weigh differently (g32 and g32p are one
    # layer of boxes on the ground: no such face)
    sc, Minv, _ = case
    two = (sc["body0"] >= 0) & (sc["body1"] >= 0)
    assert two.any() == (not name.startswith("g32"))
    assert (Minv[sc["body0"][two], 3, 3] != Minv[sc["body1"][two], 3, 3]).all()


def test_the_form_is_off_where_the_plan_is_not_faced(ctx, monkeypatch):
    case = moving("h2half")
    for sweeps in (2, 9):
        on, f_on = step(ctx, monkeypatch, case, sweeps, "face")
        off, f_off = step(ctx, monkeypatch, case, sweeps, "share")
        assert not f_on & capi.SCHED_FACE and f_on & capi.SCHED_SHARE and f_off == f_on, sweeps
        tss.assert_same(on, off, sweeps)
        tss.assert_oracle(on, oracle_step((case[0]["p"], case[0]["R"], case[0]["v"], case[0]["w"]), case, sweeps), sweeps)


def test_unequal_linear_masses_take_the_fused_launch_away(ctx, monkeypatch):
    """Bodies of different mass on the two sides of a face: the fused launch's precondition (one linear weight on both
    sides) fails, no form of it is reported, and the step is still the oracle's."""
    case = moving("h2", unequal_mass=True)
    on, f_on = step(ctx, monkeypatch, case, 9, "face")
    off, f_off = step(ctx, monkeypatch, case, 9, "share")
    assert f_on == f_off and not f_on & (capi.SCHED_FACE | capi.SCHED_SHARE | capi.SCHED_LINSYM)
    tss.assert_same(on, off, "h2")
    sc = case[0]
    tss.assert_oracle(on, oracle_step((sc["p"], sc["R"], sc["v"], sc["w"]), case, 9), "h2")


@pytest.mark.parametrize("name", ["two", "g32p"])
def test_later_steps_read_the_current_state(ctx, monkeypatch, name):
    """step, advance (the state arrays swap), step; then set_state with another state, step.  Every step against the
    same sequence with EGS_STEP_FACE=0 byte for byte, and against the oracle from the state the problem reports."""
    case = moving(name)
    sc, Minv, f_ext = case
    rng = np.random.default_rng(5)
    n = sc["p"].shape[0]
    other = (sc["p"] + rng.uniform(-2e-3, 2e-3, (n, 3)), sc["R"], rng.uniform(-0.6, 0.6, (n, 3)) + 0.01,
             rng.uniform(-1.2, 1.2, (n, 3)) + 0.01)
    got = {}
    for form in ("face", "share"):
        tsf.set_env(monkeypatch, form)
        pr = build(ctx, case)
        try:
            prm = tss.params("gs", 9)
            pr.step(DT, ERP, prm)
            first = read(pr)
            pr.advance(DT)
            moved = pr.state()
            pr.step(DT, ERP, prm)
            second = read(pr)
            pr.set_state(other[0], other[1], other[2], other[3], Minv, f_ext)
            pr.step(DT, ERP, prm)
            third = read(pr)
            got[form] = (first, second, third, moved)
        finally:
            pr.close()
    moved = got["face"][3]
    for a, b in zip(moved, got["share"][3]):
        assert a.tobytes() == b.tobytes()
    assert moved[0].tobytes() != sc["p"].tobytes()          # advance moved the bodies
    states = ((sc["p"], sc["R"], sc["v"], sc["w"]), moved, other)
    for k, label in enumerate(("first", "after advance", "after set_state")):
        (on, f_on), (off, f_off) = got["face"][k], got["share"][k]
        assert f_on & capi.SCHED_FACE and f_off == f_on & ~capi.SCHED_FACE, (name, label)
        tss.assert_same(on, off, (name, label))
        tss.assert_oracle(on, oracle_step(states[k], case, 9), (name, label))
    assert got["face"][0][0]["lam"].tobytes() != got["face"][1][0]["lam"].tobytes()
    assert got["face"][1][0]["lam"].tobytes() != got["face"][2][0]["lam"].tobytes()


def test_a_body_outside_the_tiles_moves_by_its_force(ctx, monkeypatch):
    """`two` plus one body in no constraint: the form is on, and the free body's velocity is v + dt W f."""
    case = moving("two", free_body=True)
    sc, Minv, f_ext = case
    on, f_on = step(ctx, monkeypatch, case, 2, "face")
    off, f_off = step(ctx, monkeypatch, case, 2, "share")
    assert f_on & capi.SCHED_FACE and f_off == f_on & ~capi.SCHED_FACE
    tss.assert_same(on, off, "two + free body")
    tss.assert_oracle(on, oracle_step((sc["p"], sc["R"], sc["v"], sc["w"]), case, 2), "two + free body")
    Wf = np.einsum("ij,j->i", Minv[-1], f_ext[-1])
    want = np.concatenate([sc["v"][-1], sc["w"][-1]]) + DT * Wf
    assert (on["acc"][-1] == 0).all()
    # two roundings, the product and the sum, each within half an ulp of a term no larger than |v| + dt |W f|
    bound = 2 * np.finfo(float).eps * (np.abs(np.concatenate([sc["v"][-1], sc["w"][-1]])) + DT * np.abs(Wf))
    assert (np.abs(on["v6"][-1] - want) <= bound).all()
