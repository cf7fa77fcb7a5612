"""GPU (-m gpu): the FACE form of the fused step launch (EGS_STEP_FACE; step_face.hip).  Where the plan lays the four
contact points of every box face 32 lanes apart (Plan::faced) and the four carry one normal, a tile runs on 128 threads,
a thread pair holds the four constraints, and the steady loop runs their four updates on one set of accumulator
registers behind one barrier.  The same doubles, the same multiplies, the same order: lambda, w, the accumulators and
the velocities of a step must keep every bit of

  * the same step with EGS_STEP_FACE=0 in the same process (the SHARE form),
  * the same step with EGS_STEP_PAIR=0 (one lane per constraint),
  * the sequential CPU oracle (as test_gpu_step_share.py compares it),

on the small faced scenes of step_face_cases.py (the 32-box pile with an idle wavefront at period 4, the same with twelve
groups of three, 8 x 4 x 2, two tiles of depth 16 and 64, a tile of period 8 beside one of period 4), at 1, 2, 3, 4, 9 and
10 sweeps, with EGS_STEP_STEADY=0, at both EGS_STEP_FACE_TILES, and on piles whose normal is tilted.  A group whose upper
pair carries a second normal (in the sign of a zero only, or tilted) must not report the form and must still match;
egs_problem_set_constraints decides again.  A pile with two contact points per face keeps SHARE.  Backward SOR, the
storing launch and restitution keep the SHARE form: their results are those with the form switched off.

EGS_SCHED_FACE is read from egs_problem_get_schedule_forms alone: the other three reports keep their bits
(test_gpu_step_share.py's outputs() asserts their equalities on every step here too)."""
import numpy as np
import pytest

import bench
import restitution_reference as rr
import step_face_cases as sfc
import test_gpu_step_share as tss
from eggshell_amd import capi

pytestmark = pytest.mark.gpu

DT, ERP = tss.DT, tss.ERP
SHARE_FORMS = tss.FUSED | capi.SCHED_CHAIN | capi.SCHED_SHARE


def set_env(monkeypatch, form, store=False, steady=True, tiles=None):
    """form: "face" (the default launch), "share" (EGS_STEP_FACE=0) or "lane" (EGS_STEP_PAIR=0)."""
    tss.set_env(monkeypatch, "lane" if form == "lane" else "share", store, steady)
    if form == "share":
        monkeypatch.setenv("EGS_STEP_FACE", "0")
    else:
        monkeypatch.delenv("EGS_STEP_FACE", raising=False)
    if tiles is None:
        monkeypatch.delenv("EGS_STEP_FACE_TILES", raising=False)
    else:
        monkeypatch.setenv("EGS_STEP_FACE_TILES", str(tiles))


def outputs(pr, store):
    out, full = tss.outputs(pr, store)          # asserts what schedule() and the statistics report beside full
    forms = pr.schedule_forms()
    assert forms & ~capi.SCHED_FACE == full and not full & capi.SCHED_FACE
    return out, forms


def step(ctx, monkeypatch, sc, method, sweeps, form, store=False, steady=True, tiles=None, rest=None):
    set_env(monkeypatch, form, store, steady, tiles)
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    try:
        if rest is not None:
            pr.set_restitution(*rest)
        pr.step(DT, ERP, tss.params(method, sweeps))
        return outputs(pr, store)
    finally:
        pr.close()


def scene(name):
    """step_face_cases.py's scene, also where test_gpu_step_share.py's oracle looks its scenes up"""
    key = "face/" + name
    if key not in tss._scenes:
        tss._scenes[key] = sfc.scene(name)
    return tss._scenes[key]


def oracle(name, method, sweeps, rest=None):
    scene(name)
    return tss.oracle("face/" + name, method, sweeps, rest)


def check_forms(ctx, monkeypatch, name, sweeps, faces, shares=True):
    """The default launch against EGS_STEP_FACE=0, EGS_STEP_PAIR=0 and the oracle; faces: must it report the form?"""
    sc, what = scene(name), (name, sweeps)
    on, s_on = step(ctx, monkeypatch, sc, "gs", sweeps, "face")
    share, s_share = step(ctx, monkeypatch, sc, "gs", sweeps, "share")
    lane, s_lane = step(ctx, monkeypatch, sc, "gs", sweeps, "lane")
    assert s_on & tss.FUSED == tss.FUSED and s_on & capi.SCHED_CHAIN and s_on & capi.SCHED_DEFERRED_SYSTEM, what
    assert bool(s_on & capi.SCHED_FACE) == faces and bool(s_on & capi.SCHED_SHARE) == shares, what
    assert s_share == s_on & ~capi.SCHED_FACE, what
    assert s_lane == s_on & ~(capi.SCHED_FACE | capi.SCHED_SHARE | capi.SCHED_CHAIN | capi.SCHED_PAIR), what
    tss.assert_same(on, share, what)
    tss.assert_same(on, lane, what)
    tss.assert_oracle(on, oracle(name, "gs", sweeps), what)
    return on


@pytest.mark.parametrize("name", sfc.GPU_SCENES + ("h2:tilt", "g32p:tilt"))
def test_face_keeps_every_bit(ctx, monkeypatch, name):
    for sweeps in sfc.SWEEPS:
        check_forms(ctx, monkeypatch, name, sweeps, faces=True)


@pytest.mark.parametrize("name", ["g32:zeroCD", "h2:zeroCD", "two:tiltCD", "g32p:tiltC"])
def test_a_second_normal_in_a_group_keeps_the_share_form(ctx, monkeypatch, name):
    for sweeps in (2, 9):
        check_forms(ctx, monkeypatch, name, sweeps, faces=False)


@pytest.mark.parametrize("name", ["g32:zeroB", "h2:zeroD"])
def test_a_second_normal_in_a_pair_keeps_the_chain_form(ctx, monkeypatch, name):
    for sweeps in (2, 9):
        check_forms(ctx, monkeypatch, name, sweeps, faces=False, shares=False)


def test_two_contact_points_per_face_keep_the_share_form(ctx, monkeypatch):
    for sweeps in (2, 9):
        check_forms(ctx, monkeypatch, "h2half", sweeps, faces=False)


@pytest.mark.parametrize("name", ["two", "g32p", "mixed"])
def test_both_tile_counts_and_the_general_loop_alone(ctx, monkeypatch, name):
    """EGS_STEP_FACE_TILES=3 and 4 run the same kernel at another LDS request; EGS_STEP_STEADY=0 takes the CHAIN form away
    and every form above it with it."""
    sc = scene(name)
    on, s_on = step(ctx, monkeypatch, sc, "gs", 9, "face")
    assert s_on & capi.SCHED_FACE
    for tiles in (3, 4):
        got, s = step(ctx, monkeypatch, sc, "gs", 9, "face", tiles=tiles)
        assert s == s_on
        tss.assert_same(got, on, (name, tiles))
    single, s_single = step(ctx, monkeypatch, sc, "gs", 9, "face", steady=False)
    assert s_single == s_on & ~(capi.SCHED_FACE | capi.SCHED_SHARE | capi.SCHED_CHAIN)
    tss.assert_same(single, on, name)
    tss.assert_oracle(on, oracle(name, "gs", 9), name)


def test_set_constraints_decides_again(ctx, monkeypatch):
    """One problem, three steps from the same state: one normal per face, then a group whose upper pair differs in the sign
    of a zero, then one normal per face again.  The form is on, off, on, and every step is the fresh problem's."""
    set_env(monkeypatch, "face")
    pr, _ = bench.build_problem(ctx, scene("h2"), capi.F64)
    try:
        for name, faces in (("h2", True), ("h2:zeroCD", False), ("h2", True)):
            sc = scene(name)
            pr.set_constraints(sc["kind"], sc["data"])
            pr.step(DT, ERP, tss.params("gs", 9))
            got, sched = outputs(pr, False)
            assert bool(sched & capi.SCHED_FACE) == faces and sched & capi.SCHED_SHARE, name
            fresh, s_fresh = step(ctx, monkeypatch, sc, "gs", 9, "face")
            assert s_fresh == sched
            tss.assert_same(got, fresh, name)
            tss.assert_oracle(got, oracle(name, "gs", 9), name)
            set_env(monkeypatch, "face")
    finally:
        pr.close()


@pytest.mark.parametrize("case", ["sor", "storing", "restitution"])
def test_the_launches_that_keep_share(ctx, monkeypatch, case):
    """Backward SOR, the storing launch and the restitution twin run the SHARE form with EGS_STEP_FACE on or off."""
    name = "h2"
    method, store, rest = ("sor" if case == "sor" else "gs"), case == "storing", None
    sc = scene(name)
    if case == "restitution":
        name = "h2:falling"
        if "face/" + name not in tss._scenes:
            sc = dict(sc, v=sc["v"].copy())
            sc["v"][:, 2] -= np.random.default_rng(11).uniform(0.05, 2.0, sc["v"].shape[0])
            tss._scenes["face/" + name] = sc
        sc = tss._scenes["face/" + name]
        rest = (np.array([rr.COEFFICIENTS[i % 5] for i in range(sc["body0"].shape[0])]), 0.5)
    for sweeps in (2, 9):
        on, s_on = step(ctx, monkeypatch, sc, method, sweeps, "face", store, rest=rest)
        off, s_off = step(ctx, monkeypatch, sc, method, sweeps, "share", store, rest=rest)
        assert s_on == s_off and s_on & SHARE_FORMS == SHARE_FORMS and not s_on & capi.SCHED_FACE, (case, sweeps)
        tss.assert_same(on, off, (case, sweeps))
        tss.assert_oracle(on, tss.oracle("face/" + name, method, sweeps, rest), (case, sweeps))
