"""GPU (-m gpu): the FACE launch split in time (EGS_STEP_FACE_SPLIT; step_face.hip, policy.h).  A split tile runs as
two workgroups: the first part walks the accumulation and sweeps 1 .. s1, stores lambda and the accumulators and
publishes the tile; the second part waits for it and resumes with sweeps s1 + 1 .. S.  Every body's accumulator sees the
same updates in the same order, so lambda, w, the accumulators, the velocities and the blocks of a step must keep every
bit of

  * the same step with EGS_STEP_FACE_SPLIT=0 (one workgroup per tile, blockIdx = tile: the launch as it was),
  * the sequential CPU oracle (as test_gpu_step_face.py compares it).

The scenes are the small faced piles of step_face_cases.py and three 8 x 4 x 2 piles side by side (three tiles).  On all
of them every workgroup of the launch is resident at once, so every second part really waits for its first part: the
hard case of the hand-over.  EGS_STEP_FACE_SPLIT_FORCE=h,s1 splits the last h tiles after s1 sweeps: all tiles, one,
and a strict subset, at S = 2, 3, 9, 10 with s1 = 1, S - 1 and the middle.  Consecutive steps on one problem and two
problems stepping alternately on one context check the ticket counter and the flags' epochs from launch to launch.

EGS_SCHED_FACE_SPLIT is read from egs_problem_get_schedule_forms alone."""
import numpy as np
import pytest

import bench
import restitution_reference as rr
import step_face_cases as sfc
import test_gpu_step_face as tsf
import test_gpu_step_share as tss
from eggshell_amd import capi, scenes

pytestmark = pytest.mark.gpu

DT, ERP = tss.DT, tss.ERP
SCENES = ("g32", "g32p", "two", "mixed", "h2", "h2x3")
SWEEPS = (2, 3, 9, 10)
FORMS = capi.SCHED_FACE | capi.SCHED_FACE_SPLIT


def scene(name):
    key = "face/" + name
    if key not in tss._scenes and name == "h2x3":
        tss._scenes[key] = scenes.concat([scenes.box_stack(8, 4, 2, jitter=1e-3, seed=k + 1, origin=(0.0, 100.0 * k))
                                          for k in range(3)])
    return tsf.scene(name)


_tiles = {}


def n_tiles(name):
    if name not in _tiles:
        sc = scene(name)
        _tiles[name] = int(capi.debug_plan(sc["p"].shape[0], sc["body0"], sc["body1"], 256)["cons_tile"].max()) + 1
    return _tiles[name]


def set_env(monkeypatch, split, steady=True, tiles=None, form="face"):
    """split: None (the policy), 0 (EGS_STEP_FACE_SPLIT=0) or (h, s1) (EGS_STEP_FACE_SPLIT_FORCE)."""
    tsf.set_env(monkeypatch, form, False, steady, tiles)
    monkeypatch.delenv("EGS_STEP_FACE_SPLIT", raising=False)
    monkeypatch.delenv("EGS_STEP_FACE_SPLIT_FORCE", raising=False)
    if split == 0:
        monkeypatch.setenv("EGS_STEP_FACE_SPLIT", "0")
    elif split is not None:
        monkeypatch.setenv("EGS_STEP_FACE_SPLIT_FORCE", "%d,%d" % split)


def outputs(pr):
    """Every output of the step pr has just run, then the blocks (a store-free step makes them on demand), and the bits
    of egs_problem_get_schedule_forms; the other three reports keep theirs (tss.outputs asserts them)."""
    out, full = tss.outputs(pr, False)
    forms = pr.schedule_forms()
    assert forms & ~FORMS == full and not full & FORMS
    for name, a in zip(("J0", "J1", "is_eq", "lo", "hi", "rhs", "err"), pr.blocks()):
        out[name] = a
    return out, forms


def step(ctx, monkeypatch, sc, sweeps, split, steady=True, tiles=None, method="gs", rest=None, form="face"):
    set_env(monkeypatch, split, steady, tiles, form)
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    try:
        if rest is not None:
            pr.set_restitution(*rest)
        pr.step(DT, ERP, tss.params(method, sweeps))
        return outputs(pr)
    finally:
        pr.close()


_unsplit = {}


def unsplit(ctx, monkeypatch, name, sweeps):
    """The step with EGS_STEP_FACE_SPLIT=0, once per case, checked against the oracle."""
    if (name, sweeps) not in _unsplit:
        got, forms = step(ctx, monkeypatch, scene(name), sweeps, 0)
        assert forms & capi.SCHED_FACE and not forms & capi.SCHED_FACE_SPLIT, (name, sweeps)
        tss.assert_oracle(got, tsf.oracle(name, "gs", sweeps), (name, sweeps))
        _unsplit[(name, sweeps)] = (got, forms)
    return _unsplit[(name, sweeps)]


def cuts(sweeps):
    return sorted({1, sweeps // 2, sweeps - 1} - {0})


def heights(name):
    """all tiles (asked for with more than there are: clamped), one, and a strict subset of more than one where there is"""
    n = n_tiles(name)
    return sorted({n + 5} | ({1} if n > 1 else set()) | ({2} if n > 2 else set()))


@pytest.mark.parametrize("name", SCENES)
def test_split_keeps_every_bit(ctx, monkeypatch, name):
    assert n_tiles(name) >= (3 if name == "h2x3" else 1)
    for sweeps in SWEEPS:
        ref, f_ref = unsplit(ctx, monkeypatch, name, sweeps)
        for h in heights(name):
            for s1 in cuts(sweeps):
                what = (name, sweeps, h, s1)
                got, forms = step(ctx, monkeypatch, scene(name), sweeps, (h, s1))
                assert forms == f_ref | capi.SCHED_FACE_SPLIT, what
                tss.assert_same(got, ref, what)
                tss.assert_oracle(got, tsf.oracle(name, "gs", sweeps), what)


@pytest.mark.parametrize("name", ["two", "h2x3"])
def test_no_cut_inside_the_sweeps_runs_unsplit(ctx, monkeypatch, name):
    """One sweep has no place for a cut, nor has s1 = 0 or s1 = S: the launch is the unsplit one."""
    for sweeps, s1 in ((1, 1), (1, 0), (9, 0), (9, 9), (9, 12)):
        ref, f_ref = unsplit(ctx, monkeypatch, name, sweeps)
        got, forms = step(ctx, monkeypatch, scene(name), sweeps, (n_tiles(name), s1))
        assert forms == f_ref and not forms & capi.SCHED_FACE_SPLIT, (name, sweeps, s1)
        tss.assert_same(got, ref, (name, sweeps, s1))


@pytest.mark.parametrize("name", ["two", "h2x3"])
def test_the_policy_leaves_small_launches_alone(ctx, monkeypatch, name):
    """Fewer tiles than resident slots: no split without the force, and the same launch as with the switch at 0."""
    ref, f_ref = unsplit(ctx, monkeypatch, name, 10)
    got, forms = step(ctx, monkeypatch, scene(name), 10, None)
    assert forms == f_ref
    tss.assert_same(got, ref, name)


def advance_some(pr, sc, k):
    """between steps: nothing, an explicit advance, or the initial state again"""
    if k % 3 == 1:
        pr.advance(DT)
    elif k % 3 == 2:
        Minv, f_ext = bench.host_mass_and_force(sc)
        pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)


def run_steps(ctx, monkeypatch, names, split, n_steps=5, sweeps=9):
    """n_steps steps of each problem in turn on one context (one step of every problem, then the next), the outputs of
    every step"""
    set_env(monkeypatch, split)
    prs, outs = [bench.build_problem(ctx, scene(n), capi.F64)[0] for n in names], []
    try:
        for k in range(n_steps):
            for pr, name in zip(prs, names):
                pr.step(DT, ERP, tss.params("gs", sweeps))
                outs.append(outputs(pr))
                advance_some(pr, scene(name), k)
        return outs
    finally:
        for pr in prs:
            pr.close()


@pytest.mark.parametrize("names", [("h2x3",), ("two", "h2x3")], ids=["one-problem", "two-problems"])
def test_consecutive_launches(ctx, monkeypatch, names):
    """The ticket counter and the flags' epochs from launch to launch: five steps per problem, every one compared with the
    unsplit run of the same sequence."""
    ref = run_steps(ctx, monkeypatch, names, 0)
    for split in ((7, 4), (1, 8), (2, 1)):
        got = run_steps(ctx, monkeypatch, names, split)
        assert len(got) == len(ref) == 5 * len(names)
        for k, ((g, fg), (r, fr)) in enumerate(zip(got, ref)):
            assert fg == fr | capi.SCHED_FACE_SPLIT and fr & capi.SCHED_FACE, (names, split, k)
            tss.assert_same(g, r, (names, split, k))
    first, _ = unsplit(ctx, monkeypatch, names[0], 9)
    tss.assert_same(ref[0][0], first, names)


@pytest.mark.parametrize("name", ["two", "h2x3", "g32p"])
def test_both_tile_counts_and_the_general_loop_alone(ctx, monkeypatch, name):
    ref, f_ref = unsplit(ctx, monkeypatch, name, 9)
    for tiles in (3, 4):
        got, forms = step(ctx, monkeypatch, scene(name), 9, (n_tiles(name), 4), tiles=tiles)
        assert forms == f_ref | capi.SCHED_FACE_SPLIT, (name, tiles)
        tss.assert_same(got, ref, (name, tiles))
    # EGS_STEP_STEADY=0 takes the CHAIN form away and FACE with it: nothing to split
    single, f_single = step(ctx, monkeypatch, scene(name), 9, (n_tiles(name), 4), steady=False)
    off, f_off = step(ctx, monkeypatch, scene(name), 9, 0, steady=False)
    assert f_single == f_off and not f_single & FORMS, name
    tss.assert_same(single, off, name)
    tss.assert_same(single, ref, name)


@pytest.mark.parametrize("case", ["h2half", "sor", "restitution"])
def test_launches_without_the_face_form_do_not_split(ctx, monkeypatch, case):
    name, method, rest = ("h2half" if case == "h2half" else "h2"), ("sor" if case == "sor" else "gs"), None
    sc = scene(name)
    if case == "restitution":
        sc = dict(sc, v=sc["v"].copy())
        sc["v"][:, 2] -= np.random.default_rng(11).uniform(0.05, 2.0, sc["v"].shape[0])
        rest = (np.array([rr.COEFFICIENTS[i % 5] for i in range(sc["body0"].shape[0])]), 0.5)
    on, f_on = step(ctx, monkeypatch, sc, 9, (1, 4), method=method, rest=rest)
    off, f_off = step(ctx, monkeypatch, sc, 9, 0, method=method, rest=rest)
    assert f_on == f_off and not f_on & FORMS, case
    tss.assert_same(on, off, case)
