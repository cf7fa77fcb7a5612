"""GPU (-m gpu): the FACE launch on fewer workgroups than it has pieces (step_face.hip; solve.cpp: choose_sweep).  Where
the tiles take more than one round of the resident slots, `slots` persistent workgroups take the whole-tile list -- or,
split in time, the list of parts -- piece after piece by ticket.  No small scene has
more tiles than the GPU has slots, so EGS_STEP_FACE_SLOTS=k stands for the slots here: 2 and 1, on three 8 x 4 x 2 piles
side by side (three tiles) and on the 32-box pile (one).  Every output must keep every bit of the launch with one
workgroup per tile (EGS_STEP_FACE_SPLIT=0), whose outputs test_gpu_step_face_split.py holds against the oracle.

With one slot a single workgroup walks the whole list in order, second parts behind their first parts; with two a
second part can wait for a first part that the other workgroup is still running.  Two problems stepping alternately on
one context check that the counter and the epochs carry from launch to launch."""
import pytest

import bench
import test_gpu_step_face_split as tsp
import test_gpu_step_share as tss
from eggshell_amd import capi

pytestmark = pytest.mark.gpu

DT, ERP = tss.DT, tss.ERP
SLOTS = (2, 1)


def set_env(monkeypatch, split, slots):
    tsp.set_env(monkeypatch, split)
    if slots is None:
        monkeypatch.delenv("EGS_STEP_FACE_SLOTS", raising=False)
    else:
        monkeypatch.setenv("EGS_STEP_FACE_SLOTS", str(slots))


def step(ctx, monkeypatch, name, sweeps, split, slots):
    set_env(monkeypatch, split, slots)
    pr, _ = bench.build_problem(ctx, tsp.scene(name), capi.F64)
    try:
        pr.step(DT, ERP, tss.params("gs", sweeps))
        return tsp.outputs(pr)
    finally:
        pr.close()


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("name", ["h2x3", "g32"])
def test_whole_tiles_on_fewer_workgroups(ctx, monkeypatch, name, slots):
    """The policy's own launch: persistent where there are more tiles than slots (no split is reported: at these sweep
    counts the policy does not cut), one workgroup per tile otherwise."""
    for sweeps in (1, 2, 9, 10):
        ref, f_ref = tsp.unsplit(ctx, monkeypatch, name, sweeps)
        got, forms = step(ctx, monkeypatch, name, sweeps, None, slots)
        assert forms == f_ref and not forms & capi.SCHED_FACE_SPLIT, (name, slots, sweeps)
        tss.assert_same(got, ref, (name, slots, sweeps))
        off, f_off = step(ctx, monkeypatch, name, sweeps, 0, slots)      # EGS_STEP_FACE_SPLIT=0: a workgroup per tile
        assert f_off == f_ref
        tss.assert_same(off, ref, (name, slots, sweeps))


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("name", ["h2x3", "g32"])
def test_forced_splits_on_fewer_workgroups(ctx, monkeypatch, name, slots):
    for sweeps in (2, 9, 10):
        ref, f_ref = tsp.unsplit(ctx, monkeypatch, name, sweeps)
        for h in tsp.heights(name):
            for s1 in tsp.cuts(sweeps):
                what = (name, slots, sweeps, h, s1)
                got, forms = step(ctx, monkeypatch, name, sweeps, (h, s1), slots)
                assert forms == f_ref | capi.SCHED_FACE_SPLIT, what
                tss.assert_same(got, ref, what)


def test_the_policy_splits_on_two_slots_at_many_sweeps(ctx, monkeypatch):
    """Three tiles on two slots leave a last round half empty: at 100 sweeps the policy cuts the last tile."""
    ref, f_ref = tsp.unsplit(ctx, monkeypatch, "h2x3", 100)
    got, forms = step(ctx, monkeypatch, "h2x3", 100, None, 2)
    assert forms == f_ref | capi.SCHED_FACE_SPLIT
    tss.assert_same(got, ref, "h2x3")


def run_steps(ctx, monkeypatch, names, split, slots, n_steps=4, sweeps=9):
    set_env(monkeypatch, split, slots)
    prs, outs = [bench.build_problem(ctx, tsp.scene(n), capi.F64)[0] for n in names], []
    try:
        for k in range(n_steps):
            for pr, name in zip(prs, names):
                pr.step(DT, ERP, tss.params("gs", sweeps))
                outs.append(tsp.outputs(pr)[0])
                tsp.advance_some(pr, tsp.scene(name), k)
        return outs
    finally:
        for pr in prs:
            pr.close()


@pytest.mark.parametrize("slots", SLOTS)
def test_two_problems_step_alternately(ctx, monkeypatch, slots):
    names = ("two", "h2x3")
    ref = run_steps(ctx, monkeypatch, names, 0, None)
    for split in (None, (7, 4), (1, 8)):
        got = run_steps(ctx, monkeypatch, names, split, slots)
        assert len(got) == len(ref) == 8
        for k, (g, r) in enumerate(zip(got, ref)):
            tss.assert_same(g, r, (slots, split, k))
