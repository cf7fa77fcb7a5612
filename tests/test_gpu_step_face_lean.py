"""GPU (-m gpu): the LEAN kernels of the FACE form (EGS_STEP_FACE_LEAN; step_face.hip, policy.h: face_form_policy).  They
are the same source as the present kernels with fewer held products (168 VGPRs, six tiles per CU), the linear block's last
entry kept in its register through the second assembly, and the owner's rhs, inv and D off-diagonals parked in LDS
behind the accumulators.  Every operand and every multiply is the one the present kernels take: nothing may move by a
bit.

Scenes: step_face_cases.py's g32, g32p (groups of three, ground contacts: world sides), two (a deep tile and a partly
filled one), mixed, h2, g32:tilt, and three 8 x 4 x 2 piles side by side (three tiles, all resident at once), in motion
as test_gpu_step_face_prologue.py sets them: random v, w and f_ext, an inertia per body (the angular weights differ
across a face), dt 3.7e-3, erp 0.35.

  * 1, 2, 9 and 10 sweeps with EGS_STEP_FACE_LEAN=1: lambda, wres, the accumulators, velocity() and blocks() byte for
    byte against EGS_STEP_FACE_LEAN=0 and against EGS_STEP_FACE=0, and the step against the sequential oracle as
    test_gpu_step_face.py compares it;
  * forced splits (s1 = 1, the middle, S - 1; every tile, and one of three) with EGS_STEP_FACE_SLOTS = 2 and 1: the lean
    pieces kernel runs whole tiles, first parts and second parts on persistent workgroups;
  * five consecutive steps with advance and set_state between;
  * EGS_SCHED_FACE_LEAN is reported exactly when the form is forced (EGS_STEP_FACE_LEAN=1, EGS_STEP_FACE_TILES=6) or
    chosen (more than four tiles per CU where the policy predicts the shorter launch), and never on h2half, backward
    SOR or restitution, whose steps keep the bytes of the switch at 0."""
import numpy as np
import pytest

import bench
import restitution_reference as rr
import step_face_cases as sfc
import test_gpu_step_face as tsf
import test_gpu_step_face_prologue as tpr
import test_gpu_step_share as tss
from eggshell_amd import capi, scenes

pytestmark = pytest.mark.gpu

DT, ERP = tpr.DT, tpr.ERP
SCENES = ("g32", "g32p", "two", "mixed", "h2", "g32:tilt", "h2x3")
SWEEPS = (1, 2, 9, 10)
FORMS = capi.SCHED_FACE | capi.SCHED_FACE_SPLIT | capi.SCHED_FACE_LEAN
ENV = ("EGS_STEP_FACE_LEAN", "EGS_STEP_FACE_SLOTS", "EGS_STEP_FACE_SPLIT", "EGS_STEP_FACE_SPLIT_FORCE",
       "EGS_STEP_FACE_PERSIST", "EGS_STEP_FACE_VELOCITY")

_oracle = {}


_h2x3 = []


def moving(name):
    """(scene, Minv, f_ext) in motion: test_gpu_step_face_prologue.py's; h2x3: the three piles of
    test_gpu_step_face_split.py, set moving the same way, built here once"""
    if name != "h2x3":
        return tpr.moving(name)
    if not _h2x3:
        sc = scenes.concat([scenes.box_stack(8, 4, 2, jitter=1e-3, seed=k + 1, origin=(0.0, 100.0 * k)) for k in range(3)])
        rng = np.random.default_rng(2029)
        n = sc["p"].shape[0]
        sc["v"] = rng.uniform(0.05, 0.8, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
        sc["w"] = rng.uniform(0.05, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
        inertia = rng.uniform(0.05, 0.3, n)
        Minv = np.zeros((n, 6, 6))
        for k in range(3):
            Minv[:, k, k] = 1.0 / 1.25
            Minv[:, 3 + k, 3 + k] = 1.0 / inertia
        f_ext = rng.uniform(0.2, 3.0, (n, 6)) * rng.choice([-1.0, 1.0], (n, 6))
        f_ext[:, 2] -= 9.8 * 1.25
        _h2x3.append((sc, Minv, f_ext))
    return _h2x3[0]


def n_tiles(case):
    sc = case[0]
    return int(capi.debug_plan(sc["p"].shape[0], sc["body0"], sc["body1"], 256)["cons_tile"].max()) + 1


def set_env(monkeypatch, form, lean=None, split=None, slots=None, tiles=None):
    """form: "face" or "share" (EGS_STEP_FACE=0); lean: None (the policy), 0 or 1; split: None (the policy), 0 or (h, s1)"""
    tsf.set_env(monkeypatch, form, False, True, tiles)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if lean is not None:
        monkeypatch.setenv("EGS_STEP_FACE_LEAN", str(lean))
    if split == 0:
        monkeypatch.setenv("EGS_STEP_FACE_SPLIT", "0")
    elif split is not None:
        monkeypatch.setenv("EGS_STEP_FACE_SPLIT_FORCE", "%d,%d" % split)
    if slots is not None:
        monkeypatch.setenv("EGS_STEP_FACE_SLOTS", str(slots))


def read(pr):
    """every output of the step, the forms (the other three reports keep their bits: tss.outputs), then the blocks"""
    out, full = tss.outputs(pr, False)
    forms = pr.schedule_forms()
    assert forms & ~FORMS == full and not full & FORMS
    for k, a in zip(tpr.BLOCKS, pr.blocks()):
        out[k] = a
    return out, forms


def step(ctx, monkeypatch, case, sweeps, form="face", method="gs", rest=None, **env):
    set_env(monkeypatch, form, **env)
    pr = tpr.build(ctx, case)
    try:
        if rest is not None:
            pr.set_restitution(*rest)
        pr.step(DT, ERP, tss.params(method, sweeps))
        return read(pr)
    finally:
        pr.close()


def oracle(name, sweeps):
    if (name, sweeps) not in _oracle:
        case = moving(name)
        sc = case[0]
        _oracle[name, sweeps] = tpr.oracle_step((sc["p"], sc["R"], sc["v"], sc["w"]), case, sweeps)
    return _oracle[name, sweeps]


_present = {}


def present(ctx, monkeypatch, name, sweeps):
    """the step with EGS_STEP_FACE_LEAN=0 and no split, once per case, checked against the oracle"""
    if (name, sweeps) not in _present:
        got, forms = step(ctx, monkeypatch, moving(name), sweeps, lean=0, split=0)
        assert forms & capi.SCHED_FACE and not forms & (capi.SCHED_FACE_LEAN | capi.SCHED_FACE_SPLIT), (name, sweeps)
        tss.assert_oracle(got, oracle(name, sweeps), (name, sweeps))
        _present[name, sweeps] = (got, forms)
    return _present[name, sweeps]


@pytest.mark.parametrize("name", SCENES)
def test_lean_keeps_every_bit(ctx, monkeypatch, name):
    case = moving(name)
    assert n_tiles(case) >= (3 if name == "h2x3" else 1)
    for sweeps in SWEEPS:
        what = (name, sweeps)
        ref, f_ref = present(ctx, monkeypatch, name, sweeps)
        lean, f_lean = step(ctx, monkeypatch, case, sweeps, lean=1)
        share, f_share = step(ctx, monkeypatch, case, sweeps, form="share", lean=1)
        assert f_lean == f_ref | capi.SCHED_FACE_LEAN, what
        assert f_share == f_ref & ~capi.SCHED_FACE, what
        tss.assert_same(lean, ref, what)
        tss.assert_same(lean, share, what)
        tss.assert_oracle(lean, oracle(name, sweeps), what)


@pytest.mark.parametrize("name,sweeps", [("h2x3", 9), ("h2x3", 10), ("two", 10), ("g32p", 9)])
def test_lean_pieces_keep_every_bit(ctx, monkeypatch, name, sweeps):
    """the lean pieces kernel: forced splits on 2 and on 1 persistent workgroups; with one workgroup every second part
    finds its first part stored, with two some wait for it"""
    case = moving(name)
    n = n_tiles(case)
    ref, f_ref = present(ctx, monkeypatch, name, sweeps)
    heights = sorted({n + 5} | ({1} if n > 1 else set()))          # every tile (asked for with more: clamped); one of three
    for slots in (2, 1):
        # no split: the whole-tile list on persistent workgroups wherever the tiles outnumber the slots
        got, forms = step(ctx, monkeypatch, case, sweeps, lean=1, split=0, slots=slots)
        assert forms == f_ref | capi.SCHED_FACE_LEAN, (name, slots)
        tss.assert_same(got, ref, (name, slots))
        for h in heights:
            for s1 in sorted({1, sweeps // 2, sweeps - 1}):
                what = (name, sweeps, slots, h, s1)
                got, forms = step(ctx, monkeypatch, case, sweeps, lean=1, split=(h, s1), slots=slots)
                assert forms == f_ref | capi.SCHED_FACE_LEAN | capi.SCHED_FACE_SPLIT, what
                tss.assert_same(got, ref, what)
                tss.assert_oracle(got, oracle(name, sweeps), what)


@pytest.mark.parametrize("name", ["two", "h2x3"])
def test_five_steps_in_a_row(ctx, monkeypatch, name):
    """step, advance, step, set_state, step, advance, step, advance, step: every step's bytes against the present kernels';
    on h2x3 the lean launch is split on two persistent workgroups, so the ticket counter and the epochs carry over"""
    case = moving(name)
    sc, Minv, f_ext = case
    rng = np.random.default_rng(17)
    n = sc["p"].shape[0]
    other = (sc["p"] + rng.uniform(-2e-3, 2e-3, (n, 3)), sc["R"], rng.uniform(-0.6, 0.6, (n, 3)) + 0.01,
             rng.uniform(-1.2, 1.2, (n, 3)) + 0.01)
    split = dict(split=(2, 4), slots=2) if name == "h2x3" else {}
    got = {}
    for lean in (1, 0):
        set_env(monkeypatch, "face", lean=lean, **(split if lean else {}))
        pr = tpr.build(ctx, case)
        try:
            prm, seq = tss.params("gs", 9), []
            for k in range(5):
                pr.step(DT, ERP, prm)
                seq.append(read(pr))
                if k == 1:
                    pr.set_state(other[0], other[1], other[2], other[3], Minv, f_ext)
                else:
                    pr.advance(DT)
            got[lean] = seq
        finally:
            pr.close()
    want = capi.SCHED_FACE_LEAN | (capi.SCHED_FACE_SPLIT if split else 0)
    for k in range(5):
        (a, fa), (b, fb) = got[1][k], got[0][k]
        assert fa == fb | want and not fb & FORMS & ~capi.SCHED_FACE, (name, k)
        tss.assert_same(a, b, (name, k))
    for k in range(4):
        assert got[1][k][0]["lam"].tobytes() != got[1][k + 1][0]["lam"].tobytes()
    first = got[1][0][0]
    tss.assert_oracle(first, oracle(name, 9), name)


def test_the_bit_follows_the_switches(ctx, monkeypatch):
    case = moving("two")
    ref, f_ref = present(ctx, monkeypatch, "two", 9)
    for env, lean in ((dict(), False), (dict(lean=1), True), (dict(tiles=6), True), (dict(lean=0, tiles=6), False),
                      (dict(lean=1, tiles=4), True), (dict(lean=1, tiles=3), True), (dict(tiles=4), False)):
        got, forms = step(ctx, monkeypatch, case, 9, **env)
        assert forms == f_ref | (capi.SCHED_FACE_LEAN if lean else 0), env
        tss.assert_same(got, ref, env)


@pytest.mark.parametrize("case", ["h2half", "sor", "restitution"])
def test_no_lean_launch_without_the_face_form(ctx, monkeypatch, case):
    if case == "h2half":
        cs, method, rest = moving("h2half"), "gs", None
    else:
        cs, method = moving("h2"), ("sor" if case == "sor" else "gs")
        rest = None if case == "sor" else (np.array([rr.COEFFICIENTS[i % 5] for i in range(cs[0]["body0"].shape[0])]), 0.5)
    for sweeps in (2, 9):
        on, f_on = step(ctx, monkeypatch, cs, sweeps, method=method, rest=rest, lean=1)
        off, f_off = step(ctx, monkeypatch, cs, sweeps, method=method, rest=rest, lean=0)
        assert f_on == f_off and not f_on & FORMS and f_on & capi.SCHED_SHARE, (case, sweeps)
        tss.assert_same(on, off, (case, sweeps))


def test_the_policy_chooses_lean_above_four_tiles_per_cu(ctx, monkeypatch):
    """Whole C3 piles, as many as put the tile count just above four per CU: with no switch set the launch is the one
    egs_debug_face_form predicts to be shorter, the bit says so, and the bytes are those of the switch at 0."""
    cus = ctx.cu_count()
    nx, ny, nz = bench.WORKLOADS["c3"][:3]
    piles = (4 * cus) // 64 + 1                      # a C3 pile is 64 tiles of 256 constraints
    sc = scenes.concat([scenes.box_stack(nx, ny, nz, jitter=1e-3, seed=k + 1, origin=(0.0, 100.0 * k)) for k in range(piles)])
    tiles = int(sc["kind"].shape[0]) // 256
    assert 4 * cus < tiles <= 6 * cus
    sweeps = 3
    want = capi.debug_face_form(tiles, cus, 64, 8, sweeps)["lean"]
    assert want                                      # one lean round against two present ones
    got = {}
    for lean in (None, 0):
        tsf.set_env(monkeypatch, "face")
        for k in ENV + ("EGS_QUAD", "EGS_STEP"):
            monkeypatch.delenv(k, raising=False)
        if lean is not None:
            monkeypatch.setenv("EGS_STEP_FACE_LEAN", str(lean))
        pr, _ = bench.build_problem(ctx, sc, capi.F64)
        try:
            pr.step(5e-3, 0.2, tss.params("gs", sweeps))
            assert pr.stats().status == capi.OK
            got[lean] = (pr.lambda_(), pr.velocity(), pr.schedule_forms())
        finally:
            pr.close()
    assert got[None][2] & capi.SCHED_FACE and got[None][2] == got[0][2] | capi.SCHED_FACE_LEAN
    assert not got[0][2] & capi.SCHED_FACE_LEAN
    for a, b in zip(got[None][:2], got[0][:2]):
        assert a.tobytes() == b.tobytes()
