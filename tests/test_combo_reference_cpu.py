"""CPU: the combined-feature scenes (tests/world_combo_cases.py) and the composed reference (tests/combo_reference.py).
Every pair of features is on together in some scene; the recorded seeds are the first at which no reference leaves
anything out of a property, in any step; the fp64 twins and the oracle meet the composed 50-digit reference stage by
stage on every scene and step; and with one feature on the composition is that feature's own reference."""
import types

import numpy as np
import pytest

import combo_reference as cr
import friction_reference as fr
import joint_reference as jr
import model_reference as mr
import restitution_reference as rr
import sweep_reference as sw
import warm_start_reference as wsr
import world_combo_cases as wc

# the scenes are contact piles with joints in the same islands at cfm 0.01, as sweep_reference's "joint-contact": its class
CLASS = "pile"


def test_every_pair_of_features_is_on_together_somewhere():
    table = wc.pairs_covered()
    assert len(table) == len(wc.FEATURES) * (len(wc.FEATURES) - 1) // 2
    for pair, names in table.items():
        assert names, "no scene has %s on together" % sorted(pair)
    # and the table is what the scenes are built from, not a list beside them
    for name in wc.NAMES:
        sc = wc.scene(name)
        on = wc.TABLE[name][0]
        assert (sc.mu is not None) == ("P" in on) and (sc.rest is not None) == ("R" in on) and sc.warm == ("W" in on)
        assert sc.live == ("L" in on) and sc.shapes == ("S" in on) and sc.kinds == ("K" in on) and sc.f32 == ("32" in on)
        assert (sc.entry == "step_each") == ("E" in on)
        assert (sc.ens[0]["kinds"] is not None) == ("K" in on)
        if "S" in on:
            assert (sc.ens[0]["shape"] == wc.SPHERE).any() and len({tuple(s) for s in sc.ens[0]["side"]}) > 3
        if "L" in on:
            assert not cr.lic.is_skipped(sc.ens[0]["I_body"]).all() and np.abs(sc.ens[0]["w"]).min() > 0
        assert len(sc.rates) == wc.STEPS and all(e["p"].shape[0] <= 12 for e in sc.ens)


def test_the_batch_is_what_the_issue_of_its_ensembles_says():
    sc = wc.scene("BATCH")
    assert len(sc.ens) == 3 and sc.ens[1]["joints"] is None and sc.ens[2]["joints"] is not None
    assert len(set(sc.mu)) == 3 and len(set(sc.rest)) == 3 and -1.0 in sc.rest
    assert sc.rates[1][0][1] == 0.0 and all(dt[1] != 0.0 for k, (dt, _) in enumerate(sc.rates) if k != 1)
    assert len({tuple(dt) for dt, _ in sc.rates}) > 1 and all(len(set(dt)) == 3 for dt, _ in sc.rates)
    runs = cr.twin_runs("BATCH")
    assert all(len(r["contacts"][0]) == 0 for r in runs[2])                      # joints only
    assert all(len(r["contacts"][0]) > 0 for r in runs[1])
    kinds = {(int(sc.ens[1]["shape"][i]) if i >= 0 else -1, int(sc.ens[1]["shape"][j])) for r in runs[1] for i, j in zip(*r["contacts"][:2])}
    assert {(-1, 0), (-1, 1), (0, 1), (0, 0)} <= kinds


@pytest.mark.parametrize("name", wc.NAMES)
def test_nothing_is_left_out_and_the_seed_is_the_first_accepted(name):
    sc = wc.scene(name)
    runs = cr.twin_runs(name)
    for e, run in enumerate(runs):
        assert len(run) == wc.STEPS
        for k, rec in enumerate(run):
            assert all(v == 0 for v in rec["left_out"].values()), (name, e, k, rec["left_out"])
            assert sum(rec["left_out"].values()) == 0
            assert len(rec["contacts"][0]) + (0 if sc.ens[e]["joints"] is None else len(sc.ens[e]["joints"][0])) <= 40
    assert wc.accepts(sc.single(0) if len(sc.ens) > 1 else sc, runs) == []
    assert wc.redraw(name) == wc.SEEDS[name]


def test_all_replans_under_joints():
    counts = [len(r["contacts"][0]) for r in cr.twin_runs("ALL")[0]]
    assert any(a != b for a, b in zip(counts, counts[1:])), counts


@pytest.mark.parametrize("name", [n for n in wc.NAMES if "32" not in n])
def test_twins_meet_the_composed_reference(name):
    """Every stage of every step: the mass refresh, the assembly, the rhs with its decisions, lambda with its
    accumulators, w and residual, the velocities and the poses."""
    sc0 = wc.scene(name)
    worst = {}
    for e, run in enumerate(cr.twin_runs(name)):
        sc = sc0.single(e) if len(sc0.ens) > 1 else sc0
        for k, rec in enumerate(run):
            if rec["dt"] == 0.0:
                continue
            r = {}
            if sc.live:
                M, f, live = cr.mass_reference(sc, rec["state"])
                im, jf = cr.mass_entries(live)
                r["Minv"], r["torque"] = M.worst(rec["mass"][0], im)[0], f.worst(rec["mass"][1], jf)[0]
                assert cr.inertia_agrees(sc, rec["state"]) < 1e-30
            ref = cr.assembly_reference(sc, rec["state"], rec["mass"], rec["contacts"], rec["dt"], rec["erp"])
            assert ref["what"] == rec["what"], (name, e, k)
            tw = rec["tw"]
            blocks = (tw["J0"], tw["J1"], tw["is_eq"], tw["lo"], tw["hi"], tw["rhs"], tw["err"])
            r.update(cr.check_assembly(ref, blocks))
            r.update(cr.check_motion(ref["case"], ref["asm"], rec["lam"], rec["v6"], rec["after"]))
            assert all(x <= 1.0 for x in r.values()), (name, e, k, r)
            if rec["dense"]:
                A = sw.system(cr.flat(ref["case"], *blocks[:5]), rec["cfm"])
                r["lcp"] = float(sw.mixed_lcp_violation(A, tw["rhs"], rec["lam"], tw["is_eq"], tw["lo"], tw["hi"]))
                assert r["lcp"] <= 1e-9, (name, e, k, r)
            else:
                A, muf, x_ref = cr.lambda_reference(sc, ref["case"], blocks, rec["mu"], rec["x0"])
                s = cr.check_solution(A, muf, blocks, x_ref, rec["lam"], rec["acc"], rec["wres"], rec["res"])
                for q, x in s.items():
                    assert x <= fr.BOUNDS[(CLASS, False)][q], (name, e, k, q, x)
                r.update(s)
            for q, x in r.items():
                worst[q] = max(worst.get(q, 0.0), x)
    print("%s: twin against the composition, worst ratio to bound: %s" % (name, " ".join("%s=%.3g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", wc.NAMES)
def test_the_carried_twin_finds_the_references_lambda(name):
    """combo_reference.carried_sweeps, whose a and w ratios stand behind the GPU test's bounds where the class constants
    do not reach: its lambda is the reference's within the class bound, and the figures are printed for DESIGN.md."""
    sc = wc.scene(name)
    for e in range(len(sc.ens)):
        r = cr.carried_worst(name, e)
        print("%s[%d] %s: carried twin, worst over the steps: %s" % (name, e, "f32" if sc.f32 else "f64", " ".join("%s=%.4g" % kv for kv in sorted(r.items()))))
        assert r["x"] <= fr.BOUNDS[(CLASS, sc.f32)]["x"], (name, e, r)
        assert set(cr.solution_bounds(CLASS, sc.f32, r)) == {"x", "a", "w", "r"}


# ---- one feature on: the composition is that feature's reference ----------------------------------------------------------------
def same(a, b):
    return a.val == b.val and a.tol == b.tol and a.mag == b.mag


def test_joints_alone_are_joint_reference():
    case, motor, asm, _, _ = jr.generated("n4m8-b")
    rhs, what, (lo, hi) = cr.rhs_reference(case, asm, motor, None, 0.0)
    assert same(rhs, jr.rhs_reference(case, asm, motor))
    assert set(what) <= {"joint", "off"}
    blo, bhi = jr.motor_bounds(case, asm, motor)
    assert np.array_equal(lo, blo) and np.array_equal(hi, bhi)


def test_restitution_alone_is_restitution_reference():
    case, rest, vth = rr.generated("m40")[:3]
    asm = jr.assemble_reference(case)
    rhs, what, (lo, hi) = cr.rhs_reference(case, asm, None, rest, vth)
    want, wwhat = rr.rhs_reference(case, mr.assemble_reference(case), rest, vth)
    assert same(rhs, want) and what == wwhat and {"bounce", "floor", "slow"} <= set(what)
    assert np.array_equal(lo, asm["lo"]) and np.array_equal(hi, asm["hi"])


def test_nothing_on_is_model_reference():
    case = rr.generated("m40")[0]
    asm = mr.assemble_reference(case)
    assert same(cr.rhs_reference(case, jr.assemble_reference(case), None, None, 0.0)[0], mr.rhs_reference(case, asm))


def test_a_sitting_ensemble_has_rows_of_exactly_zero():
    case, rest, vth = rr.generated("m1-w0")[:3]
    out = dict(case, dt=0.0)
    asm = jr.assemble_reference(case)
    both = cr.rhs_each_reference([case, out], [asm, asm], [None, None], [rest, rest], vth)
    one = cr.rhs_reference(case, asm, None, rest, vth)[0]
    assert both.val[:3] == one.val and both.val[3:] == [0] * 3 and both.tol[3:] == [0] * 3
    assert both.worst(np.concatenate([one.array(), np.zeros(3)]))[0] <= 1.0
    assert both.worst(np.concatenate([one.array(), [0.0, 0.0, 1e-300]]))[0] == np.inf


@pytest.mark.parametrize("friction", [False, True])
def test_the_solve_alone_is_the_sweep_references(friction):
    cid, method = "start", sw.GAUSS_SEIDEL
    c = sw.case(cid)
    K = c.runs[method][0]
    sc = types.SimpleNamespace(prm=dict(method=method, omega=c.omega, max_iters=K, cfm=c.cfm), f32=False)
    case = dict(kind=np.zeros(c.s.m, np.int32), p=np.zeros((c.s.n, 3)), Minv=c.s.Minv, body0=c.s.body0, body1=c.s.body1)
    blocks = (c.s.J0, c.s.J1, c.s.is_eq, c.s.lo, c.s.hi, c.rhs, None)
    _, _, x = cr.lambda_reference(sc, case, blocks, fr.case_mu(cid) if friction else None, c.x0)
    want = (fr.case_iterates if friction else sw.case_iterates)(cid, method)[K]
    assert x == want


def test_warm_start_alone_is_the_matcher():
    rng = np.random.default_rng(5)
    old = (np.array([-1, -1, 0], np.int32), np.array([0, 1, 1], np.int32), rng.uniform(size=(3, 7)))
    new = (np.array([-1, 0, -1], np.int32), np.array([1, 1, 2], np.int32), old[2][[1, 2, 0]] + 1e-3)
    lam = rng.uniform(size=9)
    x0, src = cr.expected_x0(old + (lam,), new, 0, None)
    want, wsrc = wsr.match_contacts(*old[:2], old[2][:, :3], lam, [0, 3], [1], *new[:2], new[2][:, :3], np.zeros(9), [0, 3], wc.RADIUS)
    assert np.array_equal(src, wsrc) and np.array_equal(x0, want) and list(src) == [1, 2, -1]
    rhs = rng.uniform(size=9 + 6)
    x0, src = cr.expected_x0(None, new, 2, rhs)
    assert np.array_equal(x0, rhs) and (src == -2).all()
    x0, src = cr.expected_x0(old + (np.concatenate([rhs[:6], lam]),), new, 2, None)
    assert np.array_equal(x0[:6], rhs[:6]) and list(src) == [0, 1, 1, 2, -1]      # joints from their own rows; a contact's source counts contacts


def test_live_inertia_alone_is_the_mass_references():
    sc = wc.scene("ALL")
    e = sc.ens[0]
    state = (e["p"], e["R"], e["v"], e["w"])
    M, f, live = cr.mass_reference(sc, state)
    assert same(M, mr.minv_reference(e["R"], e["mass"], e["I_body"])) and same(f, mr.force_reference(e["R"], e["w"], e["mass"], e["I_body"]))
    cube = (e["side"] == 0.3).all(axis=1)      # a sphere and a cube have a multiple of I_3: the refresh skips them
    assert list(live) == list((e["shape"] == wc.BOX) & ~cube) and live.sum() >= 6 and cr.inertia_agrees(sc, state) < 1e-30
    im, jf = cr.mass_entries(live)
    assert M.worst(e["Minv"], im)[0] <= 1.0 and f.worst(e["f_ext"], jf)[0] <= 1.0
