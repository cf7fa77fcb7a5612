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


# ---- the scenes with hinge stops, sliders, capsules and rays ------------------------------------------------------------------
def test_the_plus_table_is_what_the_scenes_are_built_from():
    for name in wc.PLUS_NAMES:
        sc = wc.scene(name)
        on = wc.PLUS_TABLE[name][0]
        assert (sc.mu is not None) == ("P" in on) and (sc.rest is not None) == ("R" in on) and sc.warm == ("W" in on)
        assert sc.live == ("L" in on) and sc.shapes == ("S" in on) and sc.kinds == ("K" in on) and sc.f32 == ("32" in on)
        assert (sc.entry == "step_each") == ("E" in on) and {"S", "L", "W"} <= set(on)
        e = sc.ens[0]
        dense = sc.entry == "dense"
        assert (e["kinds"] is not None) == ("K" in on)
        kinds = e["kinds"] if e["kinds"] is not None else np.zeros(len(e["joints"][0]), np.int32)
        assert (e["limits"] is not None) == ("H" in on) == sc.limits and (e["travel"] is not None) == ("D" in on) == sc.travel
        assert (kinds == wc.SLIDER).any() == ("D" in on or dense) and (e["shape"] == wc.CAPSULE).any() == ("C" in on) == sc.capsules
        assert (e["rays"] is not None) == ("Y" in on) == sc.rays
        if "H" in on:      # a motor and both stops on the door's axis row
            door = int(np.nonzero(e["limits"][:, 4:8].any(axis=1))[0][0])
            assert e["kinds"][door] == jr.HINGE and e["joints"][1][door] == -1 and e["motors"][door][1] > 0 and e["limits"][door, 4:8].all()
        if "D" in on:      # a motored slider between two bodies with both stops, one to the world with a lower stop only
            t, k = e["travel"], e["kinds"] == wc.SLIDER
            both = np.nonzero(k & np.isfinite(t).all(axis=1))[0]
            lower = np.nonzero(k & np.isfinite(t[:, 0]) & np.isinf(t[:, 1]))[0]
            assert len(both) == 1 and e["joints"][1][both[0]] >= 0 and e["motors"][both[0]][1] > 0
            assert len(lower) == 1 and e["joints"][1][lower[0]] == -1 and e["motors"][lower[0]][1] < 0
        if dense:          # motored, and no finite stop anywhere
            assert all(e["motors"][i][1] > 0 for i in np.nonzero((kinds == wc.SLIDER) | (kinds == jr.HINGE))[0])
        if "C" in on:      # box-shaped inertias: live inertia follows every capsule
            assert not cr.lic.is_skipped(e["I_body"][e["shape"] == wc.CAPSULE]).any()
        if "Y" in on:
            assert 14 <= len(e["rays"]["body"]) <= 20 and (e["rays"]["body"] >= 0).sum() >= 3 and (e["rays"]["body"] < 0).sum() >= 3
        assert len(sc.rates) == wc.STEPS and all(x["p"].shape[0] <= 18 for x in sc.ens)
    sc = wc.scene("BATCH+")
    assert len(sc.ens) == 3 and sc.ens[1]["joints"] is None and (sc.ens[1]["shape"] == wc.CAPSULE).any()
    assert sc.ens[2]["limits"] is not None and sc.ens[2]["travel"] is not None and sc.rates == wc.BATCH_RATES
    assert all(len(r["contacts"][0]) == 0 for r in cr.twin_runs("BATCH+")[2])


@pytest.mark.parametrize("name", wc.PLUS_NAMES)
def test_nothing_is_left_out_of_the_plus_scenes_and_the_seed_is_the_first_accepted(name):
    sc = wc.scene(name)
    runs = cr.twin_runs(name)
    for e, run in enumerate(runs):
        assert len(run) == wc.STEPS
        for k, rec in enumerate(run):
            assert all(v == 0 for v in rec["left_out"].values()), (name, e, k, rec["left_out"])
            if rec["dt"] != 0.0:
                want = {"collision", "restitution", "branch", "warm", "dense"} | ({"limit", "travel"} if sc.limits or sc.travel else set()) | \
                       ({"rays"} if sc.rays else set())
                assert set(rec["left_out"]) == want
            assert len(rec["contacts"][0]) + (0 if sc.ens[e]["joints"] is None else len(sc.ens[e]["joints"][0])) <= 48
    assert wc.accepts(sc.single(0) if len(sc.ens) > 1 else sc, runs) == []
    assert wc.redraw(name) == wc.SEEDS[name]


@pytest.mark.parametrize("name", [n for n in wc.PLUS_NAMES if "32" not in n])
def test_stop_decisions_and_rays_of_the_twins(name):
    """Every step of every ensemble: the twin's stop decisions (the half-angle comparison, the fp64 travel) are the
    references' (atan2, the 50-digit travel), the reference's stop rows carry the one-sided bounds, and the ray twin's
    hits on the poses the step left are ray_reference's bodies, its t and normal within ray_reference's bound."""
    sc0 = wc.scene(name)
    acts, worst = set(), 0.0
    for e, run in enumerate(cr.twin_runs(name)):
        sc = sc0.single(e) if len(sc0.ens) > 1 else sc0
        for k, rec in enumerate(run):
            if rec["dt"] == 0.0:
                if sc.rays:      # nothing moved: the hits of the step before
                    assert all(np.array_equal(a, b) for a, b in zip(rec["rays"], run[k - 1]["rays"]))
                continue
            active, dist = cr.stop_reference(rec["case"], rec["lim"], rec["travel"])
            assert np.array_equal(active, rec["tw"]["active"]), (name, e, k)
            for i in np.nonzero(active)[0]:
                r = 3 * i + 2
                acts.add((int(rec["case"]["kind"][i]), int(active[i])))
                assert (rec["tw"]["lo"][r], rec["tw"]["hi"][r]) == ((-np.inf, 0.0) if active[i] > 0 else (0.0, np.inf))
                assert rec["tw"]["err"][r] != 0.0 and (rec["tw"]["err"][r] > 0) == (active[i] > 0)
            if sc.rays:
                worst = max(worst, cr.check_rays(sc, rec["after"], rec["rays"]))
    if sc0.limits:
        assert (jr.HINGE, 1) in acts
    if sc0.travel:
        assert {(wc.SLIDER, 1), (wc.SLIDER, -1)} <= acts
    if sc0.rays:
        print("%s: ray twin against ray_reference, worst error / bound %.3g" % (name, worst))
        assert worst <= 1.0


def test_all_replans_under_joints():
    counts = [len(r["contacts"][0]) for r in cr.twin_runs("ALL")[0]]
    assert any(a != b for a, b in zip(counts, counts[1:])), counts


@pytest.mark.parametrize("name", [n for n in wc.NAMES + wc.PLUS_NAMES if "32" not in n])
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


@pytest.mark.parametrize("name", wc.NAMES + wc.PLUS_NAMES)
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


def test_hinge_limits_alone_are_limit_reference():
    """A list with hinge stops and nothing else on: every row but an active stop's is joint_reference's, value and
    tolerance; an active stop's err[2], tolerance and bounds are limit_reference's, and its motor is off the row."""
    case, motor, asm0, _, _ = jr.generated("n4m8-b")
    lim = cr.lr.make_limits(case, 0)
    asm = cr.stops_assembly_reference(case, lim, None)
    rhs, what, (lo, hi) = cr.rhs_reference(case, asm, motor, None, 0.0)
    rhs0 = jr.rhs_reference(case, asm0, motor)
    lo0, hi0 = jr.motor_bounds(case, asm0, motor)
    ref = cr.lr.case_reference(case, lim)
    seen = 0
    for i in range(case["kind"].shape[0]):
        act = ref[i][0] if ref[i] is not None else 0
        assert asm["active"][i] == act
        for k in range(3 * i, 3 * i + (2 if act else 3)):
            assert asm["err"].val[k] == asm0["err"].val[k] and asm["err"].tol[k] == asm0["err"].tol[k]
            assert rhs.val[k] == rhs0.val[k] and rhs.tol[k] == rhs0.tol[k] and (lo[k], hi[k]) == (lo0[k], hi0[k])
        assert asm["J0"].val[18 * i:18 * i + 18] == asm0["J0"].val[18 * i:18 * i + 18]
        if act:
            seen += 1
            k = 3 * i + 2
            assert asm["err"].val[k] == ref[i][1] and asm["err"].tol[k] == ref[i][2]
            assert (lo[k], hi[k]) == ((-np.inf, 0.0) if act > 0 else (0.0, np.inf))
            if jr.motor_applies(case, motor, i):      # the motor's target is not in the row: it is kk err[2] - J u
                assert rhs.val[k] != rhs0.val[k]
    assert seen > 0
    tw = cr.lr.twin_assemble(case, motor, lim)
    assert rhs.worst(tw["rhs"])[0] <= 1.0 and asm["err"].worst(tw["err"])[0] <= 1.0
    assert np.array_equal(tw["lo"], lo) and np.array_equal(tw["hi"], hi)


def test_sliders_alone_are_slider_reference():
    case, motor = cr.sr.generated("n4m8-b")
    travel = cr.sr.make_travel(case, "mixed")
    asm, asm0 = cr.stops_assembly_reference(case, None, travel), cr.sr.assemble_reference(case, travel)
    assert same(asm["err"], asm0["err"]) and same(asm["J0"], asm0["J0"]) and same(asm["J1"], asm0["J1"])
    assert np.array_equal(asm["active"], asm0["active"]) and asm["active"].any()
    rhs, what, (lo, hi) = cr.rhs_reference(case, asm, motor, None, 0.0)
    assert same(rhs, cr.sr.rhs_reference(case, asm0, motor))
    lo0, hi0 = cr.sr.bounds_reference(case, asm0, motor)
    assert np.array_equal(lo, lo0) and np.array_equal(hi, hi0)


def test_a_pinned_row_is_in_none_of_the_residuals_sums():
    """Free hinges (no motor): their axis rows are pinned by lo == hi == 0 and carry w != 0.  friction_port's residual
    sorts such a row as 'on lo with w < 0' or 'on hi with w > 0'; the kernels leave it out.
    check_solution holds a reported residual to the second rule: the port's own value misses it by the pinned rows' w,
    the value with those rows left out meets the class bound."""
    case, _, _, plain, _ = jr.generated("n4m8-b")
    s = cr.flat(case, plain["J0"], plain["J1"], plain["is_eq"], plain["lo"], plain["hi"])
    pinned = cr.pinned_rows(plain["is_eq"], plain["lo"], plain["hi"])
    assert pinned.any() and list(np.nonzero(pinned)[0] % 3) == [2] * int(pinned.sum())
    mu = np.full(s.m, -1.0)
    lam, acc, wres, res = cr.friction_port.sweeps(s, plain["rhs"], 0.01, mu, sw.GAUSS_SEIDEL, 1.0, 12)
    assert np.abs(wres[pinned]).max() > 1e-3 and (lam[pinned] == 0.0).all()
    left_out = cr.friction_port.residual(lam, np.where(pinned, 0.0, wres), plain["is_eq"], plain["lo"], plain["hi"], mu)
    assert res - left_out > 1e-3
    blocks = (plain["J0"], plain["J1"], plain["is_eq"], plain["lo"], plain["hi"], plain["rhs"], plain["err"])
    A = sw.system(s, 0.01, False)
    bound = fr.BOUNDS[(CLASS, False)]["r"]
    assert cr.check_solution(A, mu, blocks, lam, lam, acc, wres, left_out)["r"] <= bound
    assert cr.check_solution(A, mu, blocks, lam, lam, acc, wres, res)["r"] > 1e6 * bound
