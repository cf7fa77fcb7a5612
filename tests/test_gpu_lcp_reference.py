"""GPU (-m gpu): the dense direct LCP solvers against the certified reference of tests/lcp_reference.py (DESIGN.md
section 7d): Lcp::MixedConstraintsSolver under both pivot rules and batched, SolveLCP_BoxDantzig / BoxMurty / BoxSchur
and its batch, and the dense step of a problem and of a world.  Per case: ok as the oracle; the active set read off x
equal to the certified one row for row, clamped x equal to their bound and w on equality rows equal to zero bit for bit;
x, the backward error of the free system and w within the constants the CPU statements produced
(tests/test_lcp_reference_cpu.py) -- never the device's own figures.  Every test prints its figures:
`<case> dev-<entry> [<class>]: x  b  wf  wc` in the units of lcp_reference.measure."""
import numpy as np
import pytest

import lcp_reference as lr
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def check(label, entry, cls, ref, prob, x, w):
    A, b, Ceq, lo, hi = prob
    fig = lr.measure(ref, A, b, Ceq, lo, hi, x, w)
    print("%s dev-%s [%s]: x %.3g  b %.3g  wf %.3g  wc %.3g   (rows %d %d %d %d; kappa %.3g)" %
          (label, entry, cls, fig["x"], fig["b"], fig["wf"], fig["wc"], fig["row_x"], fig["row_b"], fig["row_wf"], fig["row_wc"], ref.kappa))
    bad = lr.within(fig, cls)
    assert not bad, (label, entry, cls, bad, fig, lr.BOUNDS[cls])


def check_case(cid, entry, x, w, cls=None):
    c = lr.case(cid)
    check(cid, entry, cls or c.cls, lr.reference(cid), (c.A, c.b, c.Ceq, c.lo, c.hi), x, w)


@pytest.mark.parametrize("cid", lr.MIXED_REF)
def test_mixed_constraints_reference_rule(ctx, cid):
    """egs_mixed_constraints_solve with use_bounds 0 / 1.  The pivot loop sees the inequality rows: boxi / c5i (none
    other) at 1 ... 112 run in murty_small_kernel, at 113, 128 (one panel), 129 (two), 193 and 300 (three and more,
    ragged) a launch per pivot; c5 / box / spec / pile put the Schur stage of the equality rows in front.  ok and the
    pivot count are the oracle's, which fixes the path the pivots took."""
    c = lr.case(cid)
    ok, x, w, piv = ctx.mixed_constraints_solve(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=c.use_bounds)
    oko, _, _, pivo = orc.mixed_constraints(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=c.use_bounds)
    assert ok and oko and piv == pivo
    check_case(cid, "mixed%d" % c.use_bounds, x, w)


@pytest.mark.parametrize("cid", lr.MIXED_BLOCK)
def test_mixed_constraints_block_rule(ctx, cid):
    """The same entry with block principal pivoting (use_bounds 2 / 3): always a launch per pivot, the multi-panel
    factorisations, from 1024 rows the split upload and the 1024 limits of the condition and back-solve kernels,
    boxeq-n1200 with 1077 equality rows, C5 itself at 2048.  Bordered pivots (EGS_DENSE_TRACE shows them): c5-n2048
    takes three (pivots 4 to 6 of its 6, 20 rows in and 21 out against the factored set at the last), and so do the
    other cases of 1023 rows and more; under the reference's rule (the test above) every pivot but the first of a
    launch-per-pivot case is one."""
    c = lr.case(cid)
    ok, x, w, piv = ctx.mixed_constraints_solve(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=c.use_bounds + 2)
    assert ok and piv > 0
    if c.n <= 300:
        assert orc.mixed_constraints(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=c.use_bounds)[0]
    check_case(cid, "block%d" % (c.use_bounds + 2), x, w)


def test_pile_without_bounds_fails_as_the_oracle(ctx):
    """use_bounds = 0 on a pile is degenerate (x = 0 and w = 0 on the tangential rows; no certificate exists,
    test_lcp_reference_cpu.test_pile_without_bounds_is_degenerate): the reference's rule ends at its 1000-pivot cap
    in the oracle, and on the device, in the single-workgroup kernel (96 rows) and on the launch-per-pivot path
    (144 rows)."""
    for cid in ("pile222-cfm0.01", "pile223-cfm0.01"):
        c = lr.case(cid)
        ok, _, _, piv = ctx.mixed_constraints_solve(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=0)
        oko, _, _, pivo = orc.mixed_constraints(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=0)
        assert not ok and not oko and piv == pivo == 1000


def test_mixed_constraints_batch(ctx):
    """One ragged batch through egs_mixed_constraints_solve_batch: n = 31, 32, 33 / 63, 64, 65 / 111, 112 in the three
    fused classes, 113 falling through to the single entry; box and spectrum families with their boxes.  Every
    problem against its own reference."""
    cs = [lr.case(cid) for cid in lr.BATCH]
    assert sorted({c.n for c in cs}) == sorted(lr.BATCH_SIZES) and all(c.use_bounds == 1 for c in cs)
    oks, xs, ws, pivs = ctx.mixed_constraints_solve_batch([c.A for c in cs], [c.b for c in cs], [c.Ceq for c in cs],
                                                          [c.lo for c in cs], [c.hi for c in cs], use_bounds=1)
    for c, ok, x, w, piv in zip(cs, oks, xs, ws, pivs):
        oko, _, _, pivo = orc.mixed_constraints(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=1)
        assert ok and oko and piv == pivo, c.id
        check_case(c.id, "batch", x, w)


@pytest.mark.parametrize("cid", lr.LCP_BOX + lr.LCP_SCHUR)
def test_box_lcp_entries(ctx, cid):
    """SolveLCP_BoxDantzig, BoxMurty and BoxSchur with either inner algorithm: 24 ... 96 rows with one wavefront in
    LDS, 97 and 200 with four; the schur cases have rows without bounds, so nub > 0 and the Schur stage runs.  Pivot
    counts as the oracle's."""
    c = lr.case(cid)
    if c.nub == 0:
        ok, x, w, _, _, piv = ctx.box_lcp_dantzig(c.A, c.b, c.lo, c.hi)
        assert ok and piv == orc.tk_box_dantzig(c.A, c.b, c.lo, c.hi)[5]
        check_case(cid, "dantzig", x, w, lr.lcp_class(c, False))
        ok, x, w, _, _, piv = ctx.box_lcp_murty(c.A, c.b, c.lo, c.hi)
        assert ok and piv == orc.tk_box_murty(c.A, c.b, c.lo, c.hi)[5]
        check_case(cid, "murty", x, w, lr.lcp_class(c, True))
    for alg in (0, 1):
        ok, x, w, _, _, nub, piv = ctx.box_lcp_schur(c.A, c.b, c.lo, c.hi, algorithm=alg)
        ro = orc.tk_box_schur(c.A, c.b, c.lo, c.hi, algorithm=alg)
        assert ok and ro[0] and nub == c.nub == ro[5] and piv == ro[6]
        check_case(cid, "schur%d" % alg, x, w, lr.lcp_class(c, alg == 0))


@pytest.mark.parametrize("alg", [0, 1])
def test_box_lcp_schur_batch(ctx, alg):
    """egs_box_lcp_schur_batch on the cases of up to 97 rows (96 and below fused, 97 one after another), with and
    without unbounded rows, every problem against its own reference."""
    cs = [lr.case(cid) for cid in lr.LCP_BATCH]
    assert {c.n for c in cs} == set(lr.LCP_SIZES) and any(c.nub for c in cs)
    oks, xs, ws, _, _, nubs, _ = ctx.box_lcp_schur_batch([c.A for c in cs], [c.b for c in cs], [c.lo for c in cs], [c.hi for c in cs],
                                                         algorithm=alg)
    for c, ok, x, w, nub in zip(cs, oks, xs, ws, nubs):
        assert ok and nub == c.nub, c.id
        check_case(c.id, "schurbatch%d" % alg, x, w, lr.lcp_class(c, alg == 0))


# ---- the dense step: the reference's inputs are the device's own dense_system(cfm) and the rhs of blocks() --------------
def resident(ctx, n, cons, st, Minv, f_ext):
    kind, b0, b1, data = cons
    pr = capi.Problem(ctx, n, b0, b1)
    pr.set_state(st["p"], st["R"], st["v"], st["w"], Minv, f_ext)
    pr.set_constraints(kind, data)
    return pr


def device_system(pr, dt, erp, cfm, use_bounds):
    """(A, rhs, is_eq, lo, hi) of an assembled problem as the dense step solves it.  The upper triangle is mirrored
    from the lower one (the assembly is symmetric to rounding only and the certificate wants one matrix; the assembly
    itself has its reference in section 6a); use_bounds = 0 is quirk Q3, lo = 0 and hi = inf."""
    pr.assemble(dt, erp)
    A = pr.dense_system(cfm)
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    A = np.tril(A) + np.tril(A, -1).T
    _, _, is_eq, lo, hi, rhs, _ = pr.blocks()
    if not use_bounds:
        lo, hi = np.zeros_like(lo), np.full_like(hi, np.inf)
    return A, rhs, is_eq, lo, hi


def check_step(label, entry, cls, prob, lam):
    """lambda of a dense step against the certified solution of the system it solved; w is not returned by the step,
    so its figures are those of w = 0 on the rows off a bound and of the exact A lambda - b on the clamped rows."""
    A, b, Ceq, lo, hi = prob
    ref = lr.solve(A, b, Ceq, lo, hi)
    assert lr.margins_ok(ref, cls), (label, ref.margin_x, ref.margin_w)
    w = np.zeros_like(b)
    Cl = np.flatnonzero(lr.state_of(lam, Ceq, lo, hi) >= lr.LO)
    w[Cl] = lr.exact_rows(A, b, [np.asarray(lam, dtype=np.float64)], Cl)
    check(label, entry, cls, ref, prob, lam, w)


@pytest.mark.parametrize("scene,cfm,ub,cls", [("chain8", 0.0, 0, "single"), ("stack222", 0.01, 1, "single-hard")])
def test_problem_step_dense(ctx, scene, cfm, ub, cls):
    """egs_problem_step_dense on Chain(8) (24 equality rows) and on box_stack(2,2,2) at cfm = 0.01 with its box
    (96 rows): lambda against the certified solution of the device's own system."""
    sc = scenes.chain(8) if scene == "chain8" else scenes.box_stack(2, 2, 2)
    dt = 1e-3 if scene == "chain8" else 5e-3
    n = sc["p"].shape[0]
    Minv = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    pr = resident(ctx, n, (sc["kind"], sc["body0"], sc["body1"], sc["data"]), sc, Minv, f_ext)
    prob = device_system(pr, dt, 0.2, cfm, ub)
    ok, piv = pr.step_dense(dt, 0.2, cfm, use_bounds=ub)
    assert ok
    lam = pr.lambda_()
    pr.close()
    check_step(scene, "step", cls, prob, lam)


@pytest.mark.parametrize("kind", ["chains", "piles"])
def test_world_step_dense(ctx, kind):
    """egs_world_step_dense with E = 3: Chain(8) between two shorter chains (no contact detection: the links of the
    reference's chain touch corner to corner), and box_stack(2,2,2) between two smaller piles with use_bounds = 1,
    contacts from the device, cfm = 0.01 added by the world's own condition check.  Each ensemble's slice of lambda
    against the certified solution of that ensemble's system, assembled by the device from the pre-step state and
    the world's own contact list."""
    from test_gpu_world_dense import ensemble, make_world, pile, states, view
    if kind == "chains":
        ens = [ensemble(scenes.chain(5)), ensemble(scenes.chain(8, anchor=(0.0, 5.0, 2.0))), ensemble(scenes.chain(3, anchor=(0.0, 9.0, 2.0)))]
        dt, ub, cls, kw = 1e-3, 0, "single", dict(detect_contacts=False)
    else:
        ens = [pile(1, 1, 2, seed=4), pile(2, 2, 2, seed=5, origin=(3.0, 0.0)), pile(2, 1, 2, seed=6, origin=(6.0, 0.0))]
        dt, ub, cls, kw = 5e-3, 1, "single-hard", {}
    w, off = make_world(ctx, ens)
    pre = states(w, off, ens)
    assert w.step_dense(dt, 0.2, 0.01, use_bounds=ub, **kw) == 0
    info = w.dense_info()
    assert info["ok"].all()
    for e in range(3):
        _, cons, lam = view(w, off, e, ens[e])
        pr = resident(ctx, ens[e]["p"].shape[0], cons, pre[e], ens[e]["Minv"], ens[e]["f_ext"])
        prob = device_system(pr, dt, 0.2, float(info["cfm"][e]), ub)
        pr.close()
        assert prob[1].shape[0] == lam.shape[0] and (kind == "chains") == (info["cfm"][e] == 0.0)
        check_step("%s-e%d" % (kind, e), "world", cls, prob, lam)
    w.close()
