"""GPU (-m gpu): world steps with every feature on at once (tests/world_combo_cases.py), every step of every scene

  a  against an egs_problem built by hand from the state the step read, the world's contact list and the per-constraint
     tables the world must have filled in -- bit for bit: contacts, blocks, start and sources, lambda, bodies, mass;
  b  each ensemble of a batch against the world that holds it alone -- bit for bit; one that sits out keeps every bit;
  c  against the composed 50-digit reference (tests/combo_reference.py), stage by stage, with the bounds the references
     already carry: the Checked tolerances for M^-1, torque, blocks, err and rhs; exact x0; friction_reference.BOUNDS of
     the class "pile" (contact piles with joints at cfm 0.01, as sweep_reference's joint-contact case) for lambda,
     accumulators, w and the residual; test_gpu_model_reference.py's for velocities and poses.  Accumulators and w come
     from the hand-built problem, whose lambda check a has just shown to be the world's.
     Where a scene needs more than the class constant for a or w -- the kernels CARRY the accumulators through the
     sweeps, so they keep rounding noise of the size of the largest iterate, while the class bounds are stated at the
     final x: a bouncing contact that lets go under the pyramid ends at x = 0, a cold start = rhs starts far out -- the
     bound is 4 x the worst ratio of combo_reference.carried_sweeps, a CPU twin that carries them too, over the steps
     of the CPU twin's run of that scene (combo_reference.carried_worst; DESIGN.md section 6f has both numbers);
  d  for the sweep form choose_sweep gives it: these lists hold joints, friction, a given start or anisotropic bodies, and
     they are small, so none of LINSYM, FUSED_ASSEMBLY, DEFERRED_SYSTEM, PAIR, CHAIN, SHARE may be reported; FRICTION
     exactly with a friction table, START exactly on a warm step; and the problem reports the same bits;
  e  the contact count changes between steps, so the list is re-planned under angular blocks with the motors, the
     coefficients and the warm match filled in again.

fp32: bits are compared after the cast to fp32; a Checked tolerance gains the one rounding to fp32 the device makes after
assembling in fp64 (combo_reference.worst); velocities and poses follow fp32 lambdas, so their bounds are taken in units
of 2^-24 where the fp64 rule has 2^-53.

The dense steps of DENSE have the mixed-LCP conditions (1e-9, sweep_reference.mixed_lcp_violation on the 50-digit A) in
place of the sweeps' reference and agree with egs_problem_step_dense to 1e-9 (the rule of tests/test_gpu_world_dense.py);
the sweep steps between them are held as above, with the start taken from the dense lambda.

The hand-built problem of check a always assembles with EACH = no: for a step_each scene the two kernels are held to each
other's bits.

The scenes of world_combo_cases.PLUS_TABLE add hinge stops (H), sliders with motor and travel stops (D), capsules (C) and
rays (Y) and go through a - e as above, with the two stop tables set on the hand-built problem, and

  f  after every step of a scene with rays: World.cast_rays is the stateless Context.cast_rays on the bodies read back and
     ray_twin's, bit for bit, and within ray_reference's bound; a second world of the scene that never casts has the same
     bits after every step; in a batch a ray sees its own ensemble only, and the rays of the ensemble that sits out return
     the hits of the step before.

A row pinned by lo == hi (the platform's rail row before it reaches its stop) is in none of the residual's sums (DESIGN.md
section 4k); combo_reference.check_solution states that rule beside friction_reference's.

assemble_kernel<REAL, EACH, RATES, REST, ANGULAR, LIMITS, SLIDER> (RATES follows EACH): launch_assemble and
launch_assemble_each have eight launch sites each -- slider (ANGULAR, SLIDER), limits (ANGULAR, LIMITS), angular, plain;
each with and without REST -- times two REAL.  The test of this file whose world launches each; a bare scene name stands
for test_one_ensemble_scenes[<scene>] or, with a +, test_one_ensemble_plus_scenes[<scene>].  The hand-built problem of a
scene launches the EACH = no site of its row as well.

  branch   EACH  REST  double                                              float
  slider   no    yes   ALL+, ALL+-minus-H, ALL+-minus-C, test_batch[BATCH+-step]   ALL+32
  slider   no    no    the problem of ALL+-minus-R-each                             ALL+32-minus-R
  slider   yes   yes   test_batch[BATCH+]                                           ALL+32-each
  slider   yes   no    ALL+-minus-R-each                                            ALL+32-minus-R-each
  limits   no    yes   ALL+-minus-D                                                 ALL+32-minus-D
  limits   no    no    (see below)                                                  ALL+32-minus-DR
  limits   yes   yes   ALL+-minus-D-each                                            ALL+32-minus-D-each
  limits   yes   no    (see below)                                                  ALL+32-minus-DR-each
  angular  no    yes   ALL, ALL-minus-P / -W / -L / -S, test_batch[BATCH-step], DENSE, DENSE+   ALL32
  angular  no    no    ALL-minus-R                                                  ALL+32-minus-HDR
  angular  yes   yes   test_batch[BATCH]                                            ALL32-each
  angular  yes   no    ALL-minus-R-each                                             ALL+32-minus-HDR-each
  plain    no    yes   ALL-minus-K                                                  ALL+32-minus-KHDY
  plain    no    no    (see below)                                                  (see below)
  plain    yes   yes   (see below)                                                  ALL+32-minus-KHDY-each
  plain    yes   no    (see below)                                                  (see below)

Seven sites are launched by no scene of this file (a scene without restitution and without a slider that has hinge limits
in fp64; a list without joint kinds and without restitution, or in fp64 under step_each with it) and are launched by
  limits   no / yes   no   double   test_gpu_limits_world.py::test_batched_ensembles_are_their_own_worlds[step] / [step_each]
  plain    no / yes   no   double   test_gpu_world_step_each.py::test_equal_rates_equal_the_scalar_entry[*-f64] (both entries)
  plain    no / yes   no   float    test_gpu_world_step_each.py::test_equal_rates_equal_the_scalar_entry[*-f32]
  plain    yes        yes  double   test_gpu_restitution_world.py::test_batched_world_ensembles_are_their_own_worlds[step_each]"""
import numpy as np
import pytest

import combo_reference as cr
import friction_reference as fr
import joint_reference as jr
import restitution_reference as rr
import sweep_reference as sw
import world_combo_cases as wc
from eggshell_amd import capi
from test_gpu_world_step_each import ensemble_view, same_bits

pytestmark = pytest.mark.gpu

CLASS = "pile"
FAST_FORMS = (capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_DEFERRED_SYSTEM | capi.SCHED_PAIR | capi.SCHED_CHAIN |
              capi.SCHED_SHARE)
BLOCKS = ("J0", "J1", "is_eq", "lo", "hi", "rhs", "err")


def bits(sc, a, b):
    """Bit for bit; an fp32 scene compares what the device holds, the values after the cast to fp32."""
    a, b = np.asarray(a), np.asarray(b)
    if sc.f32 and a.dtype == np.float64:
        with np.errstate(over="ignore"):
            return same_bits(a.astype(np.float32), b.astype(np.float32))
    return same_bits(a, b)


def problem_step(ctx, sc, state, mass, contacts, dt, erp, x0=None, dense_cfm=None):
    """The step of a one-ensemble scene on a hand-built problem: the state and mass the world's step read, the world's
    contact list behind the scene's joints, kinds and motors, live inertia, mu and rest per constraint (-1 on the
    joints), START_GIVEN with the world's start.  Everything the problem can report afterwards."""
    e = sc.ens[0]
    case, motor, mu, rest, lim, travel = cr.full_case(sc, state, mass, contacts, dt, erp)
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"], capi.F32 if sc.f32 else capi.F64)
    try:
        pr.set_state(*state, mass[0], mass[1])
        pr.set_constraints(case["kind"], case["data"])
        if motor is not None:
            pr.set_motors(motor)
        if lim is not None:
            pr.set_hinge_limits(lim)
        if travel is not None:
            pr.set_slider_limits(travel)
        if sc.live:
            pr.set_live_inertia(e["I_body"])
        if mu is not None:
            pr.set_friction(mu)
        if rest is not None:
            pr.set_restitution(rest, sc.vth)
        out = dict(case=case, motor=motor, mu=mu, rest=rest, lim=lim, travel=travel, mass_before=pr.mass())
        if dense_cfm is not None:
            out["ok"], _ = pr.step_dense(dt, erp, dense_cfm, use_bounds=1)
        else:
            if x0 is not None:
                pr.set_start(capi.START_GIVEN, x0)
            st = pr.step(dt, erp, capi.params(**sc.prm), want_stats=True)
            assert st.status == capi.OK
            out.update(residual=st.residual, schedule=pr.schedule_full(), forms=pr.schedule_forms(), acc=pr.accumulators(), wres=pr.wres())
        out.update(blocks=pr.blocks(), lam=pr.lambda_(), v6=pr.velocity())
        pr.advance(dt)
        out.update(after=pr.state(), mass=pr.mass())
    finally:
        pr.close()
    return out


class Single:
    """The world of a one-ensemble scene, stepped as the scene says; step(k) returns what the step read and left."""

    def __init__(self, ctx, sc):
        self.ctx, self.sc = ctx, sc
        self.w, _ = wc.make_world(ctx, sc)
        self.prev = None
        # f: a second world of the scene that is stepped without ever casting a ray
        self.blind = wc.make_world(ctx, sc)[0] if sc.rays else None

    def step(self, k):
        sc, w = self.sc, self.w
        dt, erp = sc.rates[k]
        if dt[0] == 0.0:
            return None
        rec = dict(k=k, dt=dt[0], erp=erp[0], state=w.bodies(), mass_in=w.mass(), prev=self.prev if sc.warm else None,
                   dense=sc.entry == "dense" and k % 2 == 1, replans=w.info()["replans"])
        if rec["dense"]:
            if k == 1:
                assert w.step_dense(dt[0], erp[0], wc.CFM, use_bounds=1) == 0
            else:
                assert w.step_dense_each(dt, erp, wc.CFM, use_bounds=1) == 0
            rec["cfm"] = float(w.dense_info()["cfm"][0])
            rec["cond"] = float(w.dense_info()["condition"][0])
        elif sc.entry == "step_each":
            st = w.step_each(dt, erp, capi.params(**sc.prm), want_stats=True)
        else:
            st = w.step(dt[0], erp[0], capi.params(**sc.prm), want_stats=True)
        if not rec["dense"]:
            assert st.status == capi.OK
            rec.update(schedule=st.schedule, residual=st.residual, iterations=st.iterations)
        rec.update(contacts=w.contacts(), blocks=w.blocks(), lam=w.lambda_(), after=w.bodies(), mass=w.mass(),
                   replanned=w.info()["replans"] > rec["replans"])
        rec["x0"], rec["src"] = w.start() if sc.warm and not rec["dense"] else (None, None)
        self.prev = rec["contacts"] + (rec["lam"],)
        if sc.rays:
            rec["rays"] = w.cast_rays()
            if sc.entry == "step_each":
                self.blind.step_each(dt, erp, capi.params(**sc.prm))
            else:
                self.blind.step(dt[0], erp[0], capi.params(**sc.prm))
            rec["blind"] = self.blind.bodies() + (self.blind.lambda_(),) + self.blind.contacts() + self.blind.mass()
        return rec

    def close(self):
        self.w.close()
        if self.blind is not None:
            self.blind.close()


def check_step(ctx, sc, rec, worst):
    """Checks a, c and d on one step of a one-ensemble scene."""
    k, f32, e = rec["k"], sc.f32, sc.ens[0]
    who = (sc.name, k)
    mj = len(cr.joints_of(e)[0])
    # ---- a: the world is the problem ----
    pb = problem_step(ctx, sc, rec["state"], rec["mass_in"], rec["contacts"], rec["dt"], rec["erp"], rec["x0"], rec.get("cfm"))
    for name, a, b in zip(BLOCKS, rec["blocks"], pb["blocks"]):
        assert bits(sc, a, b) if name != "err" else same_bits(a, b), who + ("blocks", name)
    # (the getters refresh a live mass at the pose held when they are called: before the step that is the pose it reads)
    for a, b in zip(rec["mass_in"], pb["mass_before"]):
        assert bits(sc, a, b), who + ("mass before",)
    v6 = np.concatenate([rec["after"][2], rec["after"][3]], axis=1)
    if rec["dense"]:
        assert pb["ok"]
        after = rec["after"] + rec["mass"], pb["after"] + pb["mass"]
        exact = same_bits(rec["lam"], pb["lam"]) and all(same_bits(a, b) for a, b in zip(*after))
        print("%s step %d (dense, cfm %g, condition %.3g): world and problem %s" % (sc.name, k, rec["cfm"], rec["cond"],
                                                                                 "bit for bit" if exact else "within 1e-9"))
        assert np.abs(rec["lam"] - pb["lam"]).max() <= 1e-9 * max(1.0, np.abs(pb["lam"]).max()), who
        for a, b in zip(*after):
            assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), who
    else:
        assert bits(sc, rec["lam"], pb["lam"]), who + ("lambda",)
        assert bits(sc, v6, pb["v6"]), who + ("velocity",)
        for a, b in zip(rec["after"], pb["after"]):
            assert bits(sc, a, b), who + ("bodies",)
        for a, b in zip(rec["mass"], pb["mass"]):
            assert bits(sc, a, b), who + ("mass after",)
    # ---- the reference of the step, and what its guard bands leave out: nothing ----
    case = pb["case"]
    J0, J1, is_eq, lo, hi, rhs, err = rec["blocks"]
    twin_rhs, what, margin = rr.twin_rhs(case, J0, J1, err, pb["rest"], sc.vth)
    contact = np.repeat(case["kind"] == jr.CONTACT, 3)
    if not f32:
        assert same_bits(rhs[contact], twin_rhs[contact]), who + ("the contacts' rhs is the restitution twin's",)
    ref = cr.assembly_reference(sc, rec["state"], rec["mass_in"], rec["contacts"], rec["dt"], rec["erp"])
    assert ref["what"] == what, who
    left = cr.left_out(sc, dict(case=case, state=rec["state"], contacts=rec["contacts"], margin=margin, prev=rec["prev"], src=rec["src"],
                                cond=rec.get("cond"), lim=pb["lim"], travel=pb["travel"], after=rec["after"] if sc.rays else None))
    assert sum(left.values()) == 0, who + (left,)
    if pb["lim"] is not None or pb["travel"] is not None:      # the stops' decisions are the references', and their rows one-sided
        active, _ = cr.stop_reference(case, pb["lim"], pb["travel"])
        assert np.array_equal(active, ref["asm"]["active"]), who
        for i in np.nonzero(active)[0]:
            row = 3 * i + 2
            assert (lo[row], hi[row]) == ((-np.inf, 0.0) if active[i] > 0 else (0.0, np.inf)), who + ("stop row", i, lo[row], hi[row])
            assert rec["lam"][row] <= 0.0 if active[i] > 0 else rec["lam"][row] >= 0.0, who + ("a stop pulls", i, rec["lam"][row])
        rec["active"] = active
    # ---- c: stage by stage ----
    r = {}
    if sc.live:
        M, f, live = cr.mass_reference(sc, rec["state"])
        im, jf = cr.mass_entries(live)
        r["Minv"], r["torque"] = cr.worst(M, rec["mass_in"][0], f32, im), cr.worst(f, rec["mass_in"][1], f32, jf)
    r.update(cr.check_assembly(ref, rec["blocks"], f32))
    scale = sw.U[True] / sw.U[False] if f32 else 1.0
    r.update(cr.check_motion(case, ref["asm"], rec["lam"], v6, rec["after"], scale))
    if f32:      # p and R: Checked tolerances in units of 2^-53
        r["p"], r["R"] = r["p"] / scale, r["R"] / scale
    assert all(x <= 1.0 for x in r.values()), who + (r,)
    if rec["dense"]:
        A = sw.system(cr.flat(case, J0, J1, is_eq, lo, hi), rec["cfm"])
        r["lcp"] = float(sw.mixed_lcp_violation(A, rhs, rec["lam"], is_eq, lo, hi)) / 1e-9
        assert r["lcp"] <= 1.0, who + (r,)
    else:
        if sc.warm:
            want, wsrc = cr.expected_x0(rec["prev"], rec["contacts"], mj, rhs)
            assert np.array_equal(rec["src"], wsrc), who + ("sources", rec["src"], wsrc)
            assert bits(sc, rec["x0"], want), who + ("x0",)
        A, muf, x_ref = cr.lambda_reference(sc, case, rec["blocks"], pb["mu"], rec["x0"])
        s = cr.check_solution(A, muf, rec["blocks"], x_ref, rec["lam"], pb["acc"], pb["wres"], rec["residual"])
        carried = cr.carried_worst(sc.base, sc.index)
        bound = cr.solution_bounds(CLASS, f32, carried)
        for q, x in s.items():
            r[q] = x / bound[q]
            if x > fr.BOUNDS[(CLASS, f32)][q]:
                print("%s step %d: %s = %.4g u; class bound %g, the carried twin's worst %.4g, bound %.4g" %
                      (sc.name, k, q, x, fr.BOUNDS[(CLASS, f32)][q], carried.get(q, 0.0), bound[q]))
        assert all(r[q] <= 1.0 for q in s), who + (s, bound)
        # ---- d: the form ----
        sched = rec["schedule"]
        assert sched & FAST_FORMS == 0, who + (sched,)
        # (FACE is reported by egs_problem_get_schedule_forms alone -- a world's step stats mask the form bits -- so this
        # reads the hand-built problem's launch; that the world took the same one follows from the equal bits of check a)
        if (case["kind"] == wc.SLIDER).any():
            assert pb["forms"] & capi.SCHED_FACE == 0, who + (pb["forms"],)
        assert bool(sched & capi.SCHED_FRICTION) == (sc.mu is not None), who + (sched,)
        # (a world with a friction table takes the friction forms for a list of joints too; the problem, handed -1 for
        # every constraint, has friction off: the same bits, as checked above)
        if sc.warm and rec["prev"] is not None:
            assert sched & capi.SCHED_START, who + (sched,)
        if not sc.warm:
            assert not sched & capi.SCHED_START, who + (sched,)
        same = capi.SCHED_START | (0 if sc.mu is None or (pb["mu"] >= 0).any() else capi.SCHED_FRICTION)
        assert sched | same == pb["schedule"] | same, who + (sched, pb["schedule"])
    # ---- f: the rays between the steps ----
    if sc.rays:
        r["rays"] = check_rays(ctx, sc, rec, who)
    for q, x in r.items():
        worst[q] = max(worst.get(q, 0.0), x)
    return what


def check_rays(ctx, sc, rec, who):
    """Check f on one step of a one-ensemble scene: World.cast_rays on the state the step left is the stateless cast on the
    bodies read back and ray_twin's, bit for bit, and ray_reference's within its bound; the world that never casts has the
    same bits after the step.  Returns the worst error / bound."""
    e = sc.ens[0]
    t = e["rays"]
    pos, R = rec["after"][0], rec["after"][1]
    stateless = ctx.cast_rays(pos, R, e["side"], e["shape"], t["origin"], t["dir"], t["tmax"], t["body"])
    twin = cr.twin_rays(sc, rec["after"])
    for name, a, b, c in zip(("body", "t", "normal"), rec["rays"], stateless, twin):
        assert same_bits(a, b), who + ("rays: the world's cast is not the stateless cast", name)
        assert same_bits(a, c), who + ("rays: the world's cast is not the twin's", name)
    held = rec["after"] + (rec["lam"],) + rec["contacts"] + rec["mass"]
    for a, b in zip(held, rec["blind"]):
        assert same_bits(a, b), who + ("a world that casts between its steps differs from one that never does",)
    worst = cr.check_rays(sc, rec["after"], rec["rays"])
    assert worst <= 1.0, who + ("rays", worst)
    return worst


def report(name, worst):
    print("%s: worst ratio to bound: %s" % (name, " ".join("%s=%.3g" % kv for kv in sorted(worst.items()))))


SINGLES = [n for n in wc.NAMES if not n.startswith("BATCH")]


@pytest.mark.parametrize("name", SINGLES)
def test_one_ensemble_scenes(ctx, name):
    one_ensemble_scene(ctx, name)


PLUS_SINGLES = [n for n in wc.PLUS_NAMES if not n.startswith("BATCH")]


@pytest.mark.parametrize("name", PLUS_SINGLES)
def test_one_ensemble_plus_scenes(ctx, name):
    """Checks a, c, d, e and f on the scenes with hinge stops, sliders, capsules and rays; then, over the four steps: every
    stop is seen inactive and active, the list is re-planned in a step with an active stop (so the stop tables were
    filled in again under the new offsets: check a has compared that step's rows bit for bit), the stops' decisions are
    the twin run's, and a ray's nearest hit changes body."""
    sc = wc.scene(name)
    recs = one_ensemble_scene(ctx, name)
    twin = cr.twin_runs(name)[0]
    if sc.limits or sc.travel:
        mj = len(sc.ens[0]["joints"][0])
        acts = np.array([r["active"][:mj] for r in recs])
        assert not any(r["active"][mj:].any() for r in recs)
        assert np.array_equal(acts[:, :mj], np.array([t["tw"]["active"][:mj] for t in twin])), acts[:, :mj]
        stopped = np.nonzero(acts.any(axis=0))[0]
        want = int(sc.limits) + (2 if sc.travel else 0)
        assert len(stopped) == want and all((acts[:, i] == 0).any() for i in stopped), acts[:, :mj]
        assert any(r["replanned"] and r["active"].any() for r in recs[1:]), [(r["replanned"], r["active"].any()) for r in recs]
    if sc.rays:
        hits = [r["rays"][0] for r in recs]
        assert any(((a != b) & (a > -2) & (b > -2)).any() for a, b in zip(hits, hits[1:])), hits
        for r, t in zip(recs, twin):
            assert np.array_equal(r["rays"][0], t["rays"][0])


def one_ensemble_scene(ctx, name):
    sc = wc.scene(name)
    run = Single(ctx, sc)
    worst, counts, seen, replanned, recs = {}, [], set(), [], []
    try:
        for k in range(wc.STEPS):
            rec = run.step(k)
            what = check_step(ctx, sc, rec, worst)
            recs.append(rec)
            counts.append(len(rec["contacts"][0]))
            replanned.append(rec["replanned"])
            if k == 0:
                seen = set(what)
            if sc.kinds and not rec["dense"]:
                hinge = int(np.nonzero(sc.ens[0]["kinds"] == jr.HINGE)[0][0])
                assert abs(rec["lam"][3 * hinge + 2]) == np.float32(wc.MOTOR[1]) if sc.f32 else abs(rec["lam"][3 * hinge + 2]) == wc.MOTOR[1]
    finally:
        run.close()
    report(name, worst)
    # e: the list changes under the joints, and the world re-plans for it
    assert any(a != b for a, b in zip(counts, counts[1:])), counts
    assert all(r for (a, b), r in zip(zip(counts, counts[1:]), replanned[1:]) if a != b), (counts, replanned)
    if sc.rest is not None:
        assert {"bounce", "floor", "slow"} <= seen
    twin = [len(r["contacts"][0]) for r in cr.twin_runs(name)[0]]
    assert counts == twin, (counts, twin)
    return recs


@pytest.mark.parametrize("name", ["BATCH", "BATCH-step", "BATCH+", "BATCH+-step"])
def test_batch(ctx, name):
    """b, and a / c / d on each ensemble's own world; the rows of the ensemble that sits a step out are exactly 0.  With
    rays (f): each ensemble's rays return what its own world's cast returns, bit for bit -- so a ray sees its own ensemble
    only, and one of them passes through another ensemble's box -- and the rays of the ensemble that sits out return the
    hits of the step before."""
    sc = wc.scene(name)
    bw, off = wc.make_world(ctx, sc)
    singles = [Single(ctx, sc.single(e)) for e in range(len(sc.ens))]
    worst = {}
    sat = 0
    ro = np.concatenate([[0], np.cumsum([len(e["rays"]["body"]) for e in sc.ens])]) if sc.rays else None
    last_rays, crossed = [None] * len(sc.ens), 0
    try:
        for k, (dt, erp) in enumerate(sc.rates):
            before = bw.bodies()
            if sc.entry == "step_each":
                bw.step_each(dt, erp, capi.params(**sc.prm))
            else:
                bw.step(dt[0], erp[0], capi.params(**sc.prm))
            info = bw.batch_info()
            jo, co = info["joint_offset"], info["contact_offset"]
            mj = jo[-1]
            blocks = bw.blocks()
            x0, src = bw.start()
            cast = bw.cast_rays() if sc.rays else None
            view = lambda e: (np.where(cast[0][ro[e]:ro[e + 1]] >= 0, cast[0][ro[e]:ro[e + 1]] - off[e], cast[0][ro[e]:ro[e + 1]]),
                              cast[1][ro[e]:ro[e + 1]], cast[2][ro[e]:ro[e + 1]])
            rows = lambda v, e, d=3: np.concatenate([v[d * jo[e]:d * jo[e + 1]], v[d * (mj + co[e]):d * (mj + co[e + 1])]])
            for e, s in enumerate(singles):
                body, con, lam = ensemble_view(bw, info, off, e)
                if dt[e] == 0.0:
                    sat += 1
                    for a, b in zip(body, before):
                        assert same_bits(a, b[off[e]:off[e + 1]]), (name, k, e, "an ensemble that sits out moved")
                    assert (rows(blocks[5], e) == 0.0).all() and not np.signbit(rows(blocks[5], e)).any(), (name, k, e)
                    if sc.rays:
                        for a, b in zip(view(e), last_rays[e]):
                            assert same_bits(a, b), (name, k, e, "the rays of an ensemble that sits out")
                    continue
                rec = s.step(k)
                for a, b in zip(con, rec["contacts"]):
                    assert same_bits(a, b), (name, k, e, "contacts")
                assert same_bits(lam, rec["lam"]), (name, k, e, "lambda")
                for a, b in zip(body, rec["after"]):
                    assert same_bits(a, b), (name, k, e, "bodies")
                for i, nm in enumerate(BLOCKS[2:], 2):
                    assert same_bits(rows(blocks[i], e), rec["blocks"][i]), (name, k, e, nm)
                assert same_bits(rows(x0, e), rec["x0"]), (name, k, e, "x0")
                check_step(ctx, s.sc, rec, worst)
                if sc.rays:
                    last_rays[e] = view(e)
                    for a, b in zip(last_rays[e], rec["rays"]):
                        assert same_bits(a, b), (name, k, e, "rays")
                    # what the same rays would hit if they saw every ensemble's bodies
                    t = sc.ens[e]["rays"]
                    pos, R = bw.bodies()[:2]
                    every = cr.ray_twin.cast(pos, R, np.concatenate([x["side"] for x in sc.ens]), np.concatenate([x["shape"] for x in sc.ens]),
                                             t["origin"], t["dir"], t["tmax"], np.where(t["body"] >= 0, t["body"] + off[e], -1))
                    crossed += int((np.where(every[0] >= 0, every[0] - off[e], every[0]) != rec["rays"][0]).sum())
    finally:
        bw.close()
        for s in singles:
            s.close()
    assert sat == (1 if sc.entry == "step_each" else 0)
    assert crossed > 0 or not sc.rays, "no ray passes through a body of another ensemble"
    report(name, worst)


# ---- the dense step's refusals, with the other features on ------------------------------------------------------------------------
def snapshot(w):
    return w.bodies() + (w.lambda_(),) + w.contacts() + w.mass()


REFUSED = {"pyramid": "friction pyramid", "free hinge": "free hinge", "limited hinge": "no hinge limits: hinge joint",
           "slider with a finite stop": "no travel stops: slider joint"}


@pytest.mark.parametrize("why", ["pyramid", "free hinge", "limited hinge", "slider with a finite stop"])
def test_dense_refusals_leave_everything_as_it_was(ctx, why):
    """DENSE's world after a sweep step: the dense step refuses the pyramid (no dense friction configured) and a hinge
    without a motor, by name, and bodies, lambda and the warm history keep every bit -- the next sweep step is, start and
    sources included, that of a world which never made the refused call.  DENSE+'s world with the door's stops or the
    drawer's set (both joints motored, which the dense step would otherwise take as box rows): the same."""
    plus = why in ("limited hinge", "slider with a finite stop")
    sc = wc.build("DENSE+", wc.SEEDS["DENSE+"]) if plus else wc.build("DENSE", wc.SEEDS["DENSE"])
    if why == "free hinge":
        hinge = sc.ens[0]["kinds"] == jr.HINGE
        sc.ens[0]["motors"] = np.where(hinge[:, None], [0.0, -1.0], sc.ens[0]["motors"])
    worlds = [wc.make_world(ctx, sc)[0] for _ in range(2)]
    prm = capi.params(**sc.prm)
    try:
        for w in worlds:
            if why == "limited hinge":
                e = wc.build("ALL+", wc.SEEDS["DENSE+"]).ens[0]      # the same door with its table
                door = int(np.nonzero(e["limits"][:, 4:8].any(axis=1))[0][0])
                lim = np.zeros((len(sc.ens[0]["kinds"]), 8))
                at = int(np.nonzero((sc.ens[0]["kinds"] == jr.HINGE) & (sc.ens[0]["joints"][1] == -1))[0][0])
                lim[at] = e["limits"][door]
                w.set_joint_limits(lim)
            if why == "slider with a finite stop":
                travel = np.tile([-np.inf, np.inf], (len(sc.ens[0]["kinds"]), 1))
                travel[sc.ens[0]["kinds"] == wc.SLIDER] = wc.DRAWER_TRAVEL
                w.set_slider_limits(travel)
            if why == "pyramid":
                w.set_friction(wc.MU)
            w.step(wc.DT, wc.ERP, prm)
        w = worlds[0]
        held = snapshot(w)
        for each in (False, True):
            with pytest.raises(capi.EgsError) as ei:
                if each:
                    w.step_dense_each([wc.DT], [wc.ERP], wc.CFM, use_bounds=1)
                else:
                    w.step_dense(wc.DT, wc.ERP, wc.CFM, use_bounds=1)
            assert ei.value.status == capi.ERR_UNSUPPORTED
            assert REFUSED[why] in str(ei.value), str(ei.value)
            for a, b in zip(held, snapshot(w)):
                assert same_bits(a, b)
        outs = []
        for w in worlds:
            w.step(wc.DT, wc.ERP, prm)
            outs.append(snapshot(w) + w.start())
        assert (outs[0][-1] >= 0).any()
        for a, b in zip(*outs):
            assert same_bits(a, b)
    finally:
        for w in worlds:
            w.close()


# ---- a slider exactly ON a stop ---------------------------------------------------------------------------------------------------
def test_a_slider_exactly_on_its_stop_is_not_past_it(ctx):
    """The scenes keep every travel at least slider_reference.MARGIN from its stops (left_out == 0), so none of them can
    tell x > xhi from x >= xhi.  Here the comparison is no close call but an equality of exact fp64 numbers: a vertical
    rail through (0, 0, 2) and a piston at z = 2.25 (at z = 1.75) give D = (0, 0, +-0.25) and x = +-0.25 without a
    rounding, and the stop is at that very number.  "Past the stop" is x > xhi (x < xlo): the row stays the motor's
    (+-f) in the first ensemble and pinned in the second, on the device as in the twin and in the 50-digit decision;
    with the stop one ulp nearer it takes the row."""
    import math
    import slider_cases as sc_
    import slider_reference as sr
    from test_gpu_joints import assert_twin
    for bump, want in ((0.0, [0, 0]), (1.0, [1, -1])):
        at = math.nextafter(0.25, 0.0) if bump else 0.25      # the stop: at the travel, or one ulp inside it
        ens = [sc_.ens_piston(0.25, (-0.5, at), motor=(0.5, 3.0)), sc_.ens_piston(-0.25, (-at, 0.5), origin=(0.0, 5.0, 2.0))]
        assert ens[0]["p"][0, 2] == 2.25 and ens[1]["p"][0, 2] == 1.75 and all(e["joints"][2][1, 5] == 2.0 for e in ens)      # D is exact
        w, off = sc_.make_world(ctx, ens)
        try:
            w.step(wc.DT, wc.ERP, capi.params(method=capi.SOR, max_iters=wc.SWEEPS, tol=0.0, cfm=wc.CFM), detect_contacts=False)
            got = w.blocks()
        finally:
            w.close()
        cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
        case = dict(p=cat("p", 3), R=cat("R", 9), v=cat("v", 3), w=cat("w", 3), Minv=cat("Minv", 36), f_ext=cat("f_ext", 6),
                    kind=np.concatenate([e["kinds"] for e in ens]), body0=np.array([0, 0, 1, 1], np.int32), body1=np.full(4, -1, np.int32),
                    data=np.concatenate([e["joints"][2] for e in ens]), dt=wc.DT, erp=wc.ERP)
        motor = np.array([[0.0, -1.0], [0.5, 3.0], [0.0, -1.0], [0.0, -1.0]])
        travel = np.concatenate([e["travel"] for e in ens])
        tw = sr.twin_assemble(case, motor, travel)
        active, dist = cr.stop_reference(case, None, travel)
        assert list(tw["active"][[1, 3]]) == want and list(active[[1, 3]]) == want, (bump, tw["active"], active)
        assert_twin(got, tw, capi.F64, what="on the stop" if not bump else "one ulp past the stop")
        if not bump:
            assert dist[1] == 0.0 and dist[3] == 0.0 and tw["x"][1] == 0.25 and tw["x"][3] == -0.25
            assert (got[3][5], got[4][5]) == (-3.0, 3.0) and (got[3][11], got[4][11]) == (0.0, 0.0)
        else:
            assert (got[3][5], got[4][5]) == (-math.inf, 0.0) and (got[3][11], got[4][11]) == (0.0, math.inf)
