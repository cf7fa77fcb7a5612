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

assemble_kernel<REAL, EACH, RATES, REST, ANGULAR> (RATES follows EACH), which scene's world launches which:

  REAL    EACH  REST  ANGULAR  scene
  double  no    yes   yes      ALL, ALL-minus-P / -W / -L / -S, BATCH-step, DENSE
  double  no    no    yes      ALL-minus-R
  double  no    yes   no       ALL-minus-K
  double  yes   yes   yes      BATCH
  double  yes   no    yes      ALL-minus-R-each
  float   no    yes   yes      ALL32
  float   yes   yes   yes      ALL32-each
  the other nine (ANGULAR = no without REST, or with EACH, or in fp32; float without REST) belong to one feature each and
  are reached by that feature's own tests (test_gpu_world_step_each.py, test_gpu_restitution_world.py, test_gpu_world_warm.py)

The hand-built problem of check a always assembles with EACH = no: for a step_each scene the two kernels are held to each
other's bits."""
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
    case, motor, mu, rest = cr.full_case(sc, state, mass, contacts, dt, erp)
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"], capi.F32 if sc.f32 else capi.F64)
    try:
        pr.set_state(*state, mass[0], mass[1])
        pr.set_constraints(case["kind"], case["data"])
        if motor is not None:
            pr.set_motors(motor)
        if sc.live:
            pr.set_live_inertia(e["I_body"])
        if mu is not None:
            pr.set_friction(mu)
        if rest is not None:
            pr.set_restitution(rest, sc.vth)
        out = dict(case=case, motor=motor, mu=mu, rest=rest, mass_before=pr.mass())
        if dense_cfm is not None:
            out["ok"], _ = pr.step_dense(dt, erp, dense_cfm, use_bounds=1)
        else:
            if x0 is not None:
                pr.set_start(capi.START_GIVEN, x0)
            st = pr.step(dt, erp, capi.params(**sc.prm), want_stats=True)
            assert st.status == capi.OK
            out.update(residual=st.residual, schedule=pr.schedule_full(), acc=pr.accumulators(), wres=pr.wres())
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
        return rec

    def close(self):
        self.w.close()


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
                                cond=rec.get("cond")))
    assert sum(left.values()) == 0, who + (left,)
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
                      (sc.name, k, q, x, fr.BOUNDS[(CLASS, f32)][q], carried[q], bound[q]))
        assert all(r[q] <= 1.0 for q in s), who + (s, bound)
        # ---- d: the form ----
        sched = rec["schedule"]
        assert sched & FAST_FORMS == 0, who + (sched,)
        assert bool(sched & capi.SCHED_FRICTION) == (sc.mu is not None), who + (sched,)
        # (a world with a friction table takes the friction forms for a list of joints too; the problem, handed -1 for
        # every constraint, has friction off: the same bits, as checked above)
        if sc.warm and rec["prev"] is not None:
            assert sched & capi.SCHED_START, who + (sched,)
        if not sc.warm:
            assert not sched & capi.SCHED_START, who + (sched,)
        same = capi.SCHED_START | (0 if sc.mu is None or (pb["mu"] >= 0).any() else capi.SCHED_FRICTION)
        assert sched | same == pb["schedule"] | same, who + (sched, pb["schedule"])
    for q, x in r.items():
        worst[q] = max(worst.get(q, 0.0), x)
    return what


def report(name, worst):
    print("%s: worst ratio to bound: %s" % (name, " ".join("%s=%.3g" % kv for kv in sorted(worst.items()))))


SINGLES = [n for n in wc.NAMES if not n.startswith("BATCH")]


@pytest.mark.parametrize("name", SINGLES)
def test_one_ensemble_scenes(ctx, name):
    sc = wc.scene(name)
    run = Single(ctx, sc)
    worst, counts, seen, replanned = {}, [], set(), []
    try:
        for k in range(wc.STEPS):
            rec = run.step(k)
            what = check_step(ctx, sc, rec, worst)
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


@pytest.mark.parametrize("name", ["BATCH", "BATCH-step"])
def test_batch(ctx, name):
    """b, and a / c / d on each ensemble's own world; the rows of the ensemble that sits a step out are exactly 0."""
    sc = wc.scene(name)
    bw, off = wc.make_world(ctx, sc)
    singles = [Single(ctx, sc.single(e)) for e in range(len(sc.ens))]
    worst = {}
    sat = 0
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
            rows = lambda v, e, d=3: np.concatenate([v[d * jo[e]:d * jo[e + 1]], v[d * (mj + co[e]):d * (mj + co[e + 1])]])
            for e, s in enumerate(singles):
                body, con, lam = ensemble_view(bw, info, off, e)
                if dt[e] == 0.0:
                    sat += 1
                    for a, b in zip(body, before):
                        assert same_bits(a, b[off[e]:off[e + 1]]), (name, k, e, "an ensemble that sits out moved")
                    assert (rows(blocks[5], e) == 0.0).all() and not np.signbit(rows(blocks[5], e)).any(), (name, k, e)
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
    finally:
        bw.close()
        for s in singles:
            s.close()
    assert sat == (1 if sc.entry == "step_each" else 0)
    report(name, worst)


# ---- the dense step's refusals, with the other features on ------------------------------------------------------------------------
def snapshot(w):
    return w.bodies() + (w.lambda_(),) + w.contacts() + w.mass()


@pytest.mark.parametrize("why", ["pyramid", "free hinge"])
def test_dense_refusals_leave_everything_as_it_was(ctx, why):
    """DENSE's world after a sweep step: the dense step refuses the pyramid (no dense friction configured) and a hinge
    without a motor, by name, and bodies, lambda and the warm history keep every bit -- the next sweep step is, start and
    sources included, that of a world which never made the refused call."""
    sc = wc.build("DENSE", wc.SEEDS["DENSE"])
    if why == "free hinge":
        hinge = sc.ens[0]["kinds"] == jr.HINGE
        sc.ens[0]["motors"] = np.where(hinge[:, None], [0.0, -1.0], sc.ens[0]["motors"])
    worlds = [wc.make_world(ctx, sc)[0] for _ in range(2)]
    prm = capi.params(**sc.prm)
    try:
        for w in worlds:
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
            assert ("friction pyramid" if why == "pyramid" else "free hinge") in str(ei.value), str(ei.value)
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
