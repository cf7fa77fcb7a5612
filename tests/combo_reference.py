"""One world step with every feature on, composed from the references each feature already has (all imported
unchanged): what tests/test_gpu_world_combo.py holds the device to and tests/test_combo_reference_cpu.py the fp64 twins.

The step of one ensemble (tests/world_combo_cases.py: a Scene with one ensemble), from the state it reads:

  mass       live inertia: M^-1 and the gyroscopic torque of every body whose inertia is not a multiple of I_3, at the
             pose the step reads (model_reference.minv_reference / force_reference, which carry the tolerances;
             inertia_reference.reference states the same values and is held against them)
  contacts   collision_reference / sphere_reference on the list the code under test detected
  assembly   joint_reference.assemble_reference on the whole list, joints first (all four kinds)
  rhs        row by row: a joint's rows from joint_reference.rhs_reference (the motor's target on a driven axis row), a
             contact's from restitution_reference.rhs_reference; both extend model_reference.rhs_reference, so they
             agree on every row neither changes (asserted).  Bounds from joint_reference.motor_bounds.
  x0         warm start: a joint's rows are its own previous rows, a contact's those of the matched previous contact
             (warm_start_reference.match_contacts through test_gpu_world_warm.expected_start); no history: rhs
  lambda     friction_reference.sweeps_pyramid on the 50-digit A = J M^-1 J^T + cfm I from x0 (mu < 0 everywhere: the
             box form, sweep_reference.sweeps)
  v', p', R' model_reference.velocity_reference / position_reference

The scenes of world_combo_cases.PLUS_TABLE add four features, again from their own modules unchanged:

  contacts   capsule_twin / capsule_reference for a pair with a capsule (capsule_twin is sphere_twin on a list without one)
  assembly   slider_reference's twin and reference for a slider's rows, travel stop included; limit_reference's for the
             axis row of a hinge past a stop (err[2], its tolerance, the one-sided bounds; the motor leaves the row alone);
             every other row from joint_reference as before (the modules agree bit for bit on those: asserted)
  residual   a row pinned by lo == hi is in none of the residual's sums: check_solution
  rays       after the step, ray_twin and ray_reference on the poses it left

Every reference takes the exact fp64 values handed to the code under test, as its own module says: the lambda
reference the blocks and rhs that code assembled, the velocity reference its lambda.  So one wrong stage shows at that
stage and is not smeared over the ones that follow.

Guard bands (left_out): a decision that is a close call in fp64 is left out of the properties by the reference that
owns it -- the collision knife edges, restitution_reference.TIE, model_reference.BRANCH for contact normals and hinge
axes, the match radius of the warm start, the dense step's condition threshold.  The pyramid has none: its clamp is
continuous in both arguments (friction_reference).  The scenes are drawn so that every count is 0."""
import functools
import types

import mpmath as mp
import numpy as np

import capsule_reference as capref
import capsule_twin
import collision_reference as cref
import friction_port
import friction_reference as fr
import inertia_reference as ir
import joint_reference as jr
import limit_reference as lr
import live_inertia_cases as lic
import model_reference as mr
import ray_reference as rayref
import ray_twin
import restitution_reference as rr
import slider_reference as sr
import sphere_reference as sref
import sphere_twin
import sweep_reference as sw
import warm_start_reference as wsr
import world_combo_cases as wc
from helpers import dense_numpy
from oracle import oracle as orc

U32 = 2.0 ** -24
DENSE_COND = 1e7


# ---- the list, the tables ------------------------------------------------------------------------------------------------------
def joints_of(e):
    """(kind, body0, body1, data, motor) of an ensemble's joints in local indices; empty arrays where it has none."""
    if e["joints"] is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)), np.zeros((0, 2))
    b0, b1, data = e["joints"]
    m = len(b0)
    kind = e["kinds"] if e["kinds"] is not None else np.zeros(m, np.int32)
    motor = e["motors"] if e["motors"] is not None else np.tile([0.0, -1.0], (m, 1))
    return kind.astype(np.int32), b0.astype(np.int32), b1.astype(np.int32), np.asarray(data, np.float64), np.asarray(motor, np.float64)


def full_case(sc, state, mass, contacts, dt, erp):
    """The list a world step solves -- joints first, then the contacts -- as a model_reference case, with the
    per-constraint tables the world must have filled in: (case, motor, mu, rest, hinge limits [m][8], travel stops
    [m][2]), tables None where the scene never sets them.  A contact's rows of the two stop tables are zeros (no stop)
    and (-inf, +inf)."""
    e = sc.ens[0]
    kind, b0, b1, data, motor = joints_of(e)
    c0, c1, cd = contacts
    mj, mc = len(b0), len(c0)
    case = dict(p=np.asarray(state[0]), R=np.asarray(state[1]), v=np.asarray(state[2]), w=np.asarray(state[3]),
                Minv=np.asarray(mass[0]).reshape(-1, 36), f_ext=np.asarray(mass[1]).reshape(-1, 6),
                kind=np.concatenate([kind, np.ones(mc, np.int32)]).astype(np.int32),
                body0=np.concatenate([b0, c0]).astype(np.int32), body1=np.concatenate([b1, c1]).astype(np.int32),
                data=np.concatenate([data, np.asarray(cd, np.float64).reshape(-1, 7)]), dt=float(dt), erp=float(erp))
    table = lambda t: None if t is None else np.concatenate([np.full(mj, -1.0), np.full(mc, float(t[0]))])
    full_motor = np.concatenate([motor, np.tile([0.0, -1.0], (mc, 1))]) if sc.kinds and mj else None
    lim = np.concatenate([e["limits"], np.zeros((mc, 8))]) if sc.limits and e.get("limits") is not None else None
    travel = np.concatenate([e["travel"], np.tile([-np.inf, np.inf], (mc, 1))]) if sc.travel and e.get("travel") is not None else None
    return case, full_motor, table(sc.mu), table(sc.rest), lim, travel


class _Listed:
    """What test_gpu_world_warm.expected_start asks of a world: the list its last step solved."""

    def __init__(self, contacts):
        self._c = contacts

    def contacts(self):
        return self._c


def expected_x0(prev, contacts, mj, rhs):
    """x0 [3m] and its sources [m] for the list (joints first) of a warm step.  prev = (contacts b0, b1, data, lambda
    [3 (mj + old contacts)]) of the step before, or None: no history."""
    from test_gpu_world_warm import expected_start
    assert wc.RADIUS == 0.01      # expected_start's radius
    return expected_start(prev, _Listed(contacts), mj=mj, rhs=rhs)


def flat(case, J0, J1, is_eq, lo, hi):
    m = case["kind"].shape[0]
    return types.SimpleNamespace(n=case["p"].shape[0], m=m, Minv=case["Minv"], body0=case["body0"], body1=case["body1"],
                                 J0=np.asarray(J0).reshape(m, 18), J1=np.asarray(J1).reshape(m, 18), is_eq=np.asarray(is_eq),
                                 lo=np.asarray(lo), hi=np.asarray(hi))


# ---- the fp64 twin of the step ------------------------------------------------------------------------------------------------
def twin_mass(sc, state, mass):
    e = sc.ens[0]
    if not sc.live:
        return np.asarray(mass[0]).reshape(-1, 36), np.asarray(mass[1]).reshape(-1, 6)
    return lic.host_mass(state[1], state[3], e["mass"], e["I_body"], mass[0], mass[1])


def twin_detect(sc, state):
    e = sc.ens[0]
    shape = e["shape"] if sc.shapes else np.zeros(len(e["shape"]), np.int32)
    if sc.capsules:
        if not (shape == wc.CAPSULE).any():      # on a list without capsules the capsule twin is the sphere twin
            a, b = capsule_twin.contacts(state[0], state[1], e["side"], shape), sphere_twin.contacts(state[0], state[1], e["side"], shape)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        return capsule_twin.contacts(state[0], state[1], e["side"], shape)
    return sphere_twin.contacts(state[0], state[1], e["side"], shape)


def twin_assemble(sc, state, mass, contacts, dt, erp):
    """The system of the step in fp64: joint_reference's twin for the blocks and the joints' rows, restitution_reference's
    for the contacts' rows.  Returns (case, tables, dict J0, J1, err, lo, hi, is_eq, rhs, what, margin)."""
    case, motor, mu, rest, lim, travel = full_case(sc, state, mass, contacts, dt, erp)
    if (case["kind"] == sr.SLIDER).any() or lim is not None:
        # slider_reference's twin takes the sliders' rows and hands the others to limit_reference's, which takes the stopped
        # hinges' axis rows and hands the others to joint_reference's
        tw = sr.twin_assemble(case, motor, travel, hinge_lim=lim if lim is not None else np.zeros((case["kind"].shape[0], 8)))
        old, sub = sr._others(case)
        plain = jr.twin_assemble(sub, None if motor is None else motor[old])
        for i, k in enumerate(old):      # the three modules agree bit for bit on every row that none of them changes
            rows = slice(3 * k, 3 * k + (2 if tw["active"][k] else 3))
            for name in ("err", "lo", "hi", "rhs"):
                assert jr.bits_equal(tw[name][rows], plain[name][3 * i:3 * i + rows.stop - rows.start]), (k, name)
            assert jr.bits_equal(tw["J0"][k], plain["J0"][i]) and jr.bits_equal(tw["J1"][k], plain["J1"][i])
    else:
        tw = jr.twin_assemble(case, motor)
        tw["active"] = np.zeros(case["kind"].shape[0], np.int32)
    rhs_c, what, margin = rr.twin_rhs(case, tw["J0"], tw["J1"], tw["err"], rest, sc.vth)
    contact = np.repeat(case["kind"] == jr.CONTACT, 3)
    ball = np.repeat(case["kind"] == jr.BALL, 3)
    assert np.array_equal(rhs_c[ball], tw["rhs"][ball])      # both twins restate the same rows
    tw["rhs"] = np.where(contact, rhs_c, tw["rhs"])
    tw.update(what=what, margin=margin, lim=lim, travel=travel)
    return case, (motor, mu, rest), tw


def twin_step(sc, state, mass, prev, dt, erp, dense=False):
    """One step of a one-ensemble scene in fp64, stage by stage as the world takes it.  state = (p, R, v, w), mass =
    (Minv, f_ext) as held before the step, prev the history of expected_x0.  Returns the record of the step."""
    e = sc.ens[0]
    Minv, f_ext = twin_mass(sc, state, mass)
    contacts = twin_detect(sc, state)
    case, (motor, mu, rest), tw = twin_assemble(sc, state, (Minv, f_ext), contacts, dt, erp)
    m, mj = case["kind"].shape[0], len(joints_of(e)[0])
    s = flat(case, tw["J0"], tw["J1"], tw["is_eq"], tw["lo"], tw["hi"])
    rec = dict(state=state, mass_in=mass, mass=(Minv, f_ext), contacts=contacts, case=case, motor=motor, mu=mu, rest=rest,
               tw=tw, what=tw["what"], margin=tw["margin"], lim=tw["lim"], travel=tw["travel"], prev=prev, dt=dt, erp=erp, dense=dense, x0=None, src=None, cond=None)
    muf = np.full(m, -1.0) if mu is None else mu
    if dense:
        A0 = dense_numpy(s, 0.0)[0]
        rec["cond"] = np.linalg.cond(A0) if m else 0.0
        rec["cfm"] = wc.CFM if rec["cond"] >= DENSE_COND else 0.0
        ok, lam, _, _ = orc.mixed_constraints(A0 + rec["cfm"] * np.eye(3 * m), tw["rhs"], tw["is_eq"], tw["lo"], tw["hi"], 1)
        assert ok
    else:
        if sc.warm and m:
            rec["x0"], rec["src"] = expected_x0(prev, contacts, mj, tw["rhs"])
        p = sc.prm
        lam, acc, wres, res = friction_port.sweeps(s, tw["rhs"], p["cfm"], muf, p["method"], p["omega"], p["max_iters"], False, rec["x0"])
        pinned = pinned_rows(tw["is_eq"], tw["lo"], tw["hi"])
        if pinned.any():      # the port's residual is the rule from before pinned rows: they are in none of the sums
            res = friction_port.residual(lam, np.where(pinned, 0.0, wres), tw["is_eq"], tw["lo"], tw["hi"], muf)
        rec.update(acc=acc, wres=wres, res=res)
    v6 = orc.velocity_update(state[2], state[3], Minv, f_ext, case["body0"], case["body1"], tw["J0"], tw["J1"], lam, dt)
    p1, R1 = orc.position_update(state[0], state[1], np.concatenate([state[2], state[3]], axis=1), v6, dt)
    rec.update(lam=lam, v6=v6, after=(p1, R1, v6[:, :3].copy(), v6[:, 3:].copy()))
    if sc.rays:
        rec["rays"] = twin_rays(sc, rec["after"])
    rec["left_out"] = left_out(sc, rec)
    return rec


def twin_run(sc):
    """The scene's steps through the twin: a list of records, one per step (an ensemble that sits a step out leaves a
    record with dt 0 and nothing else)."""
    assert len(sc.ens) == 1
    e = sc.ens[0]
    state, mass, prev = (e["p"], e["R"], e["v"], e["w"]), (e["Minv"], e["f_ext"]), None
    out = []
    for k, (dt, erp) in enumerate(sc.rates):
        if dt[0] == 0.0:
            out.append(dict(dt=0.0, left_out={}, contacts=twin_detect(sc, state), src=None, what=[],
                            rays=twin_rays(sc, state) if sc.rays else None))
            continue
        dense = sc.entry == "dense" and k % 2 == 1
        rec = twin_step(sc, state, mass, prev if sc.warm else None, dt[0], erp[0], dense)
        state, mass = rec["after"], rec["mass"]
        prev = rec["contacts"] + (rec["lam"],)
        out.append(rec)
    return out


# ---- what the references leave out --------------------------------------------------------------------------------------------
def collision_left_out(sc, state, contacts):
    """Holds the contact list to collision_reference (boxes) and sphere_reference (pairs with a sphere) and returns how
    many bodies, pairs and contacts their guard bands left out of a property."""
    e = sc.ens[0]
    p, R, side = np.asarray(state[0]), np.asarray(state[1]), e["side"]
    shape = e["shape"] if sc.shapes else np.zeros(len(e["shape"]), np.int32)
    n = p.shape[0]
    b0, b1, data = contacts
    rows = {}
    for k in range(len(b0)):
        rows.setdefault((int(b0[k]), int(b1[k])), []).append(np.asarray(data[k]))
    tally, balls = cref.Tally(), {}
    radius = np.where(shape == wc.SPHERE, 0.5 * side[:, 0], np.where(shape == wc.CAPSULE, 0.5 * side[:, 2], 0.5 * np.linalg.norm(side, axis=1)))
    for b in range(n):
        got = rows.pop((-1, b), [])
        if shape[b] == wc.CAPSULE:
            capref.compare(capref.capsule_ground(p[b], R[b], side[b]), got, balls, ground=True)
        elif shape[b] == wc.SPHERE:
            g = sref.sphere_ground(p[b], side[b][0])
            g["guard_n"] = False
            sref.compare(g, got, balls)
        else:
            cref.check_ground(cref.ground_reference(p[b], R[b], side[b]), np.array(got).reshape(-1, 7), tally, "ground %d" % b)
    for i in range(n):
        for j in range(i + 1, n):
            got = rows.pop((i, j), [])
            if np.linalg.norm(p[i] - p[j]) > (radius[i] + radius[j]) * (1 + 1e-9):
                assert not got, "contacts between bodies %d and %d, whose bounding spheres are apart" % (i, j)
            elif shape[i] == wc.CAPSULE or shape[j] == wc.CAPSULE:
                capref.compare(capref.pair(p, R, side, shape, i, j), got, balls)
            elif shape[i] == wc.SPHERE or shape[j] == wc.SPHERE:
                sref.compare(sref.pair(p, R, side, shape, i, j), got, balls)
            else:
                cref.check_pair(cref.PairRef(p[i], R[i], side[i], p[j], R[j], side[j]), np.array(got).reshape(-1, 7), tally, "pair %d %d" % (i, j))
    assert not rows, "contacts of unknown pairs: %s" % sorted(rows)
    return tally.excluded + tally.bodies_excluded + tally.contacts_excluded + sum(balls.values())


def left_out(sc, rec):
    """{what: count} of everything a guard band leaves out of a property in this step: every value must be 0."""
    case = rec["case"]
    out = dict(collision=collision_left_out(sc, rec["state"], rec["contacts"]))
    out["restitution"] = sum(1 for a, b in rec["margin"] if min(a, b) < rr.TIE)
    branch = 0
    with mp.workdps(mr.DPS):
        R = [mr._m3(x) for x in case["R"]]
        for i in range(case["kind"].shape[0]):
            d = mr._v(case["data"][i])
            if case["kind"][i] == jr.CONTACT:
                axis = d[3:6]
            elif case["kind"][i] == jr.HINGE:
                axis = mr._mv(R[int(case["body0"][i])], d[0:3])
            else:
                continue
            branch += int(mr.align_to_z(axis)[2] < 10 * mr.BRANCH)
    out["branch"] = branch
    warm = 0
    if rec["prev"] is not None and rec["src"] is not None:
        c0, c1, cd = rec["contacts"]
        o0, o1, od = rec["prev"][:3]
        r2 = wc.RADIUS ** 2
        for c in range(len(c0)):
            d2 = sorted(float(np.sum((cd[c, :3] - od[o, :3]) ** 2)) for o in range(len(o0)) if o0[o] == c0[c] and o1[o] == c1[c])
            warm += int(any(abs(x - r2) < 1e-9 * r2 for x in d2) or (len(d2) > 1 and d2[0] <= r2 and d2[1] - d2[0] < 1e-9 * r2))
    out["warm"] = warm
    out["dense"] = int(rec["cond"] is not None and DENSE_COND / 10 < rec["cond"] < DENSE_COND * 10)
    if sc.limits or sc.travel:
        _, dist = stop_reference(case, rec.get("lim"), rec.get("travel"))
        out["limit"] = sum(1 for i, d in enumerate(dist) if d is not None and case["kind"][i] == jr.HINGE and d <= lr.MARGIN)
        out["travel"] = sum(1 for i, d in enumerate(dist) if d is not None and case["kind"][i] == sr.SLIDER and d <= sr.MARGIN)
    if sc.rays and rec.get("after") is not None:
        out["rays"] = sum(1 for r in reference_rays(sc, rec["after"]) if r[0] is None)
    return out


# ---- stops and rays -----------------------------------------------------------------------------------------------------------
def stop_reference(case, lim, travel):
    """Per constraint, by the references' own decisions (atan2 for a hinge, the 50-digit travel for a slider): (active
    [m]: +1 upper, -1 lower, 0; the distance from the nearest stop set, in tan(theta / 2) or in metres, None where no
    table applies)."""
    m = case["kind"].shape[0]
    active, dist = np.zeros(m, np.int32), [None] * m
    if lim is not None:
        with mp.workdps(mr.DPS):
            for i, r in enumerate(lr.case_reference(case, lim)):
                if r is not None:
                    active[i], dist[i] = r[0], float(r[3])
    if travel is not None:
        with mp.workdps(mr.DPS):
            p, R = [mr._v(x) for x in case["p"]], [mr._m3(x) for x in case["R"]]
            for i in np.nonzero(case["kind"] == sr.SLIDER)[0]:
                d, b1 = mr._v(case["data"][i]), int(case["body1"][i])
                ref = sr.slider_reference(p[int(case["body0"][i])], R[int(case["body0"][i])], p[b1] if b1 >= 0 else None, d[0:3], d[3:6])
                act, _, _, ds = sr.stop_reference(ref["x"], ref["dx"], float(travel[i][0]), float(travel[i][1]))
                assert ref["dx"] < sr.MARGIN
                active[i], dist[i] = act, (float(ds) if ds != mp.inf else None)
    return active, dist


def _rays_of(sc, state):
    """The ensemble's rays in the world frame at the pose given: (origins, directions, tmax, carrier)."""
    r = sc.ens[0]["rays"]
    o, d = [], []
    for k in range(len(r["body"])):
        b = int(r["body"][k])
        ow, dw = (r["origin"][k], r["dir"][k]) if b < 0 else ray_twin.world_frame(state[0][b], state[1][b], r["origin"][k], r["dir"][k])
        o.append(ow); d.append(dw)
    return np.array(o, np.float64), np.array(d, np.float64), r["tmax"], r["body"]


def twin_rays(sc, state):
    """(hit_body, t, normal) of the ensemble's ray table against the state given, by ray_twin."""
    e = sc.ens[0]
    r = e["rays"]
    shape = e["shape"] if sc.shapes else None
    return ray_twin.cast(state[0], state[1], e["side"], shape, r["origin"], r["dir"], r["tmax"], r["body"])


@functools.lru_cache(maxsize=256)
def _reference_rays(key):
    pos, R, side, shape, o, d, tmax, body = (np.frombuffer(b, t).reshape(s) for b, t, s in key)
    return [rayref.cast_one(pos, R, side, shape, o[k], d[k], tmax[k], int(body[k])) for k in range(len(body))]


def reference_rays(sc, state):
    """[(kind, body, t, normal)] per ray by ray_reference, on the world-frame rays the twin's fp64 frame change gives (a
    carried ray's origin and direction are inputs of the reference, as every ray's are; the frame change itself is held
    to 50 digits by frame_change_error).  Cached by the bits of its
    inputs: the CPU test and left_out ask for the same casts."""
    e = sc.ens[0]
    o, d, tmax, body = _rays_of(sc, state)
    shape = e["shape"] if sc.shapes else np.zeros(len(e["shape"]), np.int32)
    arrs = (np.asarray(state[0], np.float64), np.asarray(state[1], np.float64), e["side"], shape, o, d, tmax, body)
    return _reference_rays(tuple((np.ascontiguousarray(a).tobytes(), a.dtype.str, a.shape) for a in arrs))


def frame_change_error(sc, state, o, d):
    """The fp64 frame change of the carried rays (ray_twin.world_frame, which the device mirrors bit for bit) against
    o_w = c + R o, d_w = R d at 50 digits: the worst error over its tolerance, 5u of the magnitude sum per component (a
    three-term product sum, one addition for the origin).  ray_reference rounds its inputs to fp64, so it is handed the
    fp64 world-frame ray; this is the independent check of the step before it."""
    r = sc.ens[0]["rays"]
    worst = 0.0
    with mp.workdps(rayref.DPS):
        for k in range(len(r["body"])):
            b = int(r["body"][k])
            if b < 0:
                continue
            c, R = mr._v(state[0][b]), mr._m3(state[1][b])
            lo, ld = mr._v(r["origin"][k]), mr._v(r["dir"][k])
            for j in range(3):
                for base, loc, got in ((c[j], lo, o[k][j]), (mp.mpf(0), ld, d[k][j])):
                    want = base + sum(R[j][i] * loc[i] for i in range(3))
                    mag = abs(base) + sum(abs(R[j][i] * loc[i]) for i in range(3))
                    if mag > 0:
                        worst = max(worst, float(abs(mp.mpf(float(got)) - want) / (5 * mr.U * mag)))
                    else:
                        assert float(got) == 0.0
    return worst


def check_rays(sc, state, got):
    """got = (hit_body, t, normal) against reference_rays: the body of every decided ray; t |d| and the normal within
    ray_reference's bound for scenes of a metre or two (collision_reference.TOL).  Returns the worst error / bound."""
    hit, t, normal = got
    o, d, tmax, body = _rays_of(sc, state)
    assert frame_change_error(sc, state, o, d) <= 1.0
    worst = 0.0
    with mp.workdps(rayref.DPS):
        for k, (kind, rb, rt, rn) in enumerate(reference_rays(sc, state)):
            if kind is None:
                continue
            assert int(hit[k]) == rb, ("ray %d: body %d, the reference says %s %d" % (k, hit[k], kind, rb))
            if kind != "hit":
                assert t[k] == (0.0 if kind == "inside" else tmax[k]) and not normal[k].any(), (k, kind, t[k])
                continue
            dn = mp.sqrt(sum(mp.mpf(float(x)) ** 2 for x in d[k]))
            err = max([abs(mp.mpf(float(t[k])) - rt) * dn] + [abs(mp.mpf(float(normal[k][j])) - rn[j]) for j in range(3)])
            worst = max(worst, float(err / rayref.TOL))
    return worst


# ---- the composed reference -----------------------------------------------------------------------------------------------------
def mass_reference(sc, state):
    """(M^-1 [36 n], f [6 n]) as Checked at the pose given, and the bodies the live refresh touches."""
    e = sc.ens[0]
    live = ~lic.is_skipped(e["I_body"])
    return mr.minv_reference(state[1], e["mass"], e["I_body"]), mr.force_reference(state[1], state[3], e["mass"], e["I_body"]), live


def mass_entries(live):
    """Flat indices of what the refresh writes: the angular 3 x 3 of M^-1 and the torque rows of f."""
    M = [36 * b + 6 * (3 + k) + 3 + j for b in np.nonzero(live)[0] for k in range(3) for j in range(3)]
    f = [6 * b + 3 + k for b in np.nonzero(live)[0] for k in range(3)]
    return M, f


def inertia_agrees(sc, state):
    """inertia_reference.reference against model_reference's values, body by body: the largest difference."""
    e = sc.ens[0]
    M, f, live = mass_reference(sc, state)
    worst = mp.mpf(0)
    for b in np.nonzero(live)[0]:
        inv, tq, _ = ir.reference(state[1][b], e["I_body"][b], state[3][b])
        with mp.workdps(40):
            for k in range(3):
                worst = max(worst, abs(tq[k] - f.val[6 * b + 3 + k]))
                for j in range(3):
                    worst = max(worst, abs(inv[k, j] - M.val[36 * b + 6 * (3 + k) + 3 + j]))
    return float(worst)


def rhs_reference(case, asm, motor, rest, vth):
    """The composed rhs as Checked, the restitution decisions, and (lo, hi) with the motors' limits.  An asm of
    stops_assembly_reference (it has `active`) takes the joints' rows and the bounds from slider_reference, which leaves
    the motor off a row whose stop is active."""
    if "active" in asm:
        idle = motor
        if motor is not None:      # the motor leaves an active hinge stop's row alone, as it does a slider's
            idle = motor.copy()
            idle[(asm["active"] != 0) & (case["kind"] == jr.HINGE)] = (0.0, -1.0)
        rj = sr.rhs_reference(case, asm, idle)
    else:
        rj = jr.rhs_reference(case, asm, motor)
    rc, what = rr.rhs_reference(case, asm, rest, vth)
    m = case["kind"].shape[0]
    out = mr.Checked(3 * m)
    for i in range(m):
        src = rc if case["kind"][i] == jr.CONTACT else rj
        for k in range(3 * i, 3 * i + 3):
            if case["kind"][i] == jr.BALL:      # neither reference changes a ball joint's rows
                assert rj.val[k] == rc.val[k] and rj.tol[k] == rc.tol[k]
            out.put(k, src.val[k], src.mag[k], src.tol[k])
    return out, what, (sr.bounds_reference(case, asm, idle) if "active" in asm else jr.motor_bounds(case, asm, motor))


def rhs_each_reference(cases, asms, motors, rests, vth):
    """The _each form: one (case, asm, motor, rest) per ensemble with its own dt / erp in the case, rows concatenated;
    an ensemble whose dt is 0 sits out and its rows are exactly 0 (value 0, tolerance 0)."""
    parts = []
    for case, asm, motor, rest in zip(cases, asms, motors, rests):
        if case["dt"] == 0.0:
            parts.append(mr.Checked(3 * case["kind"].shape[0]))
        else:
            parts.append(rhs_reference(case, asm, motor, rest, vth)[0])
    out = mr.Checked(0)
    for c in parts:
        out.val, out.mag, out.tol = out.val + c.val, out.mag + c.mag, out.tol + c.tol
    return out


def stops_assembly_reference(case, lim, travel):
    """The assembly of a list that may hold sliders and stopped hinges: slider_reference.assemble_reference (the sliders
    from it with an active travel stop in place, every other row from joint_reference), then on a hinge whose stop
    limit_reference finds active, err[2] with its tolerance and the one-sided bounds."""
    asm = sr.assemble_reference(case, travel)
    if lim is not None:
        with mp.workdps(mr.DPS):
            for i, r in enumerate(lr.case_reference(case, lim)):
                if r is None or not r[0]:
                    continue
                act, err, tol = r[0], r[1], r[2]
                asm["active"][i] = act
                asm["err"].put(3 * i + 2, err, abs(err), tol)
                asm["lo"][3 * i + 2], asm["hi"][3 * i + 2] = (-np.inf, 0.0) if act > 0 else (0.0, np.inf)
    return asm


def assembly_reference(sc, state, mass, contacts, dt, erp):
    case, motor, mu, rest, lim, travel = full_case(sc, state, mass, contacts, dt, erp)
    if (case["kind"] == sr.SLIDER).any() or lim is not None:
        asm = stops_assembly_reference(case, lim, travel)
    else:
        asm = jr.assemble_reference(case)
    rhs, what, (lo, hi) = rhs_reference(case, asm, motor, rest, sc.vth)
    return dict(case=case, motor=motor, mu=mu, rest=rest, lim=lim, travel=travel, asm=asm, rhs=rhs, what=what, lo=lo, hi=hi)


def worst(checked, got, f32=False, rows=None):
    """Checked.worst; for an fp32 problem the device assembles in fp64 and rounds once to fp32 (tests/test_gpu_joints.py:
    'in fp32 after the cast'), so the tolerance gains 2^-24 |value|."""
    if not f32:
        return checked.worst(got, rows)[0]
    wide = mr.Checked(len(checked.val))
    with mp.workdps(mr.DPS):
        for k in range(len(checked.val)):
            wide.put(k, checked.val[k], checked.mag[k], checked.tol[k] + U32 * abs(checked.val[k]))
    return wide.worst(got, rows)[0]


def check_assembly(ref, blocks, f32=False):
    """blocks = (J0, J1, is_eq, lo, hi, rhs, err) of the code under test against assembly_reference: ratios to the
    tolerances; the row types and bounds bit for bit."""
    J0, J1, is_eq, lo, hi, rhs, err = blocks
    asm = ref["asm"]
    assert not asm["branch"].any()
    assert np.array_equal(is_eq, asm["is_eq"]), "row types"
    held = lambda a: sw.held(a, f32)
    assert np.array_equal(lo, held(ref["lo"])) and np.array_equal(hi, held(ref["hi"])), "bounds"
    return {"J": max(worst(asm["J0"], J0, f32), worst(asm["J1"], J1, f32)), "err": worst(asm["err"], err, False),
            "rhs": worst(ref["rhs"], rhs, f32)}


def lambda_reference(sc, case, blocks, mu, x0):
    """The 50-digit sweeps on the system the code under test assembled, from x0 (None: rhs): (System, lambda)."""
    J0, J1, is_eq, lo, hi, rhs, _ = blocks
    s = flat(case, J0, J1, is_eq, lo, hi)
    p = sc.prm
    A = sw.system(s, p["cfm"], sc.f32)
    muf = np.full(s.m, -1.0) if mu is None else mu
    return A, muf, fr.sweeps_pyramid(A, rhs, is_eq, lo, hi, muf, p["method"], p["omega"], p["max_iters"], x0)


def check_solution(A, muf, blocks, x_ref, lam, acc=None, wres=None, res=None):
    """friction_reference.measure: {x, a, w, r} ratios in units of u max(1, |ref|) etc. (sweep_reference)."""
    _, _, is_eq, lo, hi, rhs, _ = blocks
    out = fr.measure(A, rhs, is_eq, lo, hi, muf, x_ref, lam, acc, wres, res)
    pinned = pinned_rows(is_eq, lo, hi)
    if res is not None and pinned.any():
        # a row pinned by lo == hi violates nothing whatever the sign of its w, and the residual
        # kernels leave it out of all four sums.  friction_reference's rule is the one from before pinned rows existed, so
        # it is handed w = 0 on them, which puts a row in none of its sums, and no magnitude for them either.
        with mp.workdps(sw.DPS):
            w, mag = sw.wres(A, rhs, lam)
            w = [mp.mpf(0) if pinned[r] else w[r] for r in range(len(w))]
            mag = [mp.mpf(0) if pinned[r] else mag[r] for r in range(len(mag))]
            want, scale = fr.residual_pyramid(A, rhs, lam, is_eq, lo, hi, muf, w=(w, mag))
        out["r"] = sw.err_scalar(res, want, scale, A.f32)
    return out


def pinned_rows(is_eq, lo, hi):
    """[3m] bool: the inequality rows with lo == hi (a free hinge's axis row, a free slider's rail row)."""
    return (np.asarray(is_eq) == 0) & (np.asarray(lo) == np.asarray(hi))


def carried_sweeps(s, rhs, cfm, mu, method, omega, K, x0=None, f32=False):
    """The sweeps of friction_port in the form the kernels (and oracle/pgs_fast.inc) run them: per-body accumulators
    a_b = M_b^-1 sum J^T x, formed once from the start and then CARRIED -- every row reads A x from them and adds its
    change to them -- and w = J a + cfm x - rhs taken from the carried accumulators in the epilogue.  Plain numpy in the
    working precision, Gauss-Seidel / backward SOR; not the device's operation order.  It exists to measure what carrying
    costs: where x comes back to 0 after large iterates (a contact that lets go under the pyramid, a start = rhs far
    from the solution) the accumulators keep rounding noise of the size of those iterates, which the bounds of
    sweep_reference, stated at the final x, do not see.  Returns x, a [6n], w."""
    T = np.float32 if f32 else np.float64
    m, n = s.m, s.n
    W = sw.held(s.Minv, f32).reshape(n, 6, 6).astype(T)
    J = [sw.held(s.J0, f32).reshape(m, 3, 6).astype(T), sw.held(s.J1, f32).reshape(m, 3, 6).astype(T)]
    body = [np.asarray(s.body0), np.asarray(s.body1)]
    b = np.asarray(rhs).astype(T)
    x = (b if x0 is None else np.asarray(x0).astype(T)).copy()
    lo, hi, cfm = np.asarray(s.lo).astype(T), np.asarray(s.hi).astype(T), T(cfm)
    sides = [[sd for sd in range(2) if body[sd][i] >= 0] for i in range(m)]
    B = {(i, sd): (W[body[sd][i]] @ J[sd][i].T).T for i in range(m) for sd in sides[i]}      # rows of (M^-1 J^T)^T
    a = np.zeros((n, 6), T)
    D = np.full(3 * m, cfm, T)
    for i in range(m):
        for sd in sides[i]:
            a[body[sd][i]] += W[body[sd][i]] @ (J[sd][i].T @ x[3 * i:3 * i + 3])
            for q in range(3):
                D[3 * i + q] += J[sd][i][q] @ B[i, sd][q]
    k = T(1) / T(omega) if method == sw.SOR else T(1)
    order = range(3 * m - 1, -1, -1) if method == sw.SOR else range(3 * m)
    row = lambda i, q: cfm * x[3 * i + q] + sum(J[sd][i][q] @ a[body[sd][i]] for sd in sides[i])
    assert method != sw.JACOBI
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(K):
            for r in order:
                i, q = divmod(r, 3)
                t = x[r] + (b[r] - row(i, q)) / (k * D[r])
                if q < 2 and mu[i] >= 0:
                    xn = x[3 * i + 2]
                    bd = T(mu[i]) * xn if xn > 0 else T(0)
                    t = min(max(t, -bd), bd)
                elif not s.is_eq[r]:
                    t = min(max(t, lo[r]), hi[r])
                dx = t - x[r]
                x[r] = t
                for sd in sides[i]:
                    a[body[sd][i]] += B[i, sd][q] * dx
        w = np.array([row(i, q) - b[3 * i + q] for i in range(m) for q in range(3)], T)
    return x.astype(np.float64), a.reshape(-1).astype(np.float64), w.astype(np.float64)


@functools.lru_cache(maxsize=None)
def carried_worst(name, e=0):
    """{x, a, w}: the worst of check_solution's ratios for carried_sweeps over the sweep steps of the twin's run of
    ensemble e of a named scene, in the scene's precision -- the CPU measurement behind a bound that sweep_reference's
    classes do not give (4 x this, where that exceeds the class constant).  Once per process."""
    sc0 = wc.scene(name)
    sc = sc0.single(e) if len(sc0.ens) > 1 else sc0
    out = {}
    for rec in twin_runs(name)[e]:
        if rec["dt"] == 0.0 or rec["dense"]:
            continue
        tw, p = rec["tw"], sc.prm
        blocks = (tw["J0"], tw["J1"], tw["is_eq"], tw["lo"], tw["hi"], tw["rhs"], tw["err"])
        A, muf, x_ref = lambda_reference(sc, rec["case"], blocks, rec["mu"], rec["x0"])
        got = carried_sweeps(flat(rec["case"], *blocks[:5]), tw["rhs"], p["cfm"], muf, p["method"], p["omega"], p["max_iters"], rec["x0"], sc.f32)
        for q, x in check_solution(A, muf, blocks, x_ref, *got).items():
            out[q] = max(out.get(q, 0.0), x)
    return out


CARRY_ROOM = 4.0      # a kernel may order a sum differently from the twin


def solution_bounds(cls, f32, carried):
    """The bound of each quantity: friction_reference.BOUNDS of the class, or CARRY_ROOM x the carried twin's own ratio
    where that is larger."""
    return {q: max(float(c), CARRY_ROOM * carried.get(q, 0.0)) for q, c in fr.BOUNDS[(cls, f32)].items()}


def check_motion(case, asm, lam, v6, after, scale=1.0):
    """v' against model_reference.velocity_reference (the reference's J, the given lambda) in units of the bound of
    tests/test_gpu_model_reference.py, 1e-12 max(1, |v'|); p' and R' against position_reference (ratios to tolerance)."""
    m = case["kind"].shape[0]
    vr = mr.velocity_reference(case, asm["J0"].array().reshape(m, 18), asm["J1"].array().reshape(m, 18), lam).array()
    bound = scale * 1e-12 * max(1.0, np.abs(vr).max())
    v6_old = np.concatenate([case["v"], case["w"]], axis=1)
    P, Q = mr.position_reference(case["p"], case["R"], v6_old, np.asarray(v6).reshape(-1, 6), case["dt"])
    return {"v": float(np.abs(np.asarray(v6).reshape(-1) - vr).max() / bound), "p": P.worst(after[0])[0], "R": Q.worst(after[1])[0]}


@functools.lru_cache(maxsize=None)
def twin_runs(name):
    """The twin's records of a named scene, ensemble by ensemble: computed once per process."""
    sc = wc.scene(name)
    return [twin_run(sc.single(e) if len(sc.ens) > 1 else sc) for e in range(len(sc.ens))]
