"""Capsule contact geometry as mathematics, in mpmath at 50 digits on the exact fp64 inputs: an INDEPENDENT reference
for what tests/capsule_twin.py restates in fp64 and collide.hip mirrors bit for bit.  Nothing here follows the device's
operation order; the balls go through the sphere_* functions of sphere_reference.py.

A capsule is (centre c, row-major R, side row (d, d, l)): r = d / 2, half axis e = (l - d) / 2, axis u = column 2 of R,
the ball at t = the sphere of diameter d centred at c + t u, t in [-e, e]; end 0 is t = -e, end 1 is t = +e.

  ground    the sphere rule on the ball at end 0, then at end 1
  sphere    t = clamp((c_S - c) . u, -e, e); the sphere - sphere rule between the ball at t and the sphere
  capsules  end 0 of i, end 1 of i against j; end 0 of j, end 1 of j against i (each the capsule - sphere rule); then the
            interior pair at the common-perpendicular parameters (s, t) of the axes, which exists only strictly inside
            both segments and for non-parallel axes
  box       dist(t) = distance from c + t u to the box; end 0, end 1, then t* = the lowest minimiser of dist on [-e, e],
            counted only strictly inside; if the axis enters the box, the midpoint of the stretch inside.  dist^2 is a
            convex piecewise quadratic: its minimisers are found among the ends, the breakpoints and the pieces'
            stationary points, exactly.  (tests/test_capsule_reference_cpu.py checks that method against a plain
            ternary search on dist, which knows nothing of breakpoints or pieces.)
  flat rule the interior candidate is dropped if an EMITTED end candidate's centre distance (box: dist) is within 1e-9
            of its own.
  pruning   the kernel's own: a contact within 1e-6 of an earlier contact of the same pair is deleted.

Guard bands.  Every decision is three-valued (yes, no, close call); a candidate whose presence is a close call is
matched if the code reports it and skipped if not, and the case is COUNTED as left out of that property:
  decision  |s| < 1e-9 for contact / no contact (1e-12 on the ground); a pruning distance within [0.5e-6, 2e-6]
  interior  a parameter of the interior candidate within 1e-9 e of an end of its segment; the flat rule when
            (end distance - interior distance) lies in [1e-10, 1e-8]; axes whose sin^2 is below 1e-24 but not 0
  normal    L < 1e-9 (normal, and the position that rides on it); inside a box, the two smallest g_k within 1e-9, or
            |p_k| < 1e-9 on the chosen axis k, whose sign picks the face: the midpoint of an axis that pierces two
            opposite faces has p_k = 0
  position  the interior pair where sin^2 of the angle between the axes is below 1e-6 (depth and normal still checked)
Where dist has a whole stretch of minimisers (an axis parallel to a face it overhangs) the position ALONG the stretch
is unspecified: the reported position must lie on the stretch (its offset from the reference is along u and keeps the
parameter inside the stretch), depth and normal are checked as ever, and nothing is counted.
No family may leave more than 10 % of its cases out of a property.

Tolerance: TOL = 1e-12 absolute of tests/collision_reference.py, on normal, depth and position.

The seeded families at the end are shared by the CPU test (twin against this reference) and the GPU test (device
against the twin and this reference): 64 cases each, case k standing alone around x = 2 k so that one device call
takes a whole family.  Their references are computed once per process."""
import functools

import mpmath as mp
import numpy as np
from scipy.spatial.transform import Rotation

from collision_reference import TOL
from sphere_reference import (CASES, DPS, GUARD, MAX_LEFT_OUT, SPACING, _axpy, _col, _dot, _v, sphere_box, sphere_ground,
                              sphere_sphere)

BOX, SPHERE, CAPSULE = 0, 1, 2
FLAT = mp.mpf("1e-9")
PRUNE = mp.mpf("1e-6")


def and3(*xs):
    if any(x is False for x in xs):
        return False
    return None if any(x is None for x in xs) else True


def or3(*xs):
    if any(x is True for x in xs):
        return True
    return None if any(x is None for x in xs) else False


def not3(x):
    return None if x is None else not x


def _capsule(c, R, side):
    c, R, side = _v(c), _v(R), _v(side)
    return c, side[0], (side[2] - side[0]) / 2, _col(R, 2)


def _contact3(cand):
    return None if cand["guard_s"] else bool(cand["contact"])


def _near3(a, b, lo, hi):
    """|a - b| <= 1e-9 of the flat rule, a close call when (a - b) lies in [lo, hi]."""
    diff = abs(a - b)
    return None if lo <= diff <= hi else bool(diff <= FLAT)


def _clamp(x, lo, hi):
    return max(lo, min(hi, x))


def capsule_ground(c, R, side):
    """Two candidates (dicts of sphere_ground) with present3."""
    with mp.workdps(DPS):
        c, d, e, u = _capsule(c, R, side)
        out = []
        for t in (-e, e):
            g = sphere_ground(_axpy(t, u, c), d)
            g["d"] = d
            out.append(g)
        return out


def capsule_sphere(cC, RC, sideC, cS, dS, first):
    """One candidate: sphere_sphere between the capsule's nearest ball and the sphere, normal body0 -> body1."""
    with mp.workdps(DPS):
        c, d, e, u = _capsule(cC, RC, sideC)
        cS = _v(cS)
        t = _clamp(_dot([cS[k] - c[k] for k in range(3)], u) / _dot(u, u), -e, e)
        b = _axpy(t, u, c)
        dS = _v([dS])[0]
        return [sphere_sphere(b, d, cS, dS) if first else sphere_sphere(cS, dS, b, d)]


def capsule_capsule(ci, Ri, si, cj, Rj, sj):
    with mp.workdps(DPS):
        ci, di, ei, ui = _capsule(ci, Ri, si)
        cj, dj, ej, uj = _capsule(cj, Rj, sj)
        out = []
        for q in range(4):
            te = 1 if q & 1 else -1
            if q < 2:
                bi = _axpy(te * ei, ui, ci)
                bj = _axpy(_clamp(_dot([bi[k] - cj[k] for k in range(3)], uj) / _dot(uj, uj), -ej, ej), uj, cj)
            else:
                bj = _axpy(te * ej, uj, cj)
                bi = _axpy(_clamp(_dot([bj[k] - ci[k] for k in range(3)], ui) / _dot(ui, ui), -ei, ei), ui, ci)
            cand = sphere_sphere(bi, di, bj, dj)
            cand["L"] = cand["s"] + (di + dj) / 2
            out.append(cand)
        w = [cj[k] - ci[k] for k in range(3)]
        A, B, a, p, q = _dot(ui, ui), _dot(uj, uj), _dot(ui, uj), _dot(ui, w), _dot(uj, w)
        det = A * B - a * a
        sin2 = det / (A * B)
        if sin2 != 0:
            s, t = (p * B - a * q) / det, (a * p - A * q) / det
            inside = -ei < s < ei and -ej < t < ej
            close = min(abs(s - ei), abs(s + ei)) < GUARD * ei or min(abs(t - ej), abs(t + ej)) < GUARD * ej
            cand = sphere_sphere(_axpy(s, ui, ci), di, _axpy(t, uj, cj), dj)
            cand["L"] = cand["s"] + (di + dj) / 2
            inside3 = None if (close or sin2 < mp.mpf("1e-24")) else inside
            flat3 = or3(*[and3(_contact3(c), _near3(c["L"], cand["L"], mp.mpf("1e-10"), mp.mpf("1e-8"))) for c in out])
            cand["interior3"] = and3(inside3, not3(flat3))
            cand["guard_pos"] = sin2 < mp.mpf("1e-6")
            out.append(cand)
        return out


def box_distance(p0, ub, h, t):
    e = [p0[k] + t * ub[k] for k in range(3)]
    e = [x - _clamp(x, -h[k], h[k]) for k, x in enumerate(e)]
    return mp.sqrt(_dot(e, e))


def box_axis_minimisers(p0, ub, h, e):
    """(t_lo, t_hi, enters): the set of minimisers of dist on [-e, e]; enters = the axis meets the box, where t_lo =
    t_hi = the midpoint of the stretch inside."""
    lo, hi = -e, e
    knots = {-e, e}
    for k in range(3):
        if ub[k] != 0:
            xa, xb = (-h[k] - p0[k]) / ub[k], (h[k] - p0[k]) / ub[k]
            lo, hi = max(lo, min(xa, xb)), min(hi, max(xa, xb))
            knots |= {_clamp(xa, -e, e), _clamp(xb, -e, e)}
        elif abs(p0[k]) > h[k]:
            hi = -mp.inf
    if lo <= hi:
        return (lo + hi) / 2, (lo + hi) / 2, True
    knots = sorted(knots)
    cands = list(knots)
    for a, b in zip(knots[:-1], knots[1:]):
        m = (a + b) / 2
        num = den = mp.mpf(0)
        for k in range(3):
            p = p0[k] + m * ub[k]
            sg = 1 if p > h[k] else (-1 if p < -h[k] else 0)
            if sg:
                num += ub[k] * (p0[k] - sg * h[k]); den += ub[k] * ub[k]
        if den > 0:
            cands.append(_clamp(-num / den, a, b))
    f = [(box_distance(p0, ub, h, t), t) for t in cands]
    fmin = min(f)[0]
    ts = [t for v, t in f if v - fmin <= mp.mpf("1e-40")]
    return min(ts), max(ts), False


def capsule_box(cC, RC, sideC, cB, RB, sideB):
    """Three candidates (sphere_box dicts; the normal is n_BS, box towards capsule): end 0, end 1, the interior point."""
    with mp.workdps(DPS):
        c, d, e, u = _capsule(cC, RC, sideC)
        cBm, R, h = _v(cB), _v(RB), [x / 2 for x in _v(sideB)]
        ax = [_col(R, k) for k in range(3)]
        rel = [c[k] - cBm[k] for k in range(3)]
        p0, ub = [_dot(ax[k], rel) for k in range(3)], [_dot(ax[k], u) for k in range(3)]
        out = []
        for t in (-e, e):
            cand = sphere_box(_axpy(t, u, c), d, cB, RB, sideB)
            cand["L"] = box_distance(p0, ub, h, t)
            out.append(cand)
        t_lo, t_hi, enters = box_axis_minimisers(p0, ub, h, e)
        cand = sphere_box(_axpy(t_lo, u, c), d, cB, RB, sideB)
        cand["L"] = box_distance(p0, ub, h, t_lo)
        if cand.get("inside", False):     # the face's sign is sgn(p_k): a close call where the midpoint has p_k = 0,
            p = [p0[k] + t_lo * ub[k] for k in range(3)]          # as it has when the axis pierces two opposite faces
            g = [h[k] - abs(p[k]) for k in range(3)]
            k = min(range(3), key=lambda a: (g[a], a))
            cand["guard_n"] = cand["guard_n"] or abs(p[k]) < GUARD
        inside = -e < t_lo < e
        close = min(abs(t_lo - e), abs(t_lo + e)) < GUARD * e
        flat3 = or3(*[and3(_contact3(q), _near3(q["L"], cand["L"], mp.mpf("1e-10"), mp.mpf("1e-8"))) for q in out])
        # a close call on "strictly inside" matters only where the flat rule would not drop the candidate anyway
        cand["interior3"] = and3(None if close else inside, not3(flat3))
        if t_hi - t_lo > GUARD * e:
            cand["stretch"] = (u, t_hi - t_lo)
        out.append(cand)
        return out


def pair(pos, R, side, shape, i=0, j=1):
    """The candidates of bodies i < j of which at least one is a capsule, in the device's order, normals body0 -> body1."""
    ki, kj = shape[i] == CAPSULE, shape[j] == CAPSULE
    if ki and kj:
        return capsule_capsule(pos[i], R[i], side[i], pos[j], R[j], side[j])
    if ki and shape[j] == SPHERE:
        return capsule_sphere(pos[i], R[i], side[i], pos[j], side[j][0], True)
    if kj and shape[i] == SPHERE:
        return capsule_sphere(pos[j], R[j], side[j], pos[i], side[i][0], False)
    if ki:
        out = capsule_box(pos[i], R[i], side[i], pos[j], R[j], side[j])
        with mp.workdps(DPS):
            for c in out:
                c["row"] = c["row"][:3] + [-x for x in c["row"][3:6]] + c["row"][6:]
        return out
    return capsule_box(pos[j], R[j], side[j], pos[i], R[i], side[i])


def _row_error(cand, row):
    """The largest error of a reported row against a candidate over the properties not guarded; None if it is no match
    (beyond TOL).  Also returns the set of properties left out."""
    left = set()
    got = [mp.mpf(float(x)) for x in row]
    ref = cand["row"]
    err = mp.mpf(0)
    inside_guard = cand.get("guard_n", False) and cand.get("inside", False)   # the depth rides on the face chosen
    if not inside_guard:
        err = abs(got[6] - ref[6])
    if cand.get("guard_n", False):
        left.add("normal")
    else:
        err = max([err] + [abs(got[k] - ref[k]) for k in range(3, 6)])
        if cand.get("guard_pos", False):
            left.add("position")
        elif "stretch" in cand:
            u, length = cand["stretch"]
            off = [got[k] - ref[k] for k in range(3)]
            lam = _dot(off, u) / _dot(u, u)
            err = max([err] + [abs(off[k] - lam * u[k]) for k in range(3)])
            err = max(err, -lam, lam - length)          # lam in [0, length] up to the tolerance
        else:
            err = max([err] + [abs(got[k] - ref[k]) for k in range(3)])
    return (float(err) if err <= TOL else None), left


def compare(cands, rows, left_out, ground=False):
    """rows = what the code under test reports for the case whose candidates are `cands`, in order.  Asserts every
    decision outside its guard band and normal, depth, position within TOL outside theirs; adds the case to left_out
    (a dict of counters) once per property left out.  Returns the largest error seen."""
    with mp.workdps(DPS):
        rows = list(rows)
        left, worst, nxt = set(), 0.0, 0
        seen = []       # (present3 before pruning, position) of the earlier candidates
        for cand in cands:
            c3 = _contact3(cand)
            i3 = cand.get("interior3", True)
            gen3 = and3(c3, i3)
            pruned3 = False
            if not ground:
                near = []
                for g3, p in seen:
                    dist = mp.sqrt(sum((p[k] - cand["row"][k]) ** 2 for k in range(3)))
                    n3 = None if PRUNE / 2 <= dist <= PRUNE * 2 else bool(dist < PRUNE)
                    near.append(and3(g3, n3))
                pruned3 = or3(*near) if near else False
                seen.append((gen3, cand["row"][:3]))
            present3 = and3(gen3, not3(pruned3))
            if present3 is None:
                left.add("interior" if (c3 is not None and pruned3 is False) else "decision")
                if nxt < len(rows):
                    e, lf = _row_error(cand, rows[nxt])
                    if e is not None:
                        worst = max(worst, e); left |= lf; nxt += 1
                continue
            if not present3:
                continue
            assert nxt < len(rows), ("a contact is missing", float(cand["s"]), len(rows))
            e, lf = _row_error(cand, rows[nxt])
            assert e is not None, ("row", [float(mp.mpf(float(rows[nxt][k])) - cand["row"][k]) for k in range(7)])
            worst = max(worst, e); left |= lf; nxt += 1
        assert nxt == len(rows), ("contacts beyond the reference's", len(rows) - nxt)
        for what in left:
            left_out[what] = left_out.get(what, 0) + 1
        return worst


# ---- seeded case families ------------------------------------------------------------------------------------------
FAMILIES = ("ground", "cap_sphere", "crossed", "tee", "parallel", "collinear", "box_end", "box_flat", "box_edge",
            "box_corner", "box_narrow", "box_through", "near_miss")
_SEEDS = {name: 31 + k for k, name in enumerate(FAMILIES)}
_NEAR_KINDS = ("cap_sphere", "crossed", "tee", "parallel", "collinear", "box_end", "box_flat", "box_edge", "box_corner")


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _perp(rng, u):
    v = rng.normal(size=3)
    v -= v.dot(u) * u
    return v / np.linalg.norm(v)


def _frame(rng, u):
    """A rotation (row-major [9]) whose column 2 is u, with a random roll."""
    a = _perp(rng, u)
    return np.stack([a, np.cross(u, a), u], axis=1).reshape(9)


def _rot(rng):
    return Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix().reshape(9)


def _sep(rng, near):
    """The signed separation of a case: touching or in (3 of 4) or clear, over many magnitudes; near: just clear."""
    if near:
        return 10.0 ** rng.uniform(-6, -3)
    return rng.choice([-1.0, 1.0], p=[0.75, 0.25]) * 10.0 ** rng.uniform(-7, -1.3)


def _capsule_dims(rng, long=False):
    d = rng.uniform(0.1, 0.3)
    return d, d + (rng.uniform(1.0, 1.2) if long else rng.uniform(0.25, 0.6))


def _case(kind, rng, o, k, near=False):
    """Two bodies of one case around o: (pos, R, side, shape) lists in (i, j) order."""
    s = _sep(rng, near)
    d, l = _capsule_dims(rng, long=kind in ("box_through", "box_narrow"))
    r, e = d / 2, (l - d) / 2
    c = o + rng.uniform(-0.1, 0.1, 3)
    if kind == "cap_sphere":
        u = _unit(rng)
        ds = rng.uniform(0.1, 0.5)
        region = k % 3                                     # side, beyond end 0, beyond end 1
        if region == 0:
            cS = c + rng.uniform(-0.9, 0.9) * e * u + _perp(rng, u) * (r + ds / 2 + s)
        else:
            end = -1.0 if region == 1 else 1.0
            w = _unit(rng)
            w = w if w.dot(u) * end > 0 else -w
            cS = c + end * e * u + w * (r + ds / 2 + s)
        bodies = [(c, _frame(rng, u), [d, d, l], CAPSULE), (cS, _rot(rng), [ds] * 3, SPHERE)]
    elif kind in ("crossed", "tee", "parallel", "collinear"):
        d2, l2 = _capsule_dims(rng)
        r2, e2 = d2 / 2, (l2 - d2) / 2
        u = _unit(rng)
        if kind == "crossed":
            while True:
                u2 = _unit(rng)
                n = np.cross(u, u2)
                if np.linalg.norm(n) >= 0.3:
                    break
            n /= np.linalg.norm(n)
            c2 = c + rng.uniform(-0.8, 0.8) * e * u + n * (r + r2 + s) - rng.uniform(-0.8, 0.8) * e2 * u2
            R1, R2 = _frame(rng, u), _frame(rng, u2)
        elif kind == "tee":                                 # an end of the second capsule on the first one's side
            n = _perp(rng, u)
            u2 = n + 0.4 * rng.uniform(-1, 1, 3)
            u2 /= np.linalg.norm(u2)
            end = 1.0 if k % 4 < 2 else -1.0               # the stem's end 0 (axis pointing away) or its end 1
            c2 = c + rng.uniform(-0.8, 0.8) * e * u + n * (r + r2 + s) + e2 * u2
            R1, R2 = _frame(rng, u), _frame(rng, end * u2)
        elif kind == "parallel":
            R1 = R2 = _frame(rng, u)
            mode = k % 3                                    # partly overlapping, fully overlapping, equal and aligned
            if mode == 2:
                d2, l2, r2, e2, shift = d, l, r, e, 0.0
            elif mode == 1:
                shift = rng.uniform(-0.8, 0.8) * abs(e - e2)
            else:
                shift = rng.choice([-1.0, 1.0]) * (abs(e - e2) + rng.uniform(0.2, 0.8) * (e + e2 - abs(e - e2)))
            c2 = c + shift * u + _perp(rng, u) * (r + r2 + s)
        else:
            R1 = R2 = _frame(rng, u)
            c2 = c + rng.choice([-1.0, 1.0]) * (e + e2 + r + r2 + s) * u
        bodies = [(c, R1, [d, d, l], CAPSULE), (c2, R2, [d2, d2, l2], CAPSULE)]
    else:
        exact = kind in ("box_flat", "box_narrow")
        if kind == "box_flat":
            sb = np.array([rng.uniform(1.2, 1.5), rng.uniform(1.2, 1.5), rng.uniform(0.15, 0.5)])
        elif kind == "box_narrow":
            sb = np.array([rng.uniform(0.15, 0.3), rng.uniform(1.0, 1.3), rng.uniform(0.15, 0.5)])
        else:
            sb = rng.uniform(0.15, 0.6, 3)
        h = sb / 2
        if exact:                                           # the box frame is the world's; the axis has u_z = 0 exactly
            RB = np.eye(3).reshape(9)
            th = rng.uniform(-0.3, 0.3) if kind == "box_narrow" else rng.uniform(0, 2 * np.pi)
            u = np.array([np.cos(th), np.sin(th), 0.0])
            face = 1.0 if k % 2 == 0 else -1.0
            p = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), face * (h[2] + r + s)])
            RC = np.stack([[0.0, 0.0, 1.0], np.cross(u, [0.0, 0.0, 1.0]), u], axis=1).reshape(9)
        else:
            RB = _rot(rng)
            sg = rng.choice([-1.0, 1.0], 3)
            if kind == "box_through":
                u = _unit(rng)
                u[np.argmin(h)] *= 0.2      # mostly across the thin direction: piercing its two faces makes the
                u /= np.linalg.norm(u)      # midpoint's face a coin toss (guarded), which a few cases still do
                p = rng.uniform(-0.6, 0.6, 3) * h - rng.uniform(-0.3, 0.3) * e * u
            else:
                nout = dict(box_end=1, box_edge=2, box_corner=3)[kind]
                out = rng.permutation(3)[:nout]
                n = np.zeros(3)
                n[out] = rng.uniform(0.3, 1.0, nout)
                n /= np.linalg.norm(n)
                q = rng.uniform(-0.6, 0.6, 3) * h
                q[out] = h[out]
                if kind == "box_end":                       # end 0 on the face, the axis leaning away from it
                    u = n + 0.8 * rng.uniform(-1, 1, 3)
                    u /= np.linalg.norm(u)
                    if u.dot(n) < 0.3:
                        u = n
                    p = q + n * (r + s) + e * u
                else:                                       # the axis perpendicular to n through q + n (r + s), at t0
                    m = _perp(rng, n)
                    if kind == "box_edge":                  # mostly across the edge
                        free = [a for a in range(3) if a not in out][0]
                        across = np.cross(n, np.eye(3)[free])
                        m = across + 0.4 * rng.uniform(-1, 1) * np.eye(3)[free]
                        m /= np.linalg.norm(m)
                    u = m
                    p = q + n * (r + s) - rng.uniform(-0.5, 0.5) * e * u
                p, u = p * sg, u * sg                       # any of the faces / edges / corners
            RC = None
        RBm = RB.reshape(3, 3)
        cB = c
        cC = cB + RBm @ p
        if RC is None:
            RC = _frame(rng, RBm @ u)
        bodies = [(cC, RC, [d, d, l], CAPSULE), (cB, RB, list(sb), BOX)]
    if rng.uniform() < 0.5 and kind not in ("crossed", "tee", "parallel", "collinear"):
        bodies = bodies[::-1]
    return bodies


@functools.lru_cache(maxsize=None)
def family(name):
    """dict(pos [n][3], R [n][9], side [n][3], shape [n], pairs [(i, j)] or None for the ground family): CASES cases,
    case k around x = SPACING * k and well above the ground unless the family is about it."""
    rng = np.random.default_rng(_SEEDS[name])
    pos, R, side, shape, pairs = [], [], [], [], []
    for k in range(CASES):
        o = np.array([SPACING * k, 0.0, 3.0])
        if name == "ground":
            d, l = _capsule_dims(rng)
            r, e = d / 2, (l - d) / 2
            mode = k % 4                                   # one end in, both in, exactly horizontal, clear
            if mode == 0:
                u = _unit(rng)
                while abs(u[2]) < 0.3:
                    u = _unit(rng)
                s = -10.0 ** rng.uniform(-8, -1.5)
            elif mode == 1:
                s = -10.0 ** rng.uniform(-3, -1.5)
                th = rng.uniform(0, 2 * np.pi)
                uz = rng.uniform(-1, 1) * 0.2 * (-s) / e
                u = np.array([np.cos(th) * np.sqrt(1 - uz * uz), np.sin(th) * np.sqrt(1 - uz * uz), uz])
            elif mode == 2:
                th = rng.uniform(0, 2 * np.pi)
                u = np.array([np.cos(th), np.sin(th), 0.0])
                s = rng.choice([-1.0, 1.0], p=[0.75, 0.25]) * 10.0 ** rng.uniform(-8, -1.5)
            else:
                u = _unit(rng)
                s = 10.0 ** rng.uniform(-8, -1.5)
            Rc = np.stack([[0.0, 0.0, 1.0], np.cross(u, [0.0, 0.0, 1.0]), u], axis=1).reshape(9) if mode == 2 else _frame(rng, u)
            pos.append([o[0], rng.uniform(-0.3, 0.3), r + s + e * abs(u[2])]); R.append(Rc); side.append([d, d, l])
            shape.append(CAPSULE)
            continue
        kind = _NEAR_KINDS[k % len(_NEAR_KINDS)] if name == "near_miss" else name
        for c, Rb, sd, sh in _case(kind, rng, o, k, near=name == "near_miss"):
            pos.append(c); R.append(Rb); side.append(sd); shape.append(sh)
        pairs.append((2 * k, 2 * k + 1))
    return dict(pos=np.array(pos, np.float64), R=np.array(R, np.float64), side=np.array(side, np.float64),
                shape=np.array(shape, np.int32), pairs=pairs or None)


@functools.lru_cache(maxsize=None)
def family_reference(name):
    """The candidates of every case of the family, in case order."""
    f = family(name)
    if name == "ground":
        return [capsule_ground(f["pos"][b], f["R"][b], f["side"][b]) for b in range(CASES)]
    return [pair(f["pos"], f["R"], f["side"], f["shape"], i, j) for i, j in f["pairs"]]


def check_family(name, b0, b1, data):
    """A contact list of the whole family (twin's or device's) against the reference, case by case; returns
    (largest error, left-out counters) after asserting that no property left out more than MAX_LEFT_OUT of the cases."""
    f, refs = family(name), family_reference(name)
    left_out, worst, seen = {}, 0.0, 0
    for k, cands in enumerate(refs):
        if name == "ground":
            sel = (b0 == -1) & (b1 == k)
        else:
            i, j = f["pairs"][k]
            sel = (b0 == i) & (b1 == j)
        seen += int(sel.sum())
        try:
            worst = max(worst, compare(cands, list(data[sel]), left_out, ground=name == "ground"))
        except AssertionError as err:
            raise AssertionError("%s case %d: %s" % (name, k, err)) from None
    assert seen == len(b0), "contacts outside the family's cases"
    for what, c in left_out.items():
        assert c <= MAX_LEFT_OUT * CASES, (name, what, c)
    return worst, left_out
