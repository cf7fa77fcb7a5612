"""The capsule narrow phase of collide.hip in numpy fp64, operation for operation: the statement the device must match
bit for bit (tests/test_gpu_collide_capsules.py).  Every line is one rounding, as the device's -ffp-contract=off code
is; sqrt and / are IEEE in both.  Contact rows are [7] = position, normal, depth.

A capsule's side row is (d, d, l): r = side[0] * 0.5, e = (side[2] - side[0]) * 0.5, axis u = (R[2], R[5], R[8]); the
ball at t is centred at c_k + t * u_k.  The balls go through the sphere functions of sphere_twin.py."""
import math

import numpy as np

import sphere_twin as st
from sphere_twin import _dot3, _f

BOX, SPHERE, CAPSULE = 0, 1, 2
FLAT = 1e-9
INF = float("inf")


def _capsule(R, side):
    R, side = _f(R), _f(side)
    return (side[2] - side[0]) * 0.5, [R[2], R[5], R[8]]


def _ball_at(c, u, t):
    return [c[0] + t * u[0], c[1] + t * u[1], c[2] + t * u[2]]


def _balls(ci, si, cj, sj):
    """collide_balls: collide_spheres and the centre distance L."""
    ci, si, cj, sj = _f(ci), _f(si), _f(cj), _f(sj)
    d = [cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]]
    return st.collide_spheres(ci, si, cj, sj), float(np.sqrt(_dot3(d, d)))


def _nearest(cC, e, u, cS):
    w = [cS[0] - cC[0], cS[1] - cC[1], cS[2] - cC[2]]
    return min(max(_dot3(w, u), -e), e)


def ground_capsule(c, R, side):
    c = _f(c)
    e, u = _capsule(R, side)
    return st.ground_sphere(_ball_at(c, u, -e), side) + st.ground_sphere(_ball_at(c, u, e), side)


def collide_capsule_sphere(cC, RC, sideC, cS, sideS, first):
    """first: the capsule is body0."""
    cC, cS = _f(cC), _f(cS)
    e, u = _capsule(RC, sideC)
    b = _ball_at(cC, u, _nearest(cC, e, u, cS))
    return st.collide_spheres(b, sideC, cS, sideS) if first else st.collide_spheres(cS, sideS, b, sideC)


def collide_capsules(ci, Ri, si, cj, Rj, sj):
    ci, cj = _f(ci), _f(cj)
    ei, ui = _capsule(Ri, si)
    ej, uj = _capsule(Rj, sj)
    out, hit, Lend = [], [], []
    for q in range(4):
        te = 1.0 if q & 1 else -1.0
        if q < 2:
            bi = _ball_at(ci, ui, te * ei)
            bj = _ball_at(cj, uj, _nearest(cj, ej, uj, bi))
        else:
            bj = _ball_at(cj, uj, te * ej)
            bi = _ball_at(ci, ui, _nearest(ci, ei, ui, bj))
        rows, L = _balls(bi, si, bj, sj)
        hit.append(bool(rows)); Lend.append(L)
        out += rows
    w = [cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]]
    A, B, a, p, q = _dot3(ui, ui), _dot3(uj, uj), _dot3(ui, uj), _dot3(ui, w), _dot3(uj, w)
    det = A * B - a * a
    if det != 0:
        s = (p * B - a * q) / det
        t = (a * p - A * q) / det
        if -ei < s < ei and -ej < t < ej:
            rows, L = _balls(_ball_at(ci, ui, s), si, _ball_at(cj, uj, t), sj)
            flat = any(hit[k] and abs(Lend[k] - L) <= FLAT for k in range(4))
            if rows and not flat:
                out += rows
    return out


def _axis_dist2(p0, ub, h, t):
    e = []
    for k in range(3):
        p = p0[k] + t * ub[k]
        e.append(p - min(max(p, -h[k]), h[k]))
    return _dot3(e, e)


_NETWORK = ((0, 5), (1, 3), (2, 4), (1, 2), (3, 4), (0, 3), (2, 5), (0, 1), (2, 3), (4, 5), (1, 2), (3, 4))


def box_axis(cC, RC, sideC, cB, RB, sideB):
    """(e, u, p0, ub, h, t*) of collide_capsule_box: the axis in the box frame and the interior parameter."""
    cC, cB, RB, sideB = _f(cC), _f(cB), _f(RB), _f(sideB)
    e, u = _capsule(RC, sideC)
    dc = [cC[0] - cB[0], cC[1] - cB[1], cC[2] - cB[2]]
    p0 = [(RB[k] * dc[0] + RB[3 + k] * dc[1]) + RB[6 + k] * dc[2] for k in range(3)]
    ub = [(RB[k] * u[0] + RB[3 + k] * u[1]) + RB[6 + k] * u[2] for k in range(3)]
    h = [sideB[k] * 0.5 for k in range(3)]
    lo, hi = -e, e
    x = []
    for k in range(3):
        if ub[k] != 0:
            xa, xb = (-h[k] - p0[k]) / ub[k], (h[k] - p0[k]) / ub[k]
            lo = max(lo, min(xa, xb)); hi = min(hi, max(xa, xb))
        else:
            xa = xb = INF
            if abs(p0[k]) > h[k]:
                hi = -INF
        x += [xa, xb]
    if lo <= hi:
        return e, u, p0, ub, h, (lo + hi) * 0.5
    x = [min(max(v, -e), e) for v in x]
    for a, b in _NETWORK:
        x[a], x[b] = min(x[a], x[b]), max(x[a], x[b])
    tau = [-e] + x + [e]
    ts = tau[0]
    best = _axis_dist2(p0, ub, h, ts)
    for i in range(7):
        m = (tau[i] + tau[i + 1]) * 0.5
        num = den = 0.0
        for k in range(3):
            p = p0[k] + m * ub[k]
            sg = 1.0 if p > h[k] else (-1.0 if p < -h[k] else 0.0)
            if sg != 0:
                num = num + ub[k] * (p0[k] - sg * h[k])
                den = den + ub[k] * ub[k]
        if den > 0:
            s = min(max(-num / den, tau[i]), tau[i + 1])
            f = _axis_dist2(p0, ub, h, s)
            if f < best:
                best, ts = f, s
        f = _axis_dist2(p0, ub, h, tau[i + 1])
        if f < best:
            best, ts = f, tau[i + 1]
    return e, u, p0, ub, h, ts


def collide_capsule_box(cC, RC, sideC, cB, RB, sideB, flip):
    """flip: the capsule is body0."""
    e, u, p0, ub, h, ts = box_axis(cC, RC, sideC, cB, RB, sideB)
    cC = _f(cC)
    r0 = st.collide_sphere_box(_ball_at(cC, u, -e), sideC, cB, RB, sideB, flip)
    r1 = st.collide_sphere_box(_ball_at(cC, u, e), sideC, cB, RB, sideB, flip)
    out = r0 + r1
    if -e < ts < e:
        Ds = math.sqrt(_axis_dist2(p0, ub, h, ts))
        flat = False
        if r0:
            flat |= abs(math.sqrt(_axis_dist2(p0, ub, h, -e)) - Ds) <= FLAT
        if r1:
            flat |= abs(math.sqrt(_axis_dist2(p0, ub, h, e)) - Ds) <= FLAT
        if not flat:
            out += st.collide_sphere_box(_ball_at(cC, u, ts), sideC, cB, RB, sideB, flip)
    return out


def _prune(cs):
    """narrow_kernel's same-pair pruning: a contact within 1e-6 of ANY earlier contact of the pair is deleted."""
    def near(a, b):
        d = [float(b[k]) - float(a[k]) for k in range(3)]
        return float(np.sqrt(_dot3(d, d))) < 1e-6
    return [cs[a] for a in range(len(cs)) if not any(near(cs[a], cs[b]) for b in range(a))]


def pair(pos, R, side, shape, i, j):
    """The contacts of bodies i < j after the same-pair pruning, before the joint pruning."""
    ki, kj = shape[i] == CAPSULE, shape[j] == CAPSULE
    if not (ki or kj):
        return st.pair(pos, R, side, shape, i, j)
    if ki and kj:
        cs = collide_capsules(pos[i], R[i], side[i], pos[j], R[j], side[j])
    elif ki and shape[j] == SPHERE:
        cs = collide_capsule_sphere(pos[i], R[i], side[i], pos[j], side[j], True)
    elif kj and shape[i] == SPHERE:
        cs = collide_capsule_sphere(pos[j], R[j], side[j], pos[i], side[i], False)
    elif ki:
        cs = collide_capsule_box(pos[i], R[i], side[i], pos[j], R[j], side[j], True)
    else:
        cs = collide_capsule_box(pos[j], R[j], side[j], pos[i], R[i], side[i], False)
    return _prune(cs)


def contacts(pos, R, side, shape, pairs=None):
    """The whole list in the device's order: ground contacts by body, then the pairs i < j (all of them, or `pairs`)."""
    pos, R, side = (np.asarray(a, np.float64).reshape(-1, k) for a, k in ((pos, 3), (R, 9), (side, 3)))
    n = pos.shape[0]
    b0, b1, data = [], [], []
    for b in range(n):
        if shape[b] == CAPSULE:
            cs = ground_capsule(pos[b], R[b], side[b])
        elif shape[b] == SPHERE:
            cs = st.ground_sphere(pos[b], side[b])
        else:
            from oracle import oracle as orc
            cs = orc.collide_box_ground(pos[b], R[b], side[b])
        for c in cs:
            b0.append(-1); b1.append(b); data.append(c)
    for i, j in (pairs if pairs is not None else [(i, j) for i in range(n) for j in range(i + 1, n)]):
        for c in pair(pos, R, side, shape, i, j):
            b0.append(i); b1.append(j); data.append(c)
    return np.array(b0, np.int32), np.array(b1, np.int32), np.array(data, np.float64).reshape(-1, 7)
