"""The ray cast of raycast.hip in Python fp64, operation for operation: the statement the device must match bit for bit
(tests/test_gpu_raycast.py).  Every line is one rounding, as the device's -ffp-contract=off code is; sqrt and / are IEEE
in both.  The rules are stated above egs_cast_rays in include/eggshell_amd.h.

Choices the twin states (the reference measures them):
  * the entering root of |w + t d|^2 = r^2 in the perpendicular-offset form: s = (w . d) / (d . d), m = w - s d,
    disc = r^2 - m . m, t = -s - sqrt(disc / (d . d)); no root unless disc >= 0, and it counts iff t >= 0;
  * a normal is (w + t d) / |w + t d| from the same w and d the root was found with;
  * the scan goes ground, then bodies in ascending index; a later candidate replaces the best only with t strictly
    smaller, the first one needs t <= tmax.  That IS "the minimum, ties to the ground and then the lowest index".
The bounding-sphere cull of the device is not restated: it must not change a result, which the device test checks by
running every family with it off."""
import math

import numpy as np

from sphere_twin import _dot3, _f

BOX, SPHERE, CAPSULE = 0, 1, 2
MISS, GROUND = -2, -1
INF = float("inf")


def enter_root(w, d, dd, r2):
    """-1.0 where there is no entering root or it is negative."""
    s = _dot3(w, d) / dd
    m = [w[0] - s * d[0], w[1] - s * d[1], w[2] - s * d[2]]
    disc = r2 - _dot3(m, m)
    if not disc >= 0.0:
        return -1.0
    h = math.sqrt(disc / dd)
    t = -s - h
    return t if t >= 0.0 else -1.0


def radial_normal(w, d, t):
    q = [w[0] + t * d[0], w[1] + t * d[1], w[2] + t * d[2]]
    L = math.sqrt(_dot3(q, q))
    return [q[0] / L, q[1] / L, q[2] / L]


INSIDE = (0.0, [0.0, 0.0, 0.0])


def ray_ground(o, d):
    """None (no hit) or (t, normal); INSIDE where the origin is below the plane."""
    if o[2] < 0.0:
        return INSIDE
    if d[2] < 0.0:
        return o[2] / (-d[2]), [0.0, 0.0, 1.0]
    return None


def ray_sphere(c, side, o, d, dd):
    w = [o[0] - c[0], o[1] - c[1], o[2] - c[2]]
    r = side[0] * 0.5
    r2 = r * r
    if _dot3(w, w) < r2:
        return INSIDE
    t = enter_root(w, d, dd, r2)
    if t >= 0.0:
        return t, radial_normal(w, d, t)
    return None


def ray_box(c, R, side, o, d):
    w = [o[0] - c[0], o[1] - c[1], o[2] - c[2]]
    tin, tout, kin, sign_in, miss = -INF, INF, 0, False, False
    for k in range(3):
        p = (R[k] * w[0] + R[3 + k] * w[1]) + R[6 + k] * w[2]
        q = (R[k] * d[0] + R[3 + k] * d[1]) + R[6 + k] * d[2]
        h = side[k] * 0.5
        if q == 0.0:
            if abs(p) > h:
                miss = True
        else:
            ta, tb = (-h - p) / q, (h - p) / q
            tn, tf = min(ta, tb), max(ta, tb)
            if tn > tin:
                tin, kin, sign_in = tn, k, q > 0.0
            if tf < tout:
                tout = tf
    if miss or not tin <= tout or not tout > 0.0:
        return None
    if tin < 0.0:
        return INSIDE
    col = [R[kin], R[3 + kin], R[6 + kin]]
    return tin, [-x if sign_in else x for x in col]


def ray_capsule(c, R, side, o, d, dd):
    w = [o[0] - c[0], o[1] - c[1], o[2] - c[2]]
    u = [R[2], R[5], R[8]]
    r = side[0] * 0.5
    e = (side[2] - side[0]) * 0.5
    r2 = r * r
    wu = _dot3(w, u)
    s = min(max(wu, -e), e)
    v = [w[0] - s * u[0], w[1] - s * u[1], w[2] - s * u[2]]
    if _dot3(v, v) < r2:
        return INSIDE
    du = _dot3(d, u)
    wp = [w[0] - wu * u[0], w[1] - wu * u[1], w[2] - wu * u[2]]
    dp = [d[0] - du * u[0], d[1] - du * u[1], d[2] - du * u[2]]
    a = _dot3(dp, dp)
    t, part = -1.0, 0
    if a != 0.0:
        ts = enter_root(wp, dp, a, r2)
        if ts >= 0.0:
            ax = wu + ts * du
            if -e <= ax <= e:
                t = ts
    ne = -e
    w0 = [o[0] - (c[0] + ne * u[0]), o[1] - (c[1] + ne * u[1]), o[2] - (c[2] + ne * u[2])]
    t0 = enter_root(w0, d, dd, r2)
    if t0 >= 0.0 and (t < 0.0 or t0 < t):
        t, part = t0, 1
    w1 = [o[0] - (c[0] + e * u[0]), o[1] - (c[1] + e * u[1]), o[2] - (c[2] + e * u[2])]
    t1 = enter_root(w1, d, dd, r2)
    if t1 >= 0.0 and (t < 0.0 or t1 < t):
        t, part = t1, 2
    if not t >= 0.0:
        return None
    if part == 0:
        return t, radial_normal(wp, dp, t)
    return t, radial_normal(w0 if part == 1 else w1, d, t)


def world_frame(c, R, o, d):
    """An attached ray in the world frame: o_w = c + R o, d_w = R d, as the device forms them."""
    c, R, o, d = _f(c), _f(R), _f(o), _f(d)
    ow = [c[k] + ((R[3 * k] * o[0] + R[3 * k + 1] * o[1]) + R[3 * k + 2] * o[2]) for k in range(3)]
    dw = [(R[3 * k] * d[0] + R[3 * k + 1] * d[1]) + R[3 * k + 2] * d[2] for k in range(3)]
    return ow, dw


def cast_one(pos, R, side, shape, o, d, tmax, skip=-1, lo=0, hi=None):
    """One world-frame ray against the ground and the bodies [lo, hi) except skip: (body, t, normal)."""
    o, d, tmax = _f(o), _f(d), float(tmax)
    dd = _dot3(d, d)
    best = (MISS, tmax, [0.0, 0.0, 0.0])

    def offer(body, got, best):
        if got is None:
            return best
        t, n = got
        if (t <= tmax) if best[0] == MISS else (t < best[1]):
            return (body, t, n)
        return best

    best = offer(GROUND, ray_ground(o, d), best)
    for j in range(lo, len(pos) if hi is None else hi):
        if j == skip:
            continue
        c, Rj, sj = _f(pos[j]), _f(R[j]), _f(side[j])
        sh = BOX if shape is None else int(shape[j])
        if sh == BOX:
            got = ray_box(c, Rj, sj, o, d)
        elif sh == SPHERE:
            got = ray_sphere(c, sj, o, d, dd)
        else:
            got = ray_capsule(c, Rj, sj, o, d, dd)
        best = offer(j, got, best)
    return best


def cast(pos, R, side, shape, origin, dir, tmax, ray_body=None, ray_ens=None, body_off=None):
    """(hit_body int32 [n], t [n], normal [n][3]) of egs_cast_rays / egs_world_cast_rays."""
    pos, R, side = (np.asarray(a, np.float64).reshape(-1, k) for a, k in ((pos, 3), (R, 9), (side, 3)))
    origin, dir = np.asarray(origin, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
    n = origin.shape[0]
    hit, t, normal = np.full(n, MISS, np.int32), np.zeros(n), np.zeros((n, 3))
    for i in range(n):
        o, d = origin[i], dir[i]
        b = -1 if ray_body is None else int(ray_body[i])
        if b >= 0:
            o, d = world_frame(pos[b], R[b], o, d)
        lo, hi = (0, pos.shape[0]) if ray_ens is None else (int(body_off[ray_ens[i]]), int(body_off[ray_ens[i] + 1]))
        hit[i], t[i], normal[i] = cast_one(pos, R, side, shape, o, d, tmax[i], b, lo, hi)
    return hit, t, normal
