"""Ray casts as mathematics, in mpmath at 50 digits on the exact fp64 inputs: an INDEPENDENT reference for what
tests/ray_twin.py restates in fp64 and raycast.hip mirrors bit for bit.  The rules are those stated above egs_cast_rays
in include/eggshell_amd.h; nothing here follows the device's operation order -- the roots come from the plain quadratic
a t^2 + 2 b t + c = 0, t = (-b - sqrt(b^2 - a c)) / a, not from the twin's perpendicular-offset form.

A result per ray is (kind, body, t, normal): kind = "hit", "miss", "inside" or None = undecided.  Every governing
comparison is three-valued, with the and3 / or3 / not3 of capsule_reference.py: two sides that are not equal at 50 digits
but differ by less than GUARD = 1e-12 relative (of the larger side, or of the scale named at the comparison where one
side is 0) give None, and a None that the outcome depends on leaves the case out.  Two sides EQUAL at 50 digits are
decided as equal: the inputs are exact fp64 numbers, so an origin on the plane z = 0, a box-frame component that is 0
with R = I, or the same sphere listed twice are equalities of the statement, not close calls.

Families: 64 seeded rays each (heap: 256), built so that every governing margin is at least 1e-7 relative; the cap on
cases left out is 1 of 64 (0 for ground, heap and ties), asserted on the reference alone.

Tolerance.  BOUND[family] is collision_reference.TOL = 1e-12 (scenes of a metre or two) where the twin's worst error,
MEASURED[family] = max over the family of |dt| |d| (metres along the ray) and of the normal's largest component error,
is at most a quarter of it; a family above that (grazing rays, origins 100 r away: ill-conditioned by design) gets
4 x its measured worst.  MEASURED was measured once on the CPU by tests/test_ray_reference_cpu.py, which prints the
current figures; the device is held to the twin bit for bit, so no bound comes from a GPU run."""
import functools

import mpmath as mp
import numpy as np
from scipy.spatial.transform import Rotation

from capsule_reference import and3, not3, or3
from collision_reference import TOL

DPS = 50
GUARD = mp.mpf("1e-12")
BOX, SPHERE, CAPSULE = 0, 1, 2
MISS, GROUND = -2, -1
SPACING = 4.0
FAMILIES = ("ground", "sphere", "box", "capsule", "heap", "ties")
MAX_LEFT_OUT = {"ground": 0, "sphere": 1, "box": 1, "capsule": 1, "heap": 0, "ties": 0}

# the twin's worst error per family against this reference, as measured on the CPU (see the module docstring)
MEASURED = {"ground": 4.31e-16, "sphere": 3.04e-14, "box": 1.05e-15, "capsule": 8.44e-14, "heap": 3.29e-15, "ties": 4.65e-16}
BOUND = {k: (TOL if v <= TOL / 4 else 4 * v) for k, v in MEASURED.items()}


def _v(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _axpy(t, x, y):
    return [y[0] + t * x[0], y[1] + t * x[1], y[2] + t * x[2]]


def _unit(a):
    L = mp.sqrt(_dot(a, a))
    return [x / L for x in a]


def lt3(a, b, scale=None):
    """a < b: True, False, or None where a != b but |a - b| < GUARD * scale (default: the larger side)."""
    if a == b:
        return False
    s = max(abs(a), abs(b)) if scale is None else scale
    if abs(a - b) < GUARD * s:
        return None
    return bool(a < b)


def le3(a, b, scale=None):
    return True if a == b else lt3(a, b, scale)


ZERO3 = [mp.mpf(0)] * 3


def _ball(w, d, r):
    """The entering root of |w + t d| = r for an origin outside or on the ball: (present3, t)."""
    a, b, c = _dot(d, d), _dot(w, d), _dot(w, w) - r * r
    real = le3(a * c, b * b)                                  # b^2 - a c >= 0
    ahead = lt3(b, 0, mp.sqrt(a * _dot(w, w)))                # heading towards the centre
    if c == 0:                                                # on the surface: the root is 0 or behind, by the last bit
        return (None if ahead is not False else False), mp.mpf(0)
    here = and3(real, ahead)
    if here is False or real is not True:
        return here, None
    return here, (-b - mp.sqrt(b * b - a * c)) / a


def ref_ground(o, d):
    if o[2] < 0:
        return "inside", mp.mpf(0), ZERO3
    if d[2] < 0:
        return "hit", o[2] / -d[2], [mp.mpf(0), mp.mpf(0), mp.mpf(1)]
    return "miss", None, None


def ref_sphere(c, side, o, d):
    w, r = _sub(o, c), side[0] / 2
    inside = lt3(_dot(w, w), r * r)
    if inside is None:
        return None, None, None
    if inside:
        return "inside", mp.mpf(0), ZERO3
    here, t = _ball(w, d, r)
    if here is None:
        return None, None, None
    if not here:
        return "miss", None, None
    return "hit", t, _unit(_axpy(t, d, w))


def ref_box(c, R, side, o, d):
    w = _sub(o, c)
    size = mp.sqrt(_dot(side, side)) / 2
    dn, wn = mp.sqrt(_dot(d, d)), mp.sqrt(_dot(w, w))
    tscale = (wn + size) / dn                                 # what a t is compared with 0 against
    near, far, undecided = [], [], False
    for k in range(3):
        col = [R[k], R[3 + k], R[6 + k]]
        p, q, h = _dot(col, w), _dot(col, d), side[k] / 2
        if q == 0:
            out = lt3(h, abs(p))
            if out is None:
                undecided = True
            elif out:
                return "miss", None, None
            continue
        if abs(q) < GUARD * dn:
            undecided = True
        ta, tb = (-h - p) / q, (h - p) / q
        near.append((min(ta, tb), k, q))
        far.append(max(ta, tb))
    if not near:
        return (None, None, None) if undecided else ("inside", mp.mpf(0), ZERO3)
    tin, kin, qin = max(near, key=lambda x: (x[0], -x[1]))    # lowest k on an exact tie
    tout = min(far)
    hit = and3(le3(tin, tout, max(abs(tin), abs(tout), tscale)), lt3(0, tout, tscale))
    if hit is False:
        return "miss", None, None
    inside = lt3(tin, 0, tscale)
    if undecided or hit is None or inside is None:
        return None, None, None
    if inside:
        return "inside", mp.mpf(0), ZERO3
    for t2, k2, _ in near:                                    # an edge or a corner: which face is a close call
        if k2 != kin and t2 != tin and abs(t2 - tin) < GUARD * max(abs(tin), tscale):
            return None, None, None
    sg = -1 if qin > 0 else 1
    return "hit", tin, [sg * R[kin], sg * R[3 + kin], sg * R[6 + kin]]


def ref_capsule(c, R, side, o, d):
    u = [R[2], R[5], R[8]]
    uu = _dot(u, u)
    r, e = side[0] / 2, (side[2] - side[0]) / 2
    w = _sub(o, c)
    wu, du = _dot(w, u) / uu, _dot(d, u) / uu                 # axial coordinates, in units of u
    s = max(-e, min(e, wu))
    v = _axpy(-s, u, w)
    inside = lt3(_dot(v, v), r * r)
    if inside is None:
        return None, None, None
    if inside:
        return "inside", mp.mpf(0), ZERO3
    cands = []                                                # (present3, t, normal)
    wp, dp = _axpy(-wu, u, w), _axpy(-du, u, d)
    a, dd = _dot(dp, dp), _dot(d, d)
    if a != 0:
        side3 = None if a < GUARD * GUARD * dd else True     # all but parallel to the axis: a close call
        b, cc = _dot(wp, dp), _dot(wp, wp) - r * r
        real = le3(a * cc, b * b)
        if real is True and side3:
            ts = (-b - mp.sqrt(b * b - a * cc)) / a
            tscale = (mp.sqrt(_dot(w, w)) + e + r) / mp.sqrt(dd)
            ax = wu + ts * du
            side3 = and3(le3(0, ts, tscale), le3(-e, ax, e), le3(ax, e, e))
            cands.append((side3, ts, _unit(_axpy(ts, dp, wp)) if side3 is not False else None))
        elif real is None or side3 is None:
            cands.append((None, None, None))
    for end in (-e, e):
        wb = _sub(o, _axpy(end, u, c))
        here, t = _ball(wb, d, r)
        cands.append((here, t, _unit(_axpy(t, d, wb)) if here else None))
    if any(p is None for p, _, _ in cands):
        return None, None, None
    live = [(t, k, n) for k, (p, t, n) in enumerate(cands) if p]
    if not live:
        return "miss", None, None
    t, k, n = min(live, key=lambda x: (x[0], x[1]))
    for t2, k2, n2 in live:                                   # two parts all but tied: which normal is a close call,
        if k2 != k and t2 != t and abs(t2 - t) < GUARD * max(abs(t), 1):   # unless they agree (the seam)
            if max(abs(x - y) for x, y in zip(n, n2)) > mp.mpf("1e-9"):
                return None, None, None
    return "hit", t, n


def cast_one(pos, R, side, shape, o, d, tmax, skip=-1):
    """(kind, body, t, normal) of one world-frame ray; kind None = undecided."""
    with mp.workdps(DPS):
        o, d = _v(o), _v(d)
        tm = mp.inf if np.isinf(tmax) else mp.mpf(float(tmax))
        dd = _dot(d, d)
        found = [(GROUND,) + ref_ground(o, d)]
        for j in range(len(pos)):
            if j == skip:
                continue
            c, sj = _v(pos[j]), _v(side[j])
            sh = BOX if shape is None else int(shape[j])
            # a shortcut of the mathematics, not of the device: a line that passes the centre at more than twice the
            # bounding radius misses
            w = _sub(o, c)
            b2 = _dot(sj, sj) / 4 if sh == BOX else (sj[0] * sj[0] / 4 if sh == SPHERE else sj[2] * sj[2] / 4)
            wd = _dot(w, d)
            if _dot(w, w) - wd * wd / dd > 4 * b2:
                continue
            if sh == BOX:
                got = ref_box(c, _v(R[j]), sj, o, d)
            elif sh == SPHERE:
                got = ref_sphere(c, sj, o, d)
            else:
                got = ref_capsule(c, _v(R[j]), sj, o, d)
            found.append((j,) + got)
        if any(k is None for _, k, _, _ in found):
            return None, MISS, None, None
        for body, kind, t, n in found:                         # ground first, then by index
            if kind == "inside":
                return "inside", body, mp.mpf(0), ZERO3
        hits = sorted(((t, body, n) for body, kind, t, n in found if kind == "hit"), key=lambda x: (x[0], x[1]))
        if not hits:
            return "miss", MISS, tm, ZERO3
        t, body, n = hits[0]
        if len(hits) > 1 and hits[1][0] != t and abs(hits[1][0] - t) < GUARD * max(abs(t), 1):
            return None, MISS, None, None
        reach = le3(t, tm) if tm != mp.inf else True
        if reach is None:
            return None, MISS, None, None
        return ("hit", body, t, n) if reach else ("miss", MISS, tm, ZERO3)


# ---- families -------------------------------------------------------------------------------------------------------

def _rot(rng, n):
    return Rotation.random(n, random_state=int(rng.integers(1 << 30))).as_matrix().reshape(n, 9)


def _dirn(rng, down=True):
    v = rng.normal(size=3)
    v /= np.linalg.norm(v)
    if down:
        v[2] = -abs(v[2])
    return v


def _perp(rng, v):
    p = np.cross(v, rng.normal(size=3))
    return p / np.linalg.norm(p)


def _ray(rng, through, dirn, back):
    """A ray along dirn (scaled: d is not a unit vector) that passes through `through` after `back` metres."""
    return through - back * dirn, dirn * rng.uniform(0.5, 3.0)


def _ground(rng):
    o, d = np.zeros((64, 3)), np.zeros((64, 3))
    for k in range(64):
        o[k] = [rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(0.1, 3.0)]
        d[k] = _dirn(rng, down=False) * rng.uniform(0.5, 3.0)
        kind = k // 16
        if kind == 0:
            d[k, 2] = -abs(d[k, 2])
        elif kind == 1:
            d[k, 2] = 0.0
        elif kind == 2:
            d[k, 2] = abs(d[k, 2])
        else:
            o[k, 2] = -o[k, 2]
    o[16, 2] = 0.0          # level ON the plane, and down from the plane: not inside, the second a hit at t = 0
    o[0, 2] = 0.0
    return dict(pos=np.zeros((0, 3)), R=np.zeros((0, 9)), side=np.zeros((0, 3)), shape=np.zeros(0, np.int32), origin=o, dir=d,
                tmax=np.full(64, np.inf))


def _sphere(rng):
    n = 64
    pos = np.array([[SPACING * k, 0.0, rng.uniform(1.5, 2.0)] for k in range(n)])
    dia = rng.uniform(0.2, 0.5, n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n):
        r, c = dia[k] / 2, pos[k]
        v = _dirn(rng)
        p = _perp(rng, v)
        if k < 16:      # hits
            o[k], d[k] = _ray(rng, c + rng.uniform(0, 0.9) * r * p, v, rng.uniform(2, 5) * r)
        elif k < 24:    # misses
            o[k], d[k] = _ray(rng, c + rng.uniform(1.2, 3.0) * r * p, v, rng.uniform(2, 5) * r)
        elif k < 32:    # origins inside
            o[k], d[k] = c + rng.uniform(0, 0.9) * r * p, _dirn(rng, down=False) * rng.uniform(0.5, 3.0)
        elif k < 48:    # origins 100 r away: 12 hits, 4 misses
            o[k], d[k] = _ray(rng, c + (rng.uniform(0, 0.9) if k < 44 else 1.5) * r * p, v, 100 * r)
        else:           # grazing: the perpendicular offset is r (1 -+ delta)
            delta = 10 ** rng.uniform(-7, -5) * (1 if k % 2 else -1)
            o[k], d[k] = _ray(rng, c + r * (1 + delta) * p, v, rng.uniform(2, 5) * r)
    return dict(pos=pos, R=_rot(rng, n), side=np.repeat(dia[:, None], 3, axis=1), shape=np.full(n, SPHERE, np.int32),
                origin=o, dir=d, tmax=np.full(n, np.inf))


def _box(rng):
    n = 64
    pos = np.array([[SPACING * k, 0.0, 2.0] for k in range(n)])
    R = _rot(rng, n)
    side = rng.uniform(0.2, 0.8, (n, 3))
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n):
        h, c = side[k] / 2, pos[k]
        if 36 <= k < 52:
            R[k] = np.eye(3).reshape(9)
        M = R[k].reshape(3, 3)
        if k < 20:      # face hits: through a point well inside
            o[k], d[k] = _ray(rng, c + M @ (rng.uniform(-0.8, 0.8, 3) * h), _dirn(rng), 2.0)
        elif k < 36:    # past an edge (k < 28) or a corner, cutting it by delta or missing it by delta
            sg = rng.choice([-1.0, 1.0], 3)
            delta = 10 ** rng.uniform(-7, -5) * h.min() * (1 if k % 2 else -1)
            if k < 28:
                ax = int(rng.integers(3))
                e = sg * h
                e[ax] = rng.uniform(-0.8, 0.8) * h[ax]
                out = sg.copy(); out[ax] = 0.0
                v = rng.uniform(0.3, 1.0, 3) * sg
                v[(ax + 1) % 3] *= -1                          # mixed signs across the edge: the line only touches it
            else:
                e, out = sg * h, sg.copy()
                v = rng.uniform(0.3, 1.0, 3) * sg
                v[int(rng.integers(3))] *= -1
            out /= np.linalg.norm(out)
            v = M @ (v / np.linalg.norm(v))
            if v[2] > 0:
                v = -v
            o[k], d[k] = _ray(rng, c + M @ (e + delta * out), v, 2.0)
        elif k < 52:    # R = I, one (k < 44) or two box-frame components exactly 0; every other one passes beside the box
            v = _dirn(rng)
            zero = [int(rng.integers(2))] if k < 44 else [0, 1]
            v[zero] = 0.0
            v /= np.linalg.norm(v)
            q = rng.uniform(-0.8, 0.8, 3) * h
            if k % 2:
                q[zero[0]] = rng.uniform(1.2, 2.0) * h[zero[0]]
            o[k], d[k] = _ray(rng, c + q, v, 1.5)
        else:           # origins inside
            o[k], d[k] = c + M @ (rng.uniform(-0.8, 0.8, 3) * h), _dirn(rng, down=False) * rng.uniform(0.5, 3.0)
    return dict(pos=pos, R=R, side=side, shape=np.full(n, BOX, np.int32), origin=o, dir=d, tmax=np.full(n, np.inf))


def _capsule(rng):
    n = 64
    pos = np.array([[SPACING * k, 0.0, 2.0] for k in range(n)])
    R = _rot(rng, n)
    dia = rng.uniform(0.2, 0.4, n)
    side = np.stack([dia, dia, dia + rng.uniform(0.3, 0.8, n)], axis=1)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n):
        if 40 <= k < 48:
            R[k] = np.eye(3).reshape(9)
        c, r, e = pos[k], side[k, 0] / 2, (side[k, 2] - side[k, 0]) / 2
        u = R[k].reshape(3, 3)[:, 2]
        p = _perp(rng, u)
        if p[2] < 0:
            p = -p                                             # rays come from above
        if k < 14:      # side hits, across the axis
            v = -p + rng.uniform(-0.3, 0.3) * u
            v /= np.linalg.norm(v)
            o[k], d[k] = _ray(rng, c + rng.uniform(-0.8, 0.8) * e * u + rng.uniform(-0.8, 0.8) * r * np.cross(u, p), v, 2.0)
        elif k < 30:    # the end balls: end 0 (k < 22), end 1
            sg = -1.0 if k < 22 else 1.0
            v = -sg * u + rng.uniform(-0.5, 0.5) * p
            v /= np.linalg.norm(v)
            if v[2] > 0.5:
                v = v - 2 * v[2] * np.array([0, 0, 1.0])       # mirrored: still onto the cap, from above
            o[k], d[k] = _ray(rng, c + sg * (e + 0.5 * r) * u, v, 1.5)
        elif k < 40:    # the seam: radially inwards at the axial coordinate +-e (1 -+ delta)
            sg = -1.0 if k % 2 else 1.0
            delta = 10 ** rng.uniform(-3, -2) * (1 if (k // 2) % 2 else -1)   # 1e-3 .. 1e-2: the side's and the ball's t differ by (e delta)^2 / 2 r
            o[k], d[k] = _ray(rng, c + sg * e * (1 + delta) * u + r * p, -p, 1.0)
        elif k < 48:    # R = I, exactly along the axis direction: on the axis (k < 44) or beside it
            off = np.zeros(3) if k < 44 else np.array([rng.uniform(-0.6, 0.6) * r, rng.uniform(-0.6, 0.6) * r, 0.0])
            up = 1.0 if k % 2 else -1.0
            o[k] = c + off + np.array([0.0, 0.0, up * 1.5])
            d[k] = np.array([0.0, 0.0, -up * rng.uniform(0.5, 3.0)])
        elif k < 56:    # onto the infinite cylinder beyond an end: a miss of the capsule
            sg = -1.0 if k % 2 else 1.0
            o[k], d[k] = _ray(rng, c + sg * (e + rng.uniform(1.5, 3.0) * r) * u + rng.uniform(-0.5, 0.5) * r * np.cross(u, p), -p, 1.0)
        else:           # origins inside: the cylinder, and the end balls beyond +-e
            s = rng.uniform(-1, 1) * e if k < 60 else (1 if k % 2 else -1) * (e + 0.5 * r)
            o[k], d[k] = c + s * u + rng.uniform(0, 0.4) * r * p, _dirn(rng, down=False) * rng.uniform(0.5, 3.0)
    return dict(pos=pos, R=R, side=side, shape=np.full(n, CAPSULE, np.int32), origin=o, dir=d, tmax=np.full(n, np.inf))


def _heap(rng):
    """The 12-body mixed scene of test_gpu_collide_capsules.mixed_scene under a 16 x 16 fan from one point above it."""
    from test_gpu_collide_capsules import mixed_scene
    p, R, side, shape = mixed_scene()
    eye = np.array([0.45, 0.24, 1.5])
    gx, gy = np.meshgrid(np.linspace(-0.3, 1.2, 16), np.linspace(-0.3, 0.8, 16))
    target = np.stack([gx.ravel(), gy.ravel(), np.zeros(256)], axis=1) + rng.uniform(-0.01, 0.01, (256, 3)) * [1, 1, 0]
    return dict(pos=p, R=R, side=side, shape=shape, origin=np.tile(eye, (256, 1)), dir=target - eye, tmax=np.full(256, np.inf))


def _ties(rng):
    """Bodies 0 and 1: the same sphere twice; body 2: a ball resting on the ground at one point; body 3: a box."""
    pos = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [SPACING, 0.0, 0.25], [2 * SPACING, 0.0, 1.0]])
    side = np.array([[0.4] * 3, [0.4] * 3, [0.5] * 3, [0.6, 0.4, 0.5]])
    shape = np.array([SPHERE, SPHERE, SPHERE, BOX], np.int32)
    R = _rot(rng, 4)
    o, d, tmax = np.zeros((64, 3)), np.zeros((64, 3)), np.full(64, np.inf)
    for k in range(64):
        if k < 16:      # the twin spheres: the lowest index wins
            v = _dirn(rng)
            o[k], d[k] = _ray(rng, pos[0] + rng.uniform(0, 0.9) * 0.2 * _perp(rng, v), v, 1.0)
        elif k < 32:    # from the touching point itself, downwards: the ground at t = 0, the ball is left behind
            o[k], d[k] = np.array([SPACING, 0.0, 0.0]), _dirn(rng) * rng.uniform(0.5, 3.0)
        else:           # tmax just below (even k) and just above the hit: sphere 0, the ball, the box, the ground
            v = _dirn(rng)
            aim = [pos[0], pos[2], pos[3], np.array([3 * SPACING, 1.0, 0.0])][(k // 2) % 4]
            o[k], d[k] = _ray(rng, aim + 0.05 * _perp(rng, v), v, 1.5)
    fam = dict(pos=pos, R=R, side=side, shape=shape, origin=o, dir=d, tmax=tmax)
    for k in range(32, 64):
        kind, _, t, _ = cast_one(pos, R, side, shape, o[k], d[k], np.inf)
        assert kind == "hit"
        tmax[k] = float(t) * (1 + (1e-7 if k % 2 else -1e-7))
    return fam


_BUILD = {"ground": _ground, "sphere": _sphere, "box": _box, "capsule": _capsule, "heap": _heap, "ties": _ties}


@functools.lru_cache(maxsize=None)
def family(name):
    """dict(pos, R, side, shape, origin, dir, tmax), read-only, one device call per family."""
    fam = _BUILD[name](np.random.default_rng(1000 + FAMILIES.index(name)))
    for a in fam.values():
        a.setflags(write=False)
    return fam


@functools.lru_cache(maxsize=None)
def family_reference(name):
    """[(kind, body, t, normal)] per ray, computed once per process and shared."""
    f = family(name)
    return [cast_one(f["pos"], f["R"], f["side"], f["shape"], f["origin"][i], f["dir"][i], f["tmax"][i])
            for i in range(len(f["origin"]))]


def left_out(name):
    return sum(1 for r in family_reference(name) if r[0] is None)


def check_family(name, hit, t, normal):
    """Asserts the decision of every case not left out; returns (worst error, cases left out).  The error is the
    larger of |dt| |d| (metres along the ray) and the normal's largest component error."""
    f, refs = family(name), family_reference(name)
    worst = 0.0
    with mp.workdps(DPS):
        for i, (kind, body, rt, rn) in enumerate(refs):
            if kind is None:
                continue
            who = "%s[%d]" % (name, i)
            assert int(hit[i]) == body, "%s: body %d, the reference says %s %d" % (who, hit[i], kind, body)
            if kind != "hit":
                want_t = 0.0 if kind == "inside" else f["tmax"][i]
                assert t[i] == want_t and not normal[i].any(), "%s: %s reported as t = %r, normal %r" % (who, kind, t[i], normal[i])
                continue
            dn = mp.sqrt(_dot(_v(f["dir"][i]), _v(f["dir"][i])))
            err = max([abs(mp.mpf(float(t[i])) - rt) * dn] + [abs(mp.mpf(float(normal[i][k])) - rn[k]) for k in range(3)])
            worst = max(worst, float(err))
    return worst, left_out(name)
