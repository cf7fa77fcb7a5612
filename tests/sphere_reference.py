"""Sphere contact geometry as mathematics, in mpmath at 50 digits on the exact fp64 inputs: an INDEPENDENT reference
for what tests/sphere_twin.py restates in fp64 and collide.hip mirrors bit for bit.  Nothing here follows the device's
operation order.

A sphere is (centre c, diameter d), r = d / 2; a box is (centre c, row-major R whose COLUMNS are its axes, sides),
h = side / 2.  body0 < body1 or body0 = ground; the normal points from body0 towards body1; depth >= 0.

  ground    q = (c_x, c_y, c_z - r); contact iff q_z < 0: (q, (0,0,1), -q_z)
  spheres   d = c_j - c_i, L = |d|, s = L - (r_i + r_j); contact iff s <= 0; n = d / L; depth = -s;
            position c_i + n (r_i + L - r_j) / 2
  box       p = R^T (c_S - c_B), q = clamp(p, -h, h).  Outside (q != p): e = p - q, L = |e|, s = L - r, contact iff
            s <= 0, n_BS = R e / L, depth = -s, box point R q + c_B.  Inside: g_k = h_k - |p_k|, k = argmin g,
            n_BS = sgn(p_k) R[:, k], depth = g_k + r (s = -depth), box point = the centre moved onto face k.
            Sphere point c_S - r n_BS; position = the midpoint; normal n_BS if the box is body0, else -n_BS.

Guard bands.  A case is left out of a property, and COUNTED, when the deciding quantity is a close call in fp64:
|s| < 1e-9 for contact / no contact; L < 1e-9 for the normal's direction (then position too, which rides on it);
inside, the two smallest g_k within 1e-9 of each other (normal, depth's face, position); |q_z| < 1e-12 for the ground.
No family may leave out more than 10 % of its cases.

Tolerance: TOL = 1e-12 absolute of tests/collision_reference.py, the project's bound for short fp64 chains on
quantities of order 1, on normal, depth and position.

The seeded families at the end are shared by the CPU test (twin against this reference) and the GPU test (device
against the twin and this reference): 64 cases each, case k standing alone around x = 2 k so that one device call
takes a whole family.  Their references are computed once per process."""
import functools

import mpmath as mp
import numpy as np
from scipy.spatial.transform import Rotation

from collision_reference import TOL

DPS = 50
GUARD = mp.mpf("1e-9")
GUARD_Z = mp.mpf("1e-12")
MAX_LEFT_OUT = 0.10
BOX, SPHERE = 0, 1
CASES = 64
SPACING = 2.0


def _v(a):
    if isinstance(a, (list, tuple)) and all(isinstance(x, mp.mpf) for x in a):
        return list(a)
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _col(R, k):
    return [R[k], R[3 + k], R[6 + k]]


def _axpy(a, x, y):
    return [a * x[k] + y[k] for k in range(3)]


def sphere_ground(c, d):
    """dict(contact, qz, row) for a sphere above the ground plane z = 0."""
    with mp.workdps(DPS):
        c, r = _v(c), _v([d])[0] / 2
        qz = c[2] - r
        return dict(contact=qz < 0, s=qz, guard_s=abs(qz) < GUARD_Z, row=[c[0], c[1], qz, mp.mpf(0), mp.mpf(0), mp.mpf(1), -qz])


def sphere_sphere(ci, di, cj, dj):
    with mp.workdps(DPS):
        ci, cj = _v(ci), _v(cj)
        ri, rj = _v([di])[0] / 2, _v([dj])[0] / 2
        d = [cj[k] - ci[k] for k in range(3)]
        L = mp.sqrt(_dot(d, d))
        s = L - (ri + rj)
        n = [x / L for x in d] if L != 0 else [mp.mpf(0), mp.mpf(0), mp.mpf(1)]
        a = _axpy(ri, n, ci)                 # surface point of i towards j
        b = _axpy(-rj, n, cj)                # surface point of j towards i
        pos = [(a[k] + b[k]) / 2 for k in range(3)]
        return dict(contact=s <= 0, s=s, guard_s=abs(s) < GUARD, guard_n=L < GUARD, row=pos + n + [-s])


def sphere_box(cS, dS, cB, RB, sideB):
    """The normal is n_BS (box towards sphere)."""
    with mp.workdps(DPS):
        cS, cB, R, h = _v(cS), _v(cB), _v(RB), [x / 2 for x in _v(sideB)]
        r = _v([dS])[0] / 2
        ax = [_col(R, k) for k in range(3)]
        rel = [cS[k] - cB[k] for k in range(3)]
        p = [_dot(ax[k], rel) for k in range(3)]
        q = [max(-h[k], min(h[k], p[k])) for k in range(3)]
        inside = q == p
        if not inside:
            e = [p[k] - q[k] for k in range(3)]
            L = mp.sqrt(_dot(e, e))
            s = L - r
            n = [sum(ax[k][a] * e[k] for k in range(3)) / L for a in range(3)]
            guard_n = L < GUARD
        else:
            g = [h[k] - abs(p[k]) for k in range(3)]
            k = min(range(3), key=lambda a: (g[a], a))
            order = sorted(g)
            guard_n = order[1] - order[0] < GUARD
            sg = 1 if p[k] >= 0 else -1
            n = [sg * x for x in ax[k]]
            s = -(g[k] + r)
            q[k] = sg * h[k]
        boxpt = [sum(ax[k][a] * q[k] for k in range(3)) + cB[a] for a in range(3)]
        sphpt = _axpy(-r, n, cS)
        pos = [(boxpt[k] + sphpt[k]) / 2 for k in range(3)]
        return dict(contact=s <= 0, s=s, guard_s=abs(s) < GUARD, guard_n=guard_n, inside=inside, row=pos + n + [-s])


def pair(pos, R, side, shape, i=0, j=1):
    """The reference of bodies i < j of which at least one is a sphere, with the reported normal (body0 -> body1)."""
    if shape[i] == SPHERE and shape[j] == SPHERE:
        return sphere_sphere(pos[i], side[i][0], pos[j], side[j][0])
    if shape[i] == SPHERE:
        out = sphere_box(pos[i], side[i][0], pos[j], R[j], side[j])
        with mp.workdps(DPS):
            out["row"] = out["row"][:3] + [-x for x in out["row"][3:6]] + out["row"][6:]
        return out
    return sphere_box(pos[j], side[j][0], pos[i], R[i], side[i])


def compare(ref, rows, left_out):
    """rows = what the code under test reports for the case of `ref` ([] or one [7] row).  Asserts the decision exactly
    outside its guard band and normal, depth, position within TOL outside theirs; adds what it left out to left_out
    (a dict of counters).  Returns the largest error seen."""
    assert len(rows) <= 1
    if ref["guard_s"]:
        left_out["decision"] = left_out.get("decision", 0) + 1
        if len(rows) != int(ref["contact"]):
            return 0.0      # the close call went the other way: nothing to compare
    else:
        assert len(rows) == int(ref["contact"]), ("contact / no contact", ref["s"])
    if not rows:
        return 0.0
    got = [mp.mpf(float(x)) for x in rows[0]]
    err = abs(got[6] - ref["row"][6])                       # depth: |n| = 1 whichever direction
    if ref.get("guard_n", False):
        left_out["normal"] = left_out.get("normal", 0) + 1
        if ref.get("inside", False):                           # the depth of an inside case rides on the face chosen
            return 0.0
        assert err <= TOL, ("depth", float(err))
        return float(err)
    err = max([err] + [abs(got[k] - ref["row"][k]) for k in range(6)])
    assert err <= TOL, ("row", float(err), [float(got[k] - ref["row"][k]) for k in range(7)])
    return float(err)


# ---- seeded case families ------------------------------------------------------------------------------------------
FAMILIES = ("ground", "spheres", "face", "edge", "corner", "inside", "near_miss")
_SEEDS = dict(ground=11, spheres=12, face=13, edge=14, corner=15, inside=16, near_miss=17)


def _rot(rng, n):
    return Rotation.random(n, random_state=int(rng.integers(1 << 30))).as_matrix().reshape(n, 9)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def family(name):
    """dict(pos [n][3], R [n][9], side [n][3], shape [n], pairs [(i, j)] or None for the ground family): CASES cases,
    case k around x = SPACING * k and well above the ground unless the family is about it."""
    rng = np.random.default_rng(_SEEDS[name])
    pos, R, side, shape, pairs = [], [], [], [], []
    eye = np.eye(3).reshape(9)
    for k in range(CASES):
        o = np.array([SPACING * k, 0.0, 3.0])
        if name == "ground":
            d = rng.uniform(0.1, 0.5)
            dz = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-8, -1.5)      # just in, just out, deep, clear
            pos.append([o[0], rng.uniform(-0.3, 0.3), d / 2 + dz]); R.append(_rot(rng, 1)[0]); side.append([d] * 3)
            shape.append(SPHERE)
            continue
        pairs.append((2 * k, 2 * k + 1))
        if name == "spheres" or (name == "near_miss" and k % 2 == 0):
            di, dj = rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5)
            if name == "spheres":
                s = rng.choice([-1.0, 1.0], p=[0.75, 0.25]) * 10.0 ** rng.uniform(-7, -1.3)
            else:
                s = 10.0 ** rng.uniform(-6, -3)
            c = o + rng.uniform(-0.2, 0.2, 3)
            pos += [c, c + _unit(rng) * ((di + dj) / 2 + s)]
            R += [_rot(rng, 1)[0], _rot(rng, 1)[0]]; side += [[di] * 3, [dj] * 3]; shape += [SPHERE, SPHERE]
            continue
        # a sphere and a rotated box with unequal sides; the sphere's centre is given in the box's frame
        sb = rng.uniform(0.15, 0.6, 3)
        h = sb / 2
        d = rng.uniform(0.1, 0.5)
        RB = _rot(rng, 1)[0]
        cB = o + rng.uniform(-0.2, 0.2, 3)
        if name == "inside":
            p = rng.uniform(-1, 1, 3) * h
        else:
            region = dict(face=1, edge=2, corner=3).get(name, 1 + k % 3)
            out = rng.permutation(3)[:region]
            e = np.zeros(3)
            e[out] = rng.uniform(0.2, 1.0, region) * rng.choice([-1.0, 1.0], region)
            e /= np.linalg.norm(e)
            if name == "near_miss":
                s = 10.0 ** rng.uniform(-6, -3)
            else:
                s = rng.choice([-1.0, 1.0], p=[0.75, 0.25]) * 10.0 ** rng.uniform(-7, -1.3)
            p = rng.uniform(-1, 1, 3) * h
            p[out] = np.sign(e[out]) * h[out]
            p = p + e * (d / 2 + s)
        cS = cB + RB.reshape(3, 3) @ p
        if rng.uniform() < 0.5:     # the sphere is body0
            pos += [cS, cB]; R += [_rot(rng, 1)[0], RB]; side += [[d] * 3, sb]; shape += [SPHERE, BOX]
        else:
            pos += [cB, cS]; R += [RB, _rot(rng, 1)[0]]; side += [sb, [d] * 3]; shape += [BOX, SPHERE]
    return dict(pos=np.array(pos, np.float64), R=np.array(R, np.float64), side=np.array(side, np.float64),
                shape=np.array(shape, np.int32), pairs=pairs or None)


@functools.lru_cache(maxsize=None)
def family_reference(name):
    """The reference of every case of the family, in case order."""
    f = family(name)
    if name == "ground":
        return [sphere_ground(f["pos"][b], f["side"][b][0]) for b in range(CASES)]
    return [pair(f["pos"], f["R"], f["side"], f["shape"], i, j) for i, j in f["pairs"]]


def check_family(name, b0, b1, data):
    """A contact list of the whole family (twin's or device's) against the reference, case by case; returns
    (largest error, left-out counters) after asserting that no property left out more than MAX_LEFT_OUT of the cases."""
    f, refs = family(name), family_reference(name)
    left_out, worst, seen = {}, 0.0, 0
    for k, ref in enumerate(refs):
        if name == "ground":
            sel = (b0 == -1) & (b1 == k)
        else:
            i, j = f["pairs"][k]
            sel = (b0 == i) & (b1 == j)
        seen += int(sel.sum())
        worst = max(worst, compare(ref, list(data[sel]), left_out))
    assert seen == len(b0), "contacts outside the family's cases"
    for what, c in left_out.items():
        assert c <= MAX_LEFT_OUT * CASES, (name, what, c)
    return worst, left_out
