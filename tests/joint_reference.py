"""The angular joint blocks (EGS_JOINT_LOCK, EGS_JOINT_HINGE_AXIS) and the hinge motor as mathematics and as an fp64 twin.

The reference extends tests/model_reference.py (imported unchanged; it knows the ball joint and the contact) in mpmath
at 50 digits, from the exact fp64 inputs:

  lock         E = R0 Rq R1^T (R1 = I for a world side), Rq the rotation matrix of the stored quaternion (the polynomial
               form, so a quaternion that is unit only to rounding is taken as it stands)
               err = axial vector of E = (E21 - E12, E02 - E20, E10 - E01) / 2  (= sin(theta) n for E = exp(theta [n]x))
               J0 = [0 | I], J1 = [0 | -I]
  hinge axis   s = R0 a0, t = R1 a1 (a1 itself for a world side), Rn = the shortest arc taking s^ to z, rows (p, q, s^)
               c = t x s, err = (p.c, q.c, 0), J0 = [0 | Rn], J1 = [0 | -Rn]
  motor        a hinge with tau >= 0: lo[2] = -tau, hi[2] = tau, rhs[2] = speed / dt - J row 2 . (v/dt + M^-1 f)

That d err/dt = J0 s0 + J1 s1 at err = 0 is checked, not assumed: test_joint_reference_cpu.py moves both bodies by the
exact rigid motion and differences err.

Tolerances, in units of u = 2^-53, from the lengths of the product sums the fp64 code forms (a k-term product sum of
exact inputs is within k u of its magnitude sum, taken here as (k + 1) u to cover the second-order terms; an input
error d moves it by at most the other factor's magnitude times d):

  Rq entries          4u mag          (two products or squares, one or two additions)
  T = R0 Rq           4u mag + |R0| dRq
  E = T R1^T          4u mag + dT |R1^T|
  lock err            u |E_a - E_b| / 2 + (dE_a + dE_b) / 2
  s, t                4u mag
  Rn entries          64u / (1 + c)  [model_reference's bound for an exact argument]  + 20 ds / (1 + c)
                      Rn = [[1 - x^2/k, -xy/k, -x], [-xy/k, 1 - y^2/k, -y], [x, y, z]] with s^ = (x, y, z), k = 1 + z;
                      |x|, |y| <= sqrt(2k), so each entry's gradient in s^ has 1-norm at most (4 + 4 + 2) / k, and
                      normalising s (|s| = 1 to rounding) at most doubles its error ds
  c = t x s           3u mag + |t| ds + dt |s|
  hinge err           4u mag + |Rn row| dc + dRn |c|_1
  rhs rows            model_reference's: 32u mag + (J tolerance of the row) |v/dt + M^-1 f|_1, plus (erp / dt^2) times
                      the tolerance of an angular err (which is absolute, not 8u of err's own size as a ball joint's
                      is); the motor's speed / dt is one more term of the row

A tolerance of zero means "these bits": the zero linear columns, the lock's +-I, err[2] of a hinge, the bounds, the
row types.

The twin restates the device's operation order (include/eggshell_amd.h, assemble_device.h) in plain Python floats,
which never contract a multiply and an add; neither kind uses a trigonometric function, so it is the device's bits.
The generators redraw any case whose hinge axis s lies within model_reference.BRANCH of the antiparallel-to-z switch of
align_to_z, so no case has to be skipped."""
import math

import mpmath as mp
import numpy as np

import model_reference as mr

BALL, CONTACT, LOCK, HINGE = 0, 1, 2, 3
U = mr.U


# ---- the reference ---------------------------------------------------------------------------------------------------------
def quat_matrix(q):
    """(Rq, magnitude sums): the polynomial rotation matrix of q = (w, x, y, z), exact in the arithmetic of q."""
    w, x, y, z = q
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    a = [abs(v) for v in q]
    w, x, y, z = a
    M = [[1 + 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 + 2 * (x * x + z * z), 2 * (y * z + x * w)],
         [2 * (x * z + y * w), 2 * (y * z + x * w), 1 + 2 * (x * x + y * y)]]
    return R, M


def lock_reference(R0, R1, q):
    """(err [3], tolerance [3]) of a lock; R1 None: a world side.  All mpf."""
    Rq, Mq = quat_matrix(q)
    dRq = [[4 * U * Mq[i][j] for j in range(3)] for i in range(3)]
    T, Tm = mr._mul(R0, Rq), mr._absmul(R0, Rq)
    aR0 = [[abs(v) for v in row] for row in R0]
    dT = [[4 * U * Tm[i][j] + sum(aR0[i][k] * dRq[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    if R1 is None:
        E, dE = T, dT
    else:
        R1t = mr._T(R1)
        aR1t = [[abs(v) for v in row] for row in R1t]
        E, Em = mr._mul(T, R1t), mr._absmul(T, R1t)
        dE = [[4 * U * Em[i][j] + sum(dT[i][k] * aR1t[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    pairs = (((2, 1), (1, 2)), ((0, 2), (2, 0)), ((1, 0), (0, 1)))
    err = [(E[a[0]][a[1]] - E[b[0]][b[1]]) / 2 for a, b in pairs]
    tol = [U * abs(E[a[0]][a[1]] - E[b[0]][b[1]]) / 2 + (dE[a[0]][a[1]] + dE[b[0]][b[1]]) / 2 for a, b in pairs]
    return err, tol


def hinge_reference(R0, R1, a0, a1):
    """(err [3], its tolerance [3], Rn or None inside the branch, the tolerance of an Rn entry, 1 + c); R1 None: a world
    side.  All mpf."""
    s, sm = mr._mv(R0, a0), mr._absmv(R0, a0)
    ds = max(4 * U * x for x in sm)
    if R1 is None:
        t, dt = list(a1), mp.mpf(0)
    else:
        t, tm = mr._mv(R1, a1), mr._absmv(R1, a1)
        dt = max(4 * U * x for x in tm)
    Rn, sh, opc = mr.align_to_z(s)
    if Rn is None:
        return None, None, None, None, opc
    tRn = 64 * U / opc + 20 * ds / opc
    c = mr._cross(t, s)
    cm = [abs(t[1] * s[2]) + abs(t[2] * s[1]), abs(t[2] * s[0]) + abs(t[0] * s[2]), abs(t[0] * s[1]) + abs(t[1] * s[0])]
    t1, s1 = sum(abs(x) for x in t), sum(abs(x) for x in s)
    dc = [3 * U * cm[k] + t1 * ds + dt * s1 for k in range(3)]
    c1 = sum(abs(x) for x in c)
    err, tol = [], []
    for r in range(2):
        err.append(sum(Rn[r][k] * c[k] for k in range(3)))
        mag = sum(abs(Rn[r][k]) * abs(c[k]) for k in range(3))
        tol.append(4 * U * mag + sum(abs(Rn[r][k]) * dc[k] for k in range(3)) + tRn * c1)
    return err + [mp.mpf(0)], tol + [mp.mpf(0)], Rn, tRn, opc


def assemble_reference(case, pose=None):
    """mr.assemble_reference for a list of all four kinds: the ball joints and contacts from it, the angular blocks from
    the functions above.  Same dict (J0, J1, err as Checked; is_eq, lo, hi exact; branch).  The motor is applied by
    rhs_reference and motor_bounds."""
    kind = np.asarray(case["kind"])
    m = kind.shape[0]
    old = np.nonzero(kind <= CONTACT)[0]
    sub = dict(case)
    for k in ("kind", "body0", "body1", "data"):
        sub[k] = np.asarray(case[k])[old]
    base = mr.assemble_reference(sub, pose)
    with mp.workdps(mr.DPS):
        J = [mr.Checked(18 * m), mr.Checked(18 * m)]
        err = mr.Checked(3 * m)
        is_eq = np.zeros(3 * m, np.uint8)
        lo, hi = np.zeros(3 * m), np.zeros(3 * m)
        branch = np.zeros(m, bool)
        for k, i in enumerate(old):
            for s, name in enumerate(("J0", "J1")):
                for e in range(18):
                    J[s].put(18 * i + e, base[name].val[18 * k + e], base[name].mag[18 * k + e], base[name].tol[18 * k + e])
            for r in range(3):
                err.put(3 * i + r, base["err"].val[3 * k + r], base["err"].mag[3 * k + r], base["err"].tol[3 * k + r])
            is_eq[3 * i:3 * i + 3] = base["is_eq"][3 * k:3 * k + 3]
            lo[3 * i:3 * i + 3] = base["lo"][3 * k:3 * k + 3]
            hi[3 * i:3 * i + 3] = base["hi"][3 * k:3 * k + 3]
            branch[i] = base["branch"][k]
        R = [mr._m3(x) for x in case["R"]] if pose is None else pose[1]
        one, zero = mp.mpf(1), mp.mpf(0)
        for i in np.nonzero(kind > CONTACT)[0]:
            d = mr._v(case["data"][i])
            b0, b1 = int(case["body0"][i]), int(case["body1"][i])
            assert b0 >= 0
            R1 = R[b1] if b1 >= 0 else None
            if kind[i] == LOCK:
                e, tol = lock_reference(R[b0], R1, d[0:4])
                blk, btol = [[one if r == c else zero for c in range(3)] for r in range(3)], zero
                is_eq[3 * i:3 * i + 3] = 1
            else:
                e, tol, blk, btol, _ = hinge_reference(R[b0], R1, d[0:3], d[3:6])
                assert blk is not None, "hinge axis inside the antiparallel branch: the generators draw none"
                is_eq[3 * i:3 * i + 2] = 1
            for r in range(3):
                err.put(3 * i + r, e[r], abs(e[r]), tol[r])
                for c in range(3):
                    J[0].put(18 * i + 6 * r + 3 + c, blk[r][c], abs(blk[r][c]), btol)
                    if b1 >= 0:
                        J[1].put(18 * i + 6 * r + 3 + c, -blk[r][c], abs(blk[r][c]), btol)
        return dict(J0=J[0], J1=J[1], err=err, is_eq=is_eq, lo=lo, hi=hi, branch=branch, geo=None)


def motor_applies(case, motor, i):
    return motor is not None and case["kind"][i] == HINGE and float(motor[i][1]) >= 0


def motor_bounds(case, asm, motor):
    """(lo, hi) with the motor's torque limits on the axis rows."""
    lo, hi = asm["lo"].copy(), asm["hi"].copy()
    for i in range(case["kind"].shape[0]):
        if motor_applies(case, motor, i):
            lo[3 * i + 2], hi[3 * i + 2] = -float(motor[i][1]), float(motor[i][1])
    return lo, hi


def rhs_reference(case, asm, motor=None):
    """mr.rhs_reference with the motor target on the driven axis rows (err[2] of a hinge is 0: the target replaces a
    zero term).  No contact of the case may lie inside the antiparallel branch."""
    assert not asm["branch"].any()
    out = mr.rhs_reference(case, asm)
    with mp.workdps(mr.DPS):
        dt = mp.mpf(float(case["dt"]))
        kk = mp.mpf(float(case["erp"])) / (dt * dt)
        for i in range(case["kind"].shape[0]):
            if case["kind"][i] > CONTACT:      # an angular err is not within 8u of its own size: its tolerance, times erp / dt^2
                for k in range(3 * i, 3 * i + 3):
                    out.put(k, out.val[k], out.mag[k], out.tol[k] + kk * asm["err"].tol[k])
            if not motor_applies(case, motor, i):
                continue
            k = 3 * i + 2
            tgt = mp.mpf(float(motor[i][0])) / dt
            rest_of_tol = out.tol[k] - 32 * U * out.mag[k]
            mag = out.mag[k] + abs(tgt)
            out.put(k, out.val[k] + tgt, mag, 32 * U * mag + rest_of_tol)
    return out


# ---- the fp64 twin: the device's operation order in Python floats -------------------------------------------------------------
def _d3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _mv3(A, v):
    return [(A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2] for r in range(3)]


def _mm3(A, B):
    return [(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def _quat_to_R(w, x, y, z):
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def _align_to_z(a):
    na = _d3(a, a)
    if na > 0:
        s = math.sqrt(na)
        v0 = [a[0] / s, a[1] / s, a[2] / s]
    else:
        v0 = list(a)
    v1 = [0.0 / 1.0, 0.0 / 1.0, 1.0 / 1.0]
    c = _d3(v1, v0)
    if c < -1.0 + 1e-12:
        if c < -1.0:
            c = -1.0
        ax, ay, az = abs(v0[0]), abs(v0[1]), abs(v0[2])
        e = [0.0, 0.0, 0.0]
        if ax <= ay and ax <= az:
            e[0] = 1.0
        elif ay <= az:
            e[1] = 1.0
        else:
            e[2] = 1.0
        axis = [v0[1] * e[2] - v0[2] * e[1], v0[2] * e[0] - v0[0] * e[2], v0[0] * e[1] - v0[1] * e[0]]
        n = math.sqrt(_d3(axis, axis))
        axis = [axis[0] / n, axis[1] / n, axis[2] / n]
        w2 = (1.0 + c) * 0.5
        qw = math.sqrt(w2)
        sv = math.sqrt(1.0 - w2)
        q = [axis[0] * sv, axis[1] * sv, axis[2] * sv]
    else:
        axis = [v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]]
        s = math.sqrt((1.0 + c) * 2.0)
        invs = 1.0 / s
        q = [axis[0] * invs, axis[1] * invs, axis[2] * invs]
        qw = s * 0.5
    return _quat_to_R(qw, q[0], q[1], q[2])


def _dot6(a, b):
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]


def twin_block(kind, R0, R1, d):
    """(j0 [18], j1 [18], err [3], is_eq [3]) of one angular constraint; R0, R1 (None: a world side) [9], d [7]: floats."""
    j0, j1 = [0.0] * 18, [0.0] * 18
    if kind == LOCK:
        Rq = _quat_to_R(d[0], d[1], d[2], d[3])
        T = _mm3(R0, Rq)
        for r in range(3):
            j0[6 * r + 3 + r] = 1.0
        if R1 is not None:
            R1t = [R1[3 * c + r] for r in range(3) for c in range(3)]
            E = _mm3(T, R1t)
            for r in range(3):
                j1[6 * r + 3 + r] = -1.0 * 1.0
        else:
            E = T
        e = [0.5 * (E[7] - E[5]), 0.5 * (E[2] - E[6]), 0.5 * (E[3] - E[1])]
        return j0, j1, e, [1, 1, 1]
    s = _mv3(R0, d[0:3])
    t = _mv3(R1, d[3:6]) if R1 is not None else list(d[3:6])
    Rn = _align_to_z(s)
    c = [t[1] * s[2] - t[2] * s[1], t[2] * s[0] - t[0] * s[2], t[0] * s[1] - t[1] * s[0]]
    e = [_d3(Rn[0:3], c), _d3(Rn[3:6], c), 0.0]
    for r in range(3):
        for k in range(3):
            j0[6 * r + 3 + k] = Rn[3 * r + k]
            if R1 is not None:
                j1[6 * r + 3 + k] = -1.0 * Rn[3 * r + k]
    return j0, j1, e, [1, 1, 0]


def twin_assemble(case, motor=None, dt=None, erp=None):
    """The whole assembly in fp64 as the device makes it: dict of J0, J1 [m][18], err, lo, hi, rhs [3m], is_eq [3m].  The
    ball joints and contacts come from the CPU oracle (oracle/model.c, the device's bits for kinds 0 and 1), the angular
    blocks and every rhs row from the restatement here.  motor [m][2] or None.  dt / erp: scalars (default: the case's)
    or one value per constraint (the _each forms; dt 0: the constraint sits out, rhs rows exactly 0)."""
    from oracle import oracle as orc
    kind = np.asarray(case["kind"])
    m = kind.shape[0]
    old = np.nonzero(kind <= CONTACT)[0]
    J0, J1 = np.zeros((m, 18)), np.zeros((m, 18))
    err, lo, hi, rhs = np.zeros(3 * m), np.zeros(3 * m), np.zeros(3 * m), np.zeros(3 * m)
    is_eq = np.zeros(3 * m, np.uint8)
    if old.size:
        a = orc.assemble(case["p"], case["R"], kind[old], case["body0"][old], case["body1"][old], case["data"][old])
        rows = (3 * old[:, None] + np.arange(3)).reshape(-1)
        J0[old], J1[old] = np.asarray(a[0]).reshape(-1, 18), np.asarray(a[1]).reshape(-1, 18)
        is_eq[rows], lo[rows], hi[rows], err[rows] = a[2], a[3], a[4], np.asarray(a[5]).reshape(-1)
    R = np.asarray(case["R"], np.float64).reshape(-1, 9)
    for i in np.nonzero(kind > CONTACT)[0]:
        b0, b1 = int(case["body0"][i]), int(case["body1"][i])
        j0, j1, e, eq = twin_block(int(kind[i]), [float(x) for x in R[b0]], [float(x) for x in R[b1]] if b1 >= 0 else None,
                                   [float(x) for x in case["data"][i]])
        J0[i], J1[i], err[3 * i:3 * i + 3], is_eq[3 * i:3 * i + 3] = j0, j1, e, eq
    dts = np.broadcast_to(np.float64(case["dt"] if dt is None else dt), (m,)) if np.ndim(dt) == 0 else np.asarray(dt, np.float64)
    erps = np.broadcast_to(np.float64(case["erp"] if erp is None else erp), (m,)) if np.ndim(erp) == 0 else np.asarray(erp, np.float64)
    Minv, f = np.asarray(case["Minv"]).reshape(-1, 36), np.asarray(case["f_ext"]).reshape(-1, 6)
    for i in range(m):
        dti, erpi = float(dts[i]), float(erps[i])
        driven = motor_applies(case, motor, i)
        if driven:
            lo[3 * i + 2], hi[3 * i + 2] = -float(motor[i][1]), float(motor[i][1])
        if dti == 0.0:
            continue
        b = (int(case["body0"][i]), int(case["body1"][i]))
        u = [[0.0] * 6, [0.0] * 6]
        for side in range(2):
            if b[side] < 0:
                continue
            for r in range(6):
                vel = float(case["v"][b[side]][r] if r < 3 else case["w"][b[side]][r - 3])
                u[side][r] = vel / dti + _dot6([float(x) for x in Minv[b[side]][6 * r:6 * r + 6]], [float(x) for x in f[b[side]]])
        j0, j1 = [float(x) for x in J0[i]], [float(x) for x in J1[i]]
        kk = -erpi / dti / dti
        for r in range(3):
            ju = _dot6(j0[6 * r:6 * r + 6], u[0]) + _dot6(j1[6 * r:6 * r + 6], u[1])
            if r == 2 and driven:
                rhs[3 * i + r] = float(motor[i][0]) / dti - ju
            else:
                rhs[3 * i + r] = kk * float(err[3 * i + r]) - ju
    return dict(J0=J0, J1=J1, err=err, lo=lo, hi=hi, rhs=rhs, is_eq=is_eq)


def bits_equal(a, b, dtype=np.float64):
    """Bit for bit, signs of zero included, after the cast to dtype."""
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=dtype)
    b = np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=dtype)
    u = np.uint64 if dtype == np.float64 else np.uint32
    return a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def check_twin(case, asm, tw, motor=None):
    """The twin within its bounds of the reference: J, err and rhs by tolerance, the bounds and row types exactly.
    Returns the worst error / tolerance ratios."""
    r = {"J": max(asm["J0"].worst(tw["J0"])[0], asm["J1"].worst(tw["J1"])[0]), "err": asm["err"].worst(tw["err"])[0],
         "rhs": rhs_reference(case, asm, motor).worst(tw["rhs"])[0]}
    lo, hi = motor_bounds(case, asm, motor)
    assert np.array_equal(tw["is_eq"], asm["is_eq"]) and np.array_equal(tw["lo"], lo) and np.array_equal(tw["hi"], hi)
    return r


# ---- generated cases ----------------------------------------------------------------------------------------------------------
def _quat_of(Rm):
    """A unit quaternion (w, x, y, z) of the rotation matrix Rm [3][3] (numpy), by the largest-component branch."""
    t = np.trace(Rm)
    cand = np.array([1 + t, 1 + 2 * Rm[0, 0] - t, 1 + 2 * Rm[1, 1] - t, 1 + 2 * Rm[2, 2] - t])
    k = int(np.argmax(cand))
    s = 2.0 * math.sqrt(cand[k])
    if k == 0:
        q = [s / 4, (Rm[2, 1] - Rm[1, 2]) / s, (Rm[0, 2] - Rm[2, 0]) / s, (Rm[1, 0] - Rm[0, 1]) / s]
    elif k == 1:
        q = [(Rm[2, 1] - Rm[1, 2]) / s, s / 4, (Rm[0, 1] + Rm[1, 0]) / s, (Rm[0, 2] + Rm[2, 0]) / s]
    elif k == 2:
        q = [(Rm[0, 2] - Rm[2, 0]) / s, (Rm[0, 1] + Rm[1, 0]) / s, s / 4, (Rm[1, 2] + Rm[2, 1]) / s]
    else:
        q = [(Rm[1, 0] - Rm[0, 1]) / s, (Rm[0, 2] + Rm[2, 0]) / s, (Rm[1, 2] + Rm[2, 1]) / s, s / 4]
    q = np.array(q)
    return q / np.linalg.norm(q)


def lock_data(R0, R1=None):
    """data [7] of a lock that holds the current relative orientation: the quaternion of R0^T R1 (R0^T for a world side)."""
    R0 = np.asarray(R0, np.float64).reshape(3, 3)
    Rref = R0.T @ (np.asarray(R1, np.float64).reshape(3, 3) if R1 is not None else np.eye(3))
    return np.concatenate([_quat_of(Rref), np.zeros(3)])


def hinge_data(R0, axis_world, R1=None):
    """data [7] of a hinge about the world axis given, at the current pose: the axis in either body's frame."""
    a = np.asarray(axis_world, np.float64)
    a = a / np.linalg.norm(a)
    a0 = np.asarray(R0, np.float64).reshape(3, 3).T @ a
    a1 = np.asarray(R1, np.float64).reshape(3, 3).T @ a if R1 is not None else a
    return np.concatenate([a0 / np.linalg.norm(a0), a1 / np.linalg.norm(a1), np.zeros(1)])


PATTERNS = ["lock", "hinge", "joint", "contact", "lock_world", "hinge_world", "contact_w0", "joint_world"]
MOTORS = ((0.0, -1.0), (1.5, 0.0), (-2.0, math.inf), (0.7, 0.05), (3.0, -1.0))


def make_case(seed, n, m, offset=0, minv="iso", dt=5e-3, erp=0.2, bend=0.3):
    """n bodies and m constraints cycling through PATTERNS from `offset`: the ball joints and contacts as
    model_reference draws them, a lock whose stored orientation is up to `bend` rad away from the pose, a hinge whose two
    axes are up to `bend` rad apart.  Every third hinge has its axis s within 1e-2 rad of -z, where align_to_z is at its
    worst outside the branch.  motor [m][2] cycles through MOTORS.  Redrawn (seed + 1000) while a hinge axis lies inside
    the antiparallel branch."""
    while True:
        base = mr.make_case(seed, n, m, patterns=[p if p in ("joint", "joint_world", "contact", "contact_w0") else "joint"
                                                  for p in PATTERNS], offset=offset, minv=minv, dt=dt, erp=erp)
        rng = np.random.default_rng(seed + 13)
        kind, data = base["kind"].copy(), base["data"].copy()
        body1 = base["body1"].copy()
        names, nh = [], 0
        ok = True
        for i in range(m):
            pat = PATTERNS[(i + offset) % len(PATTERNS)]
            names.append(pat)
            if not (pat.startswith("lock") or pat.startswith("hinge")):
                continue
            if pat.endswith("_world") or n < 2:
                body1[i] = -1
            b0, b1 = int(base["body0"][i]), int(body1[i])
            R0 = base["R"][b0].reshape(3, 3)
            R1 = base["R"][b1].reshape(3, 3) if b1 >= 0 else None
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            ang = rng.uniform(-bend, bend)
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            off = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
            if pat.startswith("lock"):
                kind[i] = LOCK
                data[i] = lock_data(off @ R0, R1)
            else:
                kind[i] = HINGE
                nh += 1
                s = rng.normal(size=3)
                if nh % 3 == 0:
                    phi = rng.uniform(0, 2 * math.pi)
                    s = np.array([math.sin(1e-2) * math.cos(phi), math.sin(1e-2) * math.sin(phi), -math.cos(1e-2)])
                s /= np.linalg.norm(s)
                data[i] = hinge_data(R0, s, R1)
                t = off @ s
                data[i, 3:6] = (R1.T @ t) if R1 is not None else t
                data[i, 3:6] /= np.linalg.norm(data[i, 3:6])
                sw = R0 @ data[i, 0:3]
                ok = ok and 1.0 + sw[2] / np.linalg.norm(sw) > 1e-9       # far outside BRANCH = 1e-12
        if ok:
            break
        seed += 1000
    motor = np.array([MOTORS[(i + seed) % len(MOTORS)] for i in range(m)])
    case = dict(base, kind=kind, data=data, body1=body1, names=names)
    return case, motor


# (id, seed, n, m, offset, minv): the families of the issue -- 4 bodies and 8 constraints mixing all four kinds, two-body
# and world-side, on both mass forms; one list that crosses assemble_kernel's 256-thread block
CASES = [("n4m8-a", 301, 4, 8, 0, "iso"), ("n4m8-b", 302, 4, 8, 3, "aniso"), ("n4m8-c", 303, 4, 8, 5, "coupled"),
         ("m259", 304, 9, 259, 0, "iso")]
IDS = [c[0] for c in CASES]
_cache = {}


def generated(cid):
    """(case, motor, reference assembly, twin without the motor, twin with it): once per process; leave them unchanged."""
    if cid not in _cache:
        _, seed, n, m, off, minv = CASES[IDS.index(cid)]
        case, motor = make_case(seed, n, m, off, minv)
        _cache[cid] = (case, motor, assemble_reference(case), twin_assemble(case), twin_assemble(case, motor))
    return _cache[cid]


# ---- the solve: the bounded system of a step, solved directly in mpmath ------------------------------------------------------------
def solve_reference(case, tw, cfm, tie=1e-9):
    """lambda of  A x = rhs - w,  A = J M^-1 J^T + cfm I,  equality rows: w = 0; bounded rows: lo <= x <= hi with w >= 0
    at lo, w <= 0 at hi, w = 0 between -- from the fp64 system `tw` (twin_assemble's dict), in mpmath.  The active set is
    found by enumeration over the bounded rows that are not pinned (lo = hi: x fixed), so it is decided in exact
    arithmetic; tie: the smallest relative margin of a decision (the caller redraws below 1e-9).  Returns (x [3m] mpf,
    the 1-norm of the inverse of the free block, margin)."""
    import itertools
    with mp.workdps(mr.DPS):
        m = case["kind"].shape[0]
        N = 3 * m
        n = np.asarray(case["p"]).shape[0]
        Minv = [[mr._v(case["Minv"][b])[6 * r:6 * r + 6] for r in range(6)] for b in range(n)]
        rows = []
        for i in range(m):
            for r in range(3):
                rows.append([(int(case[bn][i]), mr._v(tw[Jn][i])[6 * r:6 * r + 6]) for bn, Jn in (("body0", "J0"), ("body1", "J1"))
                             if int(case[bn][i]) >= 0])
        A = mp.zeros(N, N)
        for a in range(N):
            for b in range(N):
                acc = mp.mpf(0)
                for ba, ja in rows[a]:
                    for bb, jb in rows[b]:
                        if ba == bb:
                            acc += sum(ja[r] * sum(Minv[ba][r][c] * jb[c] for c in range(6)) for r in range(6))
                A[a, b] = acc + (mp.mpf(float(cfm)) if a == b else 0)
        rhs = mr._v(tw["rhs"])
        lo = [mp.mpf(float(x)) if math.isfinite(x) else (mp.inf if x > 0 else -mp.inf) for x in tw["lo"]]
        hi = [mp.mpf(float(x)) if math.isfinite(x) else (mp.inf if x > 0 else -mp.inf) for x in tw["hi"]]
        eq = [bool(x) for x in tw["is_eq"]]
        pinned = [k for k in range(N) if not eq[k] and lo[k] == hi[k]]
        boxed = [k for k in range(N) if not eq[k] and lo[k] != hi[k]]
        for states in itertools.product((0, -1, 1), repeat=len(boxed)):      # 0: free, -1: at lo, +1: at hi
            fixed = {k: lo[k] for k in pinned}
            bad = False
            for k, st in zip(boxed, states):
                if st:
                    fixed[k] = lo[k] if st < 0 else hi[k]
                    bad = bad or mp.isinf(fixed[k])
            if bad:
                continue
            free = [k for k in range(N) if k not in fixed]
            x = [mp.mpf(0)] * N
            for k, val in fixed.items():
                x[k] = val
            if free:
                Aff = mp.matrix(len(free), len(free))
                bf = mp.matrix(len(free), 1)
                for a, ka in enumerate(free):
                    for b, kb in enumerate(free):
                        Aff[a, b] = A[ka, kb]
                    bf[a] = rhs[ka] - sum(A[ka, kf] * xv for kf, xv in fixed.items())
                inv = Aff ** -1
                sol = inv * bf
                for a, ka in enumerate(free):
                    x[ka] = sol[a]
                norm1 = max(sum(abs(inv[a, b]) for a in range(len(free))) for b in range(len(free)))
            else:
                norm1 = mp.mpf(0)
            w = [sum(A[a, b] * x[b] for b in range(N)) - rhs[a] for a in range(N)]
            good, margin = True, mp.inf
            scale = max([abs(v) for v in rhs] + [mp.mpf(1)])
            for k, st in zip(boxed, states):
                if st == 0:
                    good = good and lo[k] <= x[k] <= hi[k]
                    margin = min([margin] + [abs(x[k] - bnd) / scale for bnd in (lo[k], hi[k]) if not mp.isinf(bnd)])
                else:
                    good = good and (w[k] >= 0 if st < 0 else w[k] <= 0)
                    margin = min(margin, abs(w[k]) / scale)
            if good:
                return x, norm1, float(margin)
        raise AssertionError("no complementary solution found")
