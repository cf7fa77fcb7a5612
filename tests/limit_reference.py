"""Hinge angle limits (egs_problem_set_hinge_limits) as mathematics and as an fp64 twin.  joint_reference is imported
unchanged; this file adds the angle read-out and the one-sided axis row.

The reference, in mpmath at 50 digits from the exact fp64 inputs (R0, R1, a0 and the table row
(qw, qx, qy, qz, sin lo, cos lo, sin hi, cos hi)):

  E = R0 Rq R1^T (R1 = I for a world side), Rq the polynomial rotation matrix of q as it stands
  s = R0 a0,  sn = s . axial(E),  cs = (trace(E) - 1) / 2,  theta = atan2(sn, cs)
  upper stop set and theta > atan2(shi, chi):       err[2] = sn chi - cs shi, lo = -inf, hi = 0
  else lower stop set and theta < atan2(slo, clo):  err[2] = sn clo - cs slo, lo = 0, hi = +inf
  else the axis row as without the table

For E a rotation by theta about s, sn = sin(theta), cs = cos(theta) and err[2] = sin(theta - limit).  That d theta/dt =
s^ . (w0 - w1) is checked in test_limit_reference_cpu.py against the exact rigid motion.

The device compares tan(theta/2) = sn / (1 + cs) with tan(limit/2) = sl / (1 + cl), cross-multiplied; for sn^2 + cs^2 = 1
that is the atan2 comparison (tan(x/2) is monotone on (-pi, pi)).  The generators keep every case at least MARGIN from its
stops in tan(theta/2), so the twin's decision and the reference's must agree: the tests assert it, no case is skipped.

Tolerances, in units of u = 2^-53, by joint_reference's rules (a k-term product sum of exact inputs is within (k + 1) u
of its magnitude sum; an input error d moves it by the other factor's magnitude times d):

  E                  joint_reference.lock_reference's dE (4u mag per product, the input errors carried along)
  ax_k               u |E_a - E_b| / 2 + (dE_a + dE_b) / 2
  s_k                4u mag
  sn = d3(s, ax)     4u mag + sum(|s_k| dax_k + ds_k |ax_k| + ds_k dax_k)
  cs                 (dE_00 + dE_11 + dE_22) / 2 + 4u (|E_00| + |E_11| + |E_22| + 1) / 2       three additions, one halving
  err[2]             3u (|sn cl| + |cs sl|) + dsn |cl| + dcs |sl|

The twin restates assemble_device.h's limit_row in Python floats (no contraction, no trigonometric function): the
device's bits."""
import math

import mpmath as mp
import numpy as np

import joint_reference as jr
import model_reference as mr

U = mr.U
HINGE = jr.HINGE
MARGIN = 1e-9
INF = math.inf


# ---- the table ---------------------------------------------------------------------------------------------------------------
def pair(angle):
    """(sin, cos) of a stop; None: no stop on that side, (0, 0)."""
    return (0.0, 0.0) if angle is None else (math.sin(angle), math.cos(angle))


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def limit_row(R0, a0, R1=None, theta=0.0, lo=None, hi=None):
    """The table row of a hinge that stands at `theta` now: q is the quaternion of R0(0)^T R1(0) with
    R0 = exp(theta [s]x) R0(0), s = R0 a0; lo / hi in radians or None."""
    R0 = np.asarray(R0, np.float64).reshape(3, 3)
    s = R0 @ np.asarray(a0, np.float64)
    R00 = _rot(s, -theta) @ R0
    Rref = R00.T @ (np.asarray(R1, np.float64).reshape(3, 3) if R1 is not None else np.eye(3))
    return np.concatenate([jr._quat_of(Rref), pair(lo), pair(hi)])


# ---- the reference -----------------------------------------------------------------------------------------------------------
def angle_reference(R0, R1, a0, q):
    """(sn, cs, dsn, dcs) in mpf: sin and cos of the hinge angle as the assembly reads them, and what the fp64 code may be
    off by.  R1 None: a world side."""
    Rq, Mq = jr.quat_matrix(q)
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
    ax = [(E[a[0]][a[1]] - E[b[0]][b[1]]) / 2 for a, b in pairs]
    dax = [U * abs(E[a[0]][a[1]] - E[b[0]][b[1]]) / 2 + (dE[a[0]][a[1]] + dE[b[0]][b[1]]) / 2 for a, b in pairs]
    s, sm = mr._mv(R0, a0), mr._absmv(R0, a0)
    ds = [4 * U * x for x in sm]
    sn = sum(s[k] * ax[k] for k in range(3))
    dsn = 4 * U * sum(abs(s[k] * ax[k]) for k in range(3)) + sum(abs(s[k]) * dax[k] + ds[k] * abs(ax[k]) + ds[k] * dax[k] for k in range(3))
    cs = ((E[0][0] + E[1][1] + E[2][2]) - 1) / 2
    dcs = (dE[0][0] + dE[1][1] + dE[2][2]) / 2 + 4 * U * (abs(E[0][0]) + abs(E[1][1]) + abs(E[2][2]) + 1) / 2
    return sn, cs, dsn, dcs


def limit_reference(R0, R1, a0, L):
    """(active: +1 upper, -1 lower, 0 none; err2, its tolerance; the distance of tan(theta/2) from the nearest stop set;
    theta), all mpf, the decision by atan2.  L: the table row as mpf."""
    sn, cs, dsn, dcs = angle_reference(R0, R1, a0, L[0:4])
    theta = mp.atan2(sn, cs)
    slo, clo, shi, chi = L[4:8]
    lower, upper = (slo != 0 or clo != 0), (shi != 0 or chi != 0)
    dist = mp.inf
    for on, sl, cl in ((lower, slo, clo), (upper, shi, chi)):
        if on:
            dist = min(dist, abs(mp.tan(theta / 2) - mp.tan(mp.atan2(sl, cl) / 2)))
    for on, sl, cl, sign in ((upper, shi, chi, 1), (lower, slo, clo, -1)):
        if on and (theta > mp.atan2(sl, cl) if sign > 0 else theta < mp.atan2(sl, cl)):
            err = sn * cl - cs * sl
            tol = 3 * U * (abs(sn * cl) + abs(cs * sl)) + dsn * abs(cl) + dcs * abs(sl)
            return sign, err, tol, dist, theta
    return 0, mp.mpf(0), mp.mpf(0), dist, theta


def case_reference(case, lim):
    """Per constraint (active, err2, tol, dist, theta) or None where the table does not apply."""
    out = []
    with mp.workdps(mr.DPS):
        R = [mr._m3(x) for x in case["R"]]
        for i in range(case["kind"].shape[0]):
            L = [float(x) for x in lim[i]]
            if case["kind"][i] != HINGE or not any(L[4:8]):
                out.append(None)
                continue
            b0, b1 = int(case["body0"][i]), int(case["body1"][i])
            out.append(limit_reference(R[b0], R[b1] if b1 >= 0 else None, mr._v(case["data"][i][0:3]), mr._v(L)))
    return out


# ---- the fp64 twin -----------------------------------------------------------------------------------------------------------
def twin_limit_row(R0, R1, a0, L):
    """assemble_device.h's limit_row on one hinge: (active, err2, lo2, hi2, sn, cs); floats.  R1 None: a world side."""
    slo, clo, shi, chi = L[4], L[5], L[6], L[7]
    lower, upper = (slo != 0.0 or clo != 0.0), (shi != 0.0 or chi != 0.0)
    if not lower and not upper:
        return 0, 0.0, 0.0, 0.0, None, None
    s = jr._mv3(R0, a0)
    Rq = jr._quat_to_R(L[0], L[1], L[2], L[3])
    T = jr._mm3(R0, Rq)
    if R1 is not None:
        R1t = [R1[3 * c + r] for r in range(3) for c in range(3)]
        E = jr._mm3(T, R1t)
    else:
        E = T
    ax = [0.5 * (E[7] - E[5]), 0.5 * (E[2] - E[6]), 0.5 * (E[3] - E[1])]
    sn = jr._d3(s, ax)
    cs = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0)
    if upper and sn * (1.0 + chi) > shi * (1.0 + cs):
        return 1, sn * chi - cs * shi, -INF, 0.0, sn, cs
    if lower and sn * (1.0 + clo) < slo * (1.0 + cs):
        return -1, sn * clo - cs * slo, 0.0, INF, sn, cs
    return 0, 0.0, 0.0, 0.0, sn, cs


def twin_assemble(case, motor=None, lim=None, dt=None, erp=None):
    """joint_reference.twin_assemble, then the limit rows: an active stop replaces err[2], lo[2], hi[2] and
    rhs[2] = kk err[2] - ju of its hinge, the motor's row included (the motor leaves an active stop's row alone)."""
    tw = jr.twin_assemble(case, motor, dt=dt, erp=erp)
    tw["active"] = np.zeros(case["kind"].shape[0], np.int32)
    if lim is None:
        return tw
    m = case["kind"].shape[0]
    R = np.asarray(case["R"], np.float64).reshape(-1, 9)
    dts = np.broadcast_to(np.float64(case["dt"] if dt is None else dt), (m,)) if np.ndim(dt) == 0 else np.asarray(dt, np.float64)
    erps = np.broadcast_to(np.float64(case["erp"] if erp is None else erp), (m,)) if np.ndim(erp) == 0 else np.asarray(erp, np.float64)
    Minv, f = np.asarray(case["Minv"]).reshape(-1, 36), np.asarray(case["f_ext"]).reshape(-1, 6)
    for i in range(m):
        if case["kind"][i] != HINGE:
            continue
        b = (int(case["body0"][i]), int(case["body1"][i]))
        act, e2, lo2, hi2, _, _ = twin_limit_row([float(x) for x in R[b[0]]], [float(x) for x in R[b[1]]] if b[1] >= 0 else None,
                                                 [float(x) for x in case["data"][i][0:3]], [float(x) for x in lim[i]])
        tw["active"][i] = act
        if not act:
            continue
        k = 3 * i + 2
        tw["err"][k], tw["lo"][k], tw["hi"][k] = e2, lo2, hi2
        dti, erpi = float(dts[i]), float(erps[i])
        if dti == 0.0:
            tw["rhs"][k] = 0.0
            continue
        u = [[0.0] * 6, [0.0] * 6]
        for side in range(2):
            if b[side] < 0:
                continue
            for r in range(6):
                vel = float(case["v"][b[side]][r] if r < 3 else case["w"][b[side]][r - 3])
                u[side][r] = vel / dti + jr._dot6([float(x) for x in Minv[b[side]][6 * r:6 * r + 6]], [float(x) for x in f[b[side]]])
        j0, j1 = [float(x) for x in tw["J0"][i]], [float(x) for x in tw["J1"][i]]
        ju = jr._dot6(j0[12:18], u[0]) + jr._dot6(j1[12:18], u[1])
        tw["rhs"][k] = (-erpi / dti / dti) * e2 - ju
    return tw


# ---- generated tables --------------------------------------------------------------------------------------------------------
# (theta now, lo, hi): upper active, lower active, inside; one-sided tables either way, active and not; stops and angles
# beyond 3 rad; a row without a stop
SPECS = [(0.4, -0.5, 0.3), (-0.4, -0.3, 0.5), (0.1, -0.3, 0.5), (0.4, None, 0.3), (0.4, -0.3, None), (-0.4, None, 0.3),
         (-0.4, -0.3, None), (3.05, -1.0, 3.0), (-3.05, -3.0, 1.0), (3.1, None, None), (-3.1, -3.13, 3.13)]
FAMILIES = {"upper": 0, "lower": 1, "inside": 2, "one-sided": 3, "one-sided-b": 5, "near-pi": 7, "none-and-wide": 9}


def make_limits(case, offset=0):
    """lim [m][8] for the hinges of a joint_reference case, hinge number k taking SPECS[(k + offset) % len]; the rows of
    the other kinds hold a stop too (they are ignored).  Every hinge at least MARGIN from its stops."""
    m = case["kind"].shape[0]
    lim = np.zeros((m, 8))
    lim[:, 0] = 1.0
    lim[:, 6:8] = pair(0.25)
    k = 0
    for i in range(m):
        if case["kind"][i] != HINGE:
            continue
        th, lo, hi = SPECS[(k + offset) % len(SPECS)]
        k += 1
        b0, b1 = int(case["body0"][i]), int(case["body1"][i])
        lim[i] = limit_row(case["R"][b0], case["data"][i][0:3], case["R"][b1] if b1 >= 0 else None, th, lo, hi)
    with mp.workdps(mr.DPS):
        for r in case_reference(case, lim):
            assert r is None or r[3] > MARGIN, "a generated hinge sits on a stop: choose other angles"
    return lim
