"""The slider block (EGS_JOINT_SLIDER_AXIS = 5), its motor and its travel stops as mathematics and as an fp64 twin.
joint_reference and model_reference are imported unchanged; the rows of the other four kinds come from them.

The reference, in mpmath at 50 digits from the exact fp64 inputs (p0, R0, P1, a0, c and the table row (xlo, xhi)):

  s = R0 a0,  Rn = the shortest arc taking s^ to z, rows (p, q, s^)
  two bodies:  D = p0 + R0 c - P1, P1 = pos[b1];   world side:  D = p0 - c, P1 = c
  err = (p . D, q . D, 0);  x = s^ . D
  J0 = [Rn | rw], row r of rw = (P1 - p0) x Rn_r;  J1 = [-Rn | 0] (zero for a world side)
  motor (speed, f), f >= 0:   lo[2] = -f, hi[2] = f, rhs[2] = speed / dt - J row 2 . (v/dt + M^-1 f_ext)
  xhi finite and x > xhi:       err[2] = x - xhi, lo = -inf, hi = 0       (the motor leaves the row alone)
  else xlo finite and x < xlo:  err[2] = x - xlo, lo = 0, hi = +inf
  else the rail row as without the table

That d err/dt = J0 s0 + J1 s1 (rows 0, 1 at err = 0; the travel x at every pose) and that the block carries no net force
or torque is checked in test_slider_reference_cpu.py.

Tolerances, in units of u = 2^-53, by joint_reference's rules (a k-term product sum of exact inputs is within (k + 1) u
of its magnitude sum; an input error d moves it by the other factor's magnitude times d):

  s_k                4u mag;  ds = the largest of them
  Rn entries         tRn = 64u / (1 + c) + 20 ds / (1 + c)                      [joint_reference's hinge bound]
  ro = R0 c          4u mag
  D_k                two bodies: 3u (|p0_k| + |ro_k| + |P1_k|) + dro_k  (two additions of which one has an inexact input);
                     world side: 2u (|p0_k| + |c_k|)
  rel_k = p0 - P1    2u (|p0_k| + |P1_k|)
  rw entries         4u mag + sum_k (tRn |H_kj| + |Rn_rk| dH_kj + tRn dH_kj), H = [rel]x, dH its entries' drel
  err_r, x           4u mag + sum_k (|Rn_rk| dD_k + tRn |D_k| + tRn dD_k)
  err[2] at a stop   dx + 2u (|x| + |limit|)
  rhs rows           joint_reference's: 32u mag + (J tolerance of the row) |v/dt + M^-1 f|_1 + (erp / dt^2) (err tolerance);
                     the motor's speed / dt is one more term of the row

A tolerance of zero means "these bits": err[2] of a slider without an active stop, the zero angular columns of J1, the
bounds, the row types.

The twin restates assemble_device.h's slider_block, slider_stop_row and motor_row in Python floats (no contraction, no
trigonometric function): the device's bits.  The generators keep every slider at least MARGIN = 1e-9 from its stops in
x, and the tolerance of x stays below MARGIN (asserted beside it: a rail 1e-2 rad from -z has it near 1e-11), so the
twin's decision and the reference's must agree: the tests assert it, no case is skipped.  Rail directions within
model_reference.BRANCH of -z are redrawn."""
import math

import mpmath as mp
import numpy as np

import joint_reference as jr
import model_reference as mr

U = mr.U
SLIDER = 5
MARGIN = 1e-9
INF = math.inf


# ---- the reference -----------------------------------------------------------------------------------------------------------
def slider_reference(p0, R0, P1, a0, c):
    """One slider in mpf; P1 None: a world side (then c is the world point).  Returns a dict: Rn, tRn, D, dD, err, terr
    [3], x, dx, J0 / J1 as 18 (value, magnitude, tolerance) triples."""
    zero = mp.mpf(0)
    s, sm = mr._mv(R0, a0), mr._absmv(R0, a0)
    ds = max(4 * U * v for v in sm)
    Rn, _, opc = mr.align_to_z(s)
    assert Rn is not None, "rail direction inside the antiparallel branch: the generators draw none"
    tRn = 64 * U / opc + 20 * ds / opc
    if P1 is not None:
        ro, rom = mr._mv(R0, c), mr._absmv(R0, c)
        D = [p0[k] + ro[k] - P1[k] for k in range(3)]
        dD = [3 * U * (abs(p0[k]) + abs(ro[k]) + abs(P1[k])) + 4 * U * rom[k] for k in range(3)]
        target = P1
    else:
        D = [p0[k] - c[k] for k in range(3)]
        dD = [2 * U * (abs(p0[k]) + abs(c[k])) for k in range(3)]
        target = c
    rel = [p0[k] - target[k] for k in range(3)]
    drel = [2 * U * (abs(p0[k]) + abs(target[k])) for k in range(3)]
    H = mr._hat(rel)
    comp = [[None, 2, 1], [2, None, 0], [1, 0, None]]      # the component of rel behind entry (k, j) of [rel]x
    dH = [[zero if comp[k][j] is None else drel[comp[k][j]] for j in range(3)] for k in range(3)]
    rw, rwm = mr._mul(Rn, H), mr._absmul(Rn, H)
    rows, trows = [], []
    for r in range(3):
        rows.append(sum(Rn[r][k] * D[k] for k in range(3)))
        mag = sum(abs(Rn[r][k] * D[k]) for k in range(3))
        trows.append(4 * U * mag + sum(abs(Rn[r][k]) * dD[k] + tRn * abs(D[k]) + tRn * dD[k] for k in range(3)))
    J0, J1 = [(zero, zero, zero)] * 18, [(zero, zero, zero)] * 18
    for r in range(3):
        for j in range(3):
            J0[6 * r + j] = (Rn[r][j], abs(Rn[r][j]), tRn)
            tol = 4 * U * rwm[r][j] + sum(tRn * abs(H[k][j]) + abs(Rn[r][k]) * dH[k][j] + tRn * dH[k][j] for k in range(3))
            J0[6 * r + 3 + j] = (rw[r][j], rwm[r][j], tol)
            if P1 is not None:
                J1[6 * r + j] = (-Rn[r][j], abs(Rn[r][j]), tRn)
    return dict(Rn=Rn, tRn=tRn, D=D, dD=dD, err=[rows[0], rows[1], zero], terr=[trows[0], trows[1], zero], x=rows[2], dx=trows[2],
                J0=J0, J1=J1, rel=rel)


def stop_reference(x, dx, xlo, xhi):
    """(active: +1 upper, -1 lower, 0 none; err2; its tolerance; the distance of x from the nearest finite stop), mpf;
    xlo / xhi floats, -inf / +inf: no stop."""
    dist = mp.inf
    for lim in (xlo, xhi):
        if math.isfinite(lim):
            dist = min(dist, abs(x - mp.mpf(lim)))
    if math.isfinite(xhi) and x > mp.mpf(xhi):
        return 1, x - mp.mpf(xhi), dx + 2 * U * (abs(x) + abs(mp.mpf(xhi))), dist
    if math.isfinite(xlo) and x < mp.mpf(xlo):
        return -1, x - mp.mpf(xlo), dx + 2 * U * (abs(x) + abs(mp.mpf(xlo))), dist
    return 0, mp.mpf(0), mp.mpf(0), dist


def _others(case):
    """(indices of the rows that are no slider, the case restricted to them)."""
    kind = np.asarray(case["kind"])
    old = np.nonzero(kind != SLIDER)[0]
    sub = dict(case)
    for k in ("kind", "body0", "body1", "data"):
        sub[k] = np.asarray(case[k])[old]
    return old, sub


def slider_motor_applies(case, motor, i, active=None):
    return (motor is not None and case["kind"][i] == SLIDER and float(motor[i][1]) >= 0 and
            not (active is not None and active[i]))


def assemble_reference(case, travel=None):
    """jr.assemble_reference for a list that holds sliders too: the other rows from it, the sliders from
    slider_reference, an active stop's err[2] and bounds already in place.  Adds `active` [m], `x` and `dist` per slider
    (None elsewhere)."""
    kind = np.asarray(case["kind"])
    m = kind.shape[0]
    old, sub = _others(case)
    base = jr.assemble_reference(sub)
    with mp.workdps(mr.DPS):
        J = [mr.Checked(18 * m), mr.Checked(18 * m)]
        err = mr.Checked(3 * m)
        is_eq = np.zeros(3 * m, np.uint8)
        lo, hi = np.zeros(3 * m), np.zeros(3 * m)
        branch = np.zeros(m, bool)
        active = np.zeros(m, np.int32)
        xs, dist = [None] * m, [None] * m
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
        p = [mr._v(x) for x in case["p"]]
        R = [mr._m3(x) for x in case["R"]]
        for i in np.nonzero(kind == SLIDER)[0]:
            d = mr._v(case["data"][i])
            b0, b1 = int(case["body0"][i]), int(case["body1"][i])
            assert b0 >= 0
            ref = slider_reference(p[b0], R[b0], p[b1] if b1 >= 0 else None, d[0:3], d[3:6])
            for e in range(18):
                J[0].put(18 * i + e, *ref["J0"][e])
                J[1].put(18 * i + e, *ref["J1"][e])
            e3, t3 = list(ref["err"]), list(ref["terr"])
            xs[i] = (ref["x"], ref["dx"])
            if travel is not None:
                act, e2, tol, dist[i] = stop_reference(ref["x"], ref["dx"], float(travel[i][0]), float(travel[i][1]))
                active[i] = act
                if act:
                    e3[2], t3[2] = e2, tol
                    lo[3 * i + 2], hi[3 * i + 2] = (-INF, 0.0) if act > 0 else (0.0, INF)
            for r in range(3):
                err.put(3 * i + r, e3[r], abs(e3[r]), t3[r])
            is_eq[3 * i:3 * i + 2] = 1
        return dict(J0=J[0], J1=J[1], err=err, is_eq=is_eq, lo=lo, hi=hi, branch=branch, geo=None, active=active, x=xs, dist=dist)


def bounds_reference(case, asm, motor):
    """(lo, hi) with the motors' limits on the hinges' axis rows and on the rail rows without an active stop."""
    lo, hi = jr.motor_bounds(case, asm, motor)
    for i in range(case["kind"].shape[0]):
        if slider_motor_applies(case, motor, i, asm["active"]):
            lo[3 * i + 2], hi[3 * i + 2] = -float(motor[i][1]), float(motor[i][1])
    return lo, hi


def rhs_reference(case, asm, motor=None):
    """jr.rhs_reference (the hinges' motors, the absolute err tolerances of every kind above 1), then the sliders' motor
    targets as it adds a hinge's."""
    out = jr.rhs_reference(case, asm, motor)
    with mp.workdps(mr.DPS):
        dt = mp.mpf(float(case["dt"]))
        for i in range(case["kind"].shape[0]):
            if not slider_motor_applies(case, motor, i, asm["active"]):
                continue
            k = 3 * i + 2
            tgt = mp.mpf(float(motor[i][0])) / dt
            rest_of_tol = out.tol[k] - 32 * U * out.mag[k]
            mag = out.mag[k] + abs(tgt)
            out.put(k, out.val[k] + tgt, mag, 32 * U * mag + rest_of_tol)
    return out


# ---- the fp64 twin -----------------------------------------------------------------------------------------------------------
def _crossmat(a):
    return [0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0]


def twin_frame(p0, R0, P1, d):
    """assemble_device.h's slider_frame: (Rn [9], D [3], rel [3]); P1 None: a world side."""
    s = jr._mv3(R0, d[0:3])
    Rn = jr._align_to_z(s)
    if P1 is not None:
        ro = jr._mv3(R0, d[3:6])
        D = [(p0[k] + ro[k]) - P1[k] for k in range(3)]
        rel = [p0[k] - P1[k] for k in range(3)]
    else:
        D = [p0[k] - d[3 + k] for k in range(3)]
        rel = [p0[k] - d[3 + k] for k in range(3)]
    return Rn, D, rel


def twin_block(p0, R0, P1, d):
    """(j0 [18], j1 [18], err [3], x) of one slider, the device's operations in the device's order."""
    Rn, D, rel = twin_frame(p0, R0, P1, d)
    rw = jr._mm3(Rn, _crossmat(rel))
    j0, j1 = [0.0] * 18, [0.0] * 18
    e = [jr._d3(Rn[0:3], D), jr._d3(Rn[3:6], D), 0.0]
    for r in range(3):
        for k in range(3):
            j0[6 * r + k] = Rn[3 * r + k]
            j0[6 * r + 3 + k] = rw[3 * r + k]
            if P1 is not None:
                j1[6 * r + k] = -1.0 * Rn[3 * r + k]
    return j0, j1, e, jr._d3(Rn[6:9], D)


def twin_stop(x, xlo, xhi):
    """slider_stop_row's decision: (active, err2, lo2, hi2)."""
    if xhi < INF and x > xhi:
        return 1, x - xhi, -INF, 0.0
    if xlo > -INF and x < xlo:
        return -1, x - xlo, 0.0, INF
    return 0, 0.0, 0.0, 0.0


def _sub_rates(v, old, m):
    return v if v is None or np.ndim(v) == 0 else np.asarray(v, np.float64)[old]


def twin_assemble(case, motor=None, travel=None, dt=None, erp=None, hinge_lim=None):
    """The whole assembly in fp64 as the device makes it (jr.twin_assemble's dict, plus `active` and `x` per constraint):
    the rows that are no slider from jr.twin_assemble, the sliders from the restatement here.  motor [m][2], travel
    [m][2] or None.  dt / erp: scalars (default: the case's) or one value per constraint (dt 0: rhs rows exactly 0).
    hinge_lim [m][8] or None: the hinge limits' table beside them (limit_reference.twin_assemble makes those rows;
    `active` then holds the hinges' stops too)."""
    kind = np.asarray(case["kind"])
    m = kind.shape[0]
    old, sub = _others(case)
    if hinge_lim is None:
        base = jr.twin_assemble(sub, None if motor is None else np.asarray(motor)[old], dt=_sub_rates(dt, old, m), erp=_sub_rates(erp, old, m))
    else:
        import limit_reference as lr
        base = lr.twin_assemble(sub, None if motor is None else np.asarray(motor)[old], np.asarray(hinge_lim)[old],
                                dt=_sub_rates(dt, old, m), erp=_sub_rates(erp, old, m))
    J0, J1 = np.zeros((m, 18)), np.zeros((m, 18))
    err, lo, hi, rhs = np.zeros(3 * m), np.zeros(3 * m), np.zeros(3 * m), np.zeros(3 * m)
    is_eq = np.zeros(3 * m, np.uint8)
    rows = (3 * old[:, None] + np.arange(3)).reshape(-1)
    J0[old], J1[old] = base["J0"], base["J1"]
    for name, arr in (("err", err), ("lo", lo), ("hi", hi), ("rhs", rhs), ("is_eq", is_eq)):
        arr[rows] = base[name]
    active, xs = np.zeros(m, np.int32), np.full(m, np.nan)
    if hinge_lim is not None:
        active[old] = base["active"]
    dts = np.broadcast_to(np.float64(case["dt"] if dt is None else dt), (m,)) if np.ndim(dt) == 0 else np.asarray(dt, np.float64)
    erps = np.broadcast_to(np.float64(case["erp"] if erp is None else erp), (m,)) if np.ndim(erp) == 0 else np.asarray(erp, np.float64)
    P = np.asarray(case["p"], np.float64).reshape(-1, 3)
    R = np.asarray(case["R"], np.float64).reshape(-1, 9)
    Minv, f = np.asarray(case["Minv"]).reshape(-1, 36), np.asarray(case["f_ext"]).reshape(-1, 6)
    for i in np.nonzero(kind == SLIDER)[0]:
        b = (int(case["body0"][i]), int(case["body1"][i]))
        j0, j1, e, x = twin_block([float(v) for v in P[b[0]]], [float(v) for v in R[b[0]]],
                                  [float(v) for v in P[b[1]]] if b[1] >= 0 else None, [float(v) for v in case["data"][i]])
        xs[i] = x
        l2 = h2 = 0.0
        if travel is not None:
            act, e2, l2s, h2s = twin_stop(x, float(travel[i][0]), float(travel[i][1]))
            active[i] = act
            if act:
                e[2], l2, h2 = e2, l2s, h2s
        driven = slider_motor_applies(case, motor, i, active)
        if driven:
            l2, h2 = -float(motor[i][1]), float(motor[i][1])
        J0[i], J1[i], err[3 * i:3 * i + 3], is_eq[3 * i:3 * i + 3] = j0, j1, e, [1, 1, 0]
        lo[3 * i + 2], hi[3 * i + 2] = l2, h2
        dti, erpi = float(dts[i]), float(erps[i])
        if dti == 0.0:
            continue
        u = [[0.0] * 6, [0.0] * 6]
        for side in range(2):
            if b[side] < 0:
                continue
            for r in range(6):
                vel = float(case["v"][b[side]][r] if r < 3 else case["w"][b[side]][r - 3])
                u[side][r] = vel / dti + jr._dot6([float(v) for v in Minv[b[side]][6 * r:6 * r + 6]], [float(v) for v in f[b[side]]])
        kk = -erpi / dti / dti
        for r in range(3):
            ju = jr._dot6(j0[6 * r:6 * r + 6], u[0]) + jr._dot6(j1[6 * r:6 * r + 6], u[1])
            rhs[3 * i + r] = float(motor[i][0]) / dti - ju if r == 2 and driven else kk * e[r] - ju
    return dict(J0=J0, J1=J1, err=err, lo=lo, hi=hi, rhs=rhs, is_eq=is_eq, active=active, x=xs)


def check_twin(case, asm, tw, motor=None):
    """The twin within its bounds of the reference (asm from assemble_reference with the same travel table): J, err and
    rhs by tolerance; the bounds, the row types and the stops' activity exactly.  The worst error / tolerance ratios."""
    r = {"J": max(asm["J0"].worst(tw["J0"])[0], asm["J1"].worst(tw["J1"])[0]), "err": asm["err"].worst(tw["err"])[0],
         "rhs": rhs_reference(case, asm, motor).worst(tw["rhs"])[0]}
    lo, hi = bounds_reference(case, asm, motor)
    assert np.array_equal(tw["active"], asm["active"])
    assert np.array_equal(tw["is_eq"], asm["is_eq"]) and np.array_equal(tw["lo"], lo) and np.array_equal(tw["hi"], hi)
    return r


# ---- generated cases ---------------------------------------------------------------------------------------------------------
def slider_data(p0, R0, axis_world, D, p1=None):
    """data [7] of a slider along the world direction given whose D = p0 + R0 c - p1 (p0 - c for a world side) is the
    vector given, at the current pose."""
    R0 = np.asarray(R0, np.float64).reshape(3, 3)
    a = np.asarray(axis_world, np.float64)
    a0 = R0.T @ (a / np.linalg.norm(a))
    a0 /= np.linalg.norm(a0)
    p0, D = np.asarray(p0, np.float64), np.asarray(D, np.float64)
    c = R0.T @ (D - p0 + np.asarray(p1, np.float64)) if p1 is not None else p0 - D
    return np.concatenate([a0, c, np.zeros(1)])


TRAVELS = (0.4, -0.3, 0.0, 1.7, -2.2)      # the travel x of slider number k, cycling


def make_case(seed, n, m, offset=0, minv="iso", dt=5e-3, erp=0.2):
    """jr.make_case with its two-body ball joints ("joint") turned into two-body sliders and its world-side locks
    ("lock_world") into world-side sliders: every list of at least eight rows holds the kinds 0, 1, 2, 3 and 5.  A slider
    stands at travel TRAVELS[k % 5] with up to 0.05 across the rail (err != 0), so c != 0; every third rail direction
    lies within 1e-2 rad of -z.  Redrawn (seed + 1000) while a rail direction lies inside the antiparallel branch."""
    while True:
        case, motor = jr.make_case(seed, n, m, offset, minv, dt, erp)
        rng = np.random.default_rng(seed + 29)
        kind, data, body1 = case["kind"].copy(), case["data"].copy(), case["body1"].copy()
        ns, ok = 0, True
        for i in range(m):
            if case["names"][i] not in ("joint", "lock_world"):
                continue
            b0, b1 = int(case["body0"][i]), int(body1[i])
            if b0 < 0 or (case["names"][i] == "joint" and (b1 < 0 or b1 == b0)):
                continue
            s = rng.normal(size=3)
            if ns % 3 == 2:
                phi = rng.uniform(0, 2 * math.pi)
                s = np.array([math.sin(1e-2) * math.cos(phi), math.sin(1e-2) * math.sin(phi), -math.cos(1e-2)])
            s /= np.linalg.norm(s)
            across = np.cross(s, rng.normal(size=3))
            D = TRAVELS[ns % len(TRAVELS)] * s + rng.uniform(-0.05, 0.05) * across / np.linalg.norm(across)
            ns += 1
            kind[i] = SLIDER
            data[i] = slider_data(case["p"][b0], case["R"][b0], s, D, case["p"][b1] if b1 >= 0 else None)
            sw = case["R"][b0].reshape(3, 3) @ data[i, 0:3]
            ok = ok and 1.0 + sw[2] / np.linalg.norm(sw) > 1e-9
        if ok and ns > 0:
            break
        seed += 1000
    return dict(case, kind=kind, data=data, body1=body1), motor


# (xlo - x, xhi - x) per slider, cycling from the family's offset; None: no stop on that side
STOPS = [(-0.5, -0.1), (0.1, 0.5), (-0.2, 0.3), (None, -0.1), (0.1, None), (None, 0.1), (-0.1, None), (None, None)]
FAMILIES = {"upper": (0, 1), "lower": (1, 1), "inside": (2, 1), "one-sided": (3, 4), "all-infinite": (7, 1), "mixed": (0, 8)}


def make_travel(case, family):
    """travel [m][2] for the sliders of a case: slider number k takes STOPS[start + k % span] about its own travel (the
    twin's x); the rows of the other kinds hold stops too (they are ignored).  Every slider at least MARGIN from its
    stops, by the reference's x."""
    start, span = FAMILIES[family]
    m = case["kind"].shape[0]
    tw = twin_assemble(case)
    travel = np.tile([-0.25, 0.25], (m, 1))
    k = 0
    for i in range(m):
        if case["kind"][i] != SLIDER:
            continue
        a, b = STOPS[start + k % span]
        k += 1
        travel[i] = (-INF if a is None else tw["x"][i] + a, INF if b is None else tw["x"][i] + b)
    return travel


# (id, seed, n, m, offset, minv): 4 bodies and 8 constraints holding all five kinds, two-body and world-side sliders, on
# the three mass forms; one list that crosses assemble_kernel's 256-thread block
CASES = [("n4m8-a", 501, 4, 8, 0, "iso"), ("n4m8-b", 502, 4, 8, 3, "aniso"), ("n4m8-c", 503, 4, 8, 5, "coupled"),
         ("m259", 504, 9, 259, 0, "iso")]
IDS = [c[0] for c in CASES]
_cache = {}


def generated(cid):
    """(case, motor): once per process; leave them unchanged."""
    if cid not in _cache:
        _, seed, n, m, off, minv = CASES[IDS.index(cid)]
        _cache[cid] = make_case(seed, n, m, off, minv)
    return _cache[cid]


_twins = {}


def twin(cid, with_motor=False, family=None, each=None):
    """The twin of a generated case under the tables named, cached."""
    key = (cid, with_motor, family, each is not None)
    if key not in _twins:
        case, motor = generated(cid)
        dt, erp = each if each is not None else (None, None)
        _twins[key] = twin_assemble(case, motor if with_motor else None, make_travel(case, family) if family else None, dt=dt, erp=erp)
    return _twins[key]
