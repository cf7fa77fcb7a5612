"""Restitution (egs_problem_set_restitution) as mathematics and as an fp64 twin.

The reference extends tests/model_reference.py (imported unchanged): the normal row of a bouncing contact becomes

    rhs[2] = max(kk err[2], -rest vn / dt) - J (v/dt + M^-1 f),    vn = J0 row 2 . (v0, w0) + J1 row 2 . (v1, w1),

the second term taking part only where vn < -vth.  In mpmath at 50 digits, from the reference's own Jacobian.  Where
the bounce wins, the row's magnitude sum gains the bounce term's own, rest sum |J| |s| / dt, and its tolerance becomes

    32u mag' + (J tolerance of the row) |v/dt + M^-1 f|_1 + (J tolerance of row 2) |s|_1 rest / dt:

the bounce term is a 12-term product sum like the rest of the row (the existing factor 32u covers it), and an error of
the Jacobian entries moves it by at most that error times |s|_1 rest / dt.

The twin restates the device's operation order (include/eggshell_amd.h) in plain Python floats, which never contract
a multiply and an add: given the fp64 blocks and error the assembly made, its rhs is the device's bit for bit.

Both take their decisions (vn < -vth, b > t) independently, the reference in exact arithmetic and the twin in fp64; the
generators redraw any case in which a decision lies within 1e-9 relative of a tie, so the two agree on every
generated case and none has to be skipped."""
import mpmath as mp
import numpy as np

import model_reference as mr

COEFFICIENTS = (-1.0, 0.0, 0.3, 1.0, 1.7)
TIE = 1e-9
PATTERNS = ["contact_w0", "contact_w1", "contact", "joint", "+z", "contact_w0", "joint_world", "near0.1", "contact", "-x"]


def _dot6(a, b):
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]


def twin_rhs(case, J0, J1, err, rest, vth, dt=None, erp=None):
    """rhs [3m] in fp64 with the device's operation order.  J0, J1 [m][18] and err [3m]: the fp64 values of the
    assembly.  rest [m] or None (off).  dt / erp: scalars (default: the case's) or one value per constraint (the _each
    form); a constraint with dt 0 sits out, rows 0.  Also returns per constraint what was decided: 'joint', 'off'
    (rest < 0 or no table), 'slow' (vn >= -vth), 'floor' (b <= t) or 'bounce', and the pair of tie margins."""
    m = case["kind"].shape[0]
    J0 = np.asarray(J0, np.float64).reshape(m, 18); J1 = np.asarray(J1, np.float64).reshape(m, 18)
    err = np.asarray(err, np.float64).reshape(-1)
    dts = np.broadcast_to(np.float64(case["dt"] if dt is None else dt), (m,)) if np.ndim(dt) == 0 else np.asarray(dt, np.float64)
    erps = np.broadcast_to(np.float64(case["erp"] if erp is None else erp), (m,)) if np.ndim(erp) == 0 else np.asarray(erp, np.float64)
    Minv, f = case["Minv"].reshape(-1, 36), case["f_ext"].reshape(-1, 6)
    rhs = np.zeros(3 * m)
    what, margin = [], []
    for i in range(m):
        dti, erpi = float(dts[i]), float(erps[i])
        b = (int(case["body0"][i]), int(case["body1"][i]))
        if dti == 0.0:
            what.append("sits"); margin.append((np.inf, np.inf))
            continue
        u, s = [[0.0] * 6, [0.0] * 6], [[0.0] * 6, [0.0] * 6]
        for side in range(2):
            if b[side] < 0:
                continue
            for r in range(6):
                vel = float(case["v"][b[side]][r] if r < 3 else case["w"][b[side]][r - 3])
                s[side][r] = vel
                u[side][r] = vel / dti + _dot6([float(x) for x in Minv[b[side]][6 * r:6 * r + 6]], [float(x) for x in f[b[side]]])
        j0, j1 = [float(x) for x in J0[i]], [float(x) for x in J1[i]]
        kk = -erpi / dti / dti
        for r in range(3):
            ju = _dot6(j0[6 * r:6 * r + 6], u[0]) + _dot6(j1[6 * r:6 * r + 6], u[1])
            rhs[3 * i + r] = kk * float(err[3 * i + r]) - ju
        if case["kind"][i] != mr.CONTACT:
            what.append("joint"); margin.append((np.inf, np.inf))
            continue
        if rest is None or not float(rest[i]) >= 0:
            what.append("off"); margin.append((np.inf, np.inf))
            continue
        vn = _dot6(j0[12:18], s[0]) + _dot6(j1[12:18], s[1])
        t = kk * float(err[3 * i + 2])
        m1 = abs(vn + vth) / max(abs(vn), vth, 1e-300)
        if vn < -vth:
            bb = (-(float(rest[i]) * vn)) / dti
            m2 = abs(bb - t) / max(abs(bb), abs(t), 1e-300)
            if bb > t:
                t = bb
                what.append("bounce")
            else:
                what.append("floor")
            margin.append((m1, m2))
        else:
            what.append("slow"); margin.append((m1, np.inf))
        ju = _dot6(j0[12:18], u[0]) + _dot6(j1[12:18], u[1])
        rhs[3 * i + 2] = t - ju
    return rhs, what, margin


def rhs_reference(case, asm, rest, vth):
    """mr.rhs_reference with restitution: (Checked [3m], decisions [m] as twin_rhs names them).  No contact of the case
    may lie inside the antiparallel branch (the generators here draw none)."""
    assert not asm["branch"].any()
    out = mr.rhs_reference(case, asm)
    m = case["kind"].shape[0]
    what = []
    with mp.workdps(mr.DPS):
        dt, erp = mp.mpf(float(case["dt"])), mp.mpf(float(case["erp"]))
        kk = erp / (dt * dt)
        v, w = [mr._v(x) for x in case["v"]], [mr._v(x) for x in case["w"]]
        for i in range(m):
            if case["kind"][i] != mr.CONTACT:
                what.append("joint"); continue
            if rest is None or not float(rest[i]) >= 0:
                what.append("off"); continue
            e = mp.mpf(float(rest[i]))
            vn, bmag, jtol, s1 = mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(0)
            for Jc, bodies in ((asm["J0"], case["body0"]), (asm["J1"], case["body1"])):
                b = int(bodies[i])
                if b < 0:
                    continue
                s = v[b] + w[b]
                row, tol = Jc.val[18 * i + 12:18 * i + 18], Jc.tol[18 * i + 12:18 * i + 18]
                vn += sum(row[k] * s[k] for k in range(6))
                bmag += sum(abs(row[k]) * abs(s[k]) for k in range(6))
                jtol = max(jtol, max(tol))
                s1 += sum(abs(x) for x in s)
            if not vn < -mp.mpf(float(vth)):
                what.append("slow"); continue
            t = -kk * asm["err"].val[3 * i + 2]
            bnc = -e * vn / dt
            if not bnc > t:
                what.append("floor"); continue
            what.append("bounce")
            k = 3 * i + 2
            rest_of_tol = out.tol[k] - 32 * mr.U * out.mag[k]      # the J tolerance of the row times |u|_1
            mag = out.mag[k] + e * bmag / dt
            out.put(k, out.val[k] - t + bnc, mag, 32 * mr.U * mag + rest_of_tol + jtol * s1 * e / dt)
    return out, what


# ---- generated cases ----------------------------------------------------------------------------------------------------
# (id, seed, n, m, vth): one lane with the world on either side; a block plus one; two blocks plus one
CASES = [("m1-w0", 101, 4, 1, 0.25), ("m1-w1", 102, 5, 1, 0.25), ("m1-two", 103, 5, 1, 0.0), ("m40", 104, 9, 40, 0.3),
         ("m257", 105, 12, 257, 0.3), ("m513", 106, 20, 513, 0.5)]
IDS = [c[0] for c in CASES]
_OFFSET = {"m1-w0": 0, "m1-w1": 1, "m1-two": 2}
_cache = {}


def _draw(seed, n, m, offset):
    case = mr.make_case(seed, n, m, patterns=PATTERNS, offset=offset, pos_scale=1.0, minv="aniso" if seed % 2 else "iso",
                        dt=5e-3, erp=0.2)
    rng = np.random.default_rng(seed + 7)
    case["data"][:, 6] = np.where(rng.uniform(size=m) < 0.5, case["data"][:, 6], case["data"][:, 6] * 30.0)   # deep ones: the floor wins
    rest = np.array([COEFFICIENTS[(i + seed) % len(COEFFICIENTS)] for i in range(m)])
    return case, rest


def generated(cid):
    """(case, rest, vth, J0, J1, err, twin rhs, decisions): drawn once per process; leave them unchanged.  J0, J1, err
    are the oracle's fp64 assembly (oracle/model.c, the bits of the device's).  Redrawn (seed + 1000, ..) until no
    decision of the twin lies within TIE of a tie."""
    if cid not in _cache:
        from oracle import oracle as orc
        _, seed, n, m, vth = CASES[IDS.index(cid)]
        while True:
            case, rest = _draw(seed, n, m, _OFFSET.get(cid, 0))
            J0, J1, _, _, _, err = orc.assemble(case["p"], case["R"], case["kind"], case["body0"], case["body1"], case["data"])
            rhs, what, margin = twin_rhs(case, J0, J1, err, rest, vth)
            if min(min(a, b) for a, b in margin) > TIE:
                break
            seed += 1000
        _cache[cid] = (case, rest, vth, J0, J1, err, rhs, what)
    return _cache[cid]


def impact_reference(mass, vz, depth, rest, vth, dt, erp, radius=0.15):
    """A sphere of that mass falling centrally on the ground with v_z = vz < 0, one contact (world on side 0, normal
    +z, the point straight below the centre), under gravity: the exact solution of the one-row complementarity problem
    of the step, cfm 0, in mpmath.  Returns (v_z', the normal row's rhs, its tolerance, what was decided)."""
    case = dict(p=np.array([[0.0, 0.0, radius - depth]]), R=np.eye(3).reshape(1, 9), v=np.array([[0.0, 0.0, vz]]),
                w=np.zeros((1, 3)), Minv=np.diag([1.0 / mass] * 3 + [10.0] * 3).reshape(1, 36),
                f_ext=np.array([[0.0, 0.0, mass * mr.GRAVITY[2], 0.0, 0.0, 0.0]]), kind=np.ones(1, np.int32),
                body0=np.full(1, -1, np.int32), body1=np.zeros(1, np.int32),
                data=np.array([[0.0, 0.0, -depth, 0.0, 0.0, 1.0, depth]]), dt=dt, erp=erp)
    asm = mr.assemble_reference(case)
    rr, what = rhs_reference(case, asm, None if rest is None else np.array([rest]), vth)
    with mp.workdps(mr.DPS):
        J = asm["J1"].val[12:18]
        M = mr._v(case["Minv"][0]); M = [M[6 * r:6 * r + 6] for r in range(6)]
        f = mr._v(case["f_ext"][0])
        A = sum(J[r] * sum(M[r][c] * J[c] for c in range(6)) for r in range(6))
        lam = max(mp.mpf(0), rr.val[2] / A)
        g = [f[c] + J[c] * lam for c in range(6)]
        vnew = [mp.mpf(float(([0.0, 0.0, vz] + [0.0] * 3)[r])) + mp.mpf(float(dt)) * sum(M[r][c] * g[c] for c in range(6)) for r in range(6)]
        return vnew[2], rr.val[2], rr.tol[2], what[0], lam
