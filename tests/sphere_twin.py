"""The sphere narrow phase of collide.hip in numpy fp64, operation for operation: the statement the device must match
bit for bit (tests/test_gpu_collide_spheres.py).  Every line is one rounding, as the device's -ffp-contract=off code
is; sqrt and / are IEEE in both.  Contact rows are [7] = position, normal, depth.

Also the one-contact step loop of a ball on the ground (ball_steps), for the rolling-ball test of the world."""
import numpy as np

BOX, SPHERE = 0, 1


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _mat3_vec(A, v):
    return [(A[0] * v[0] + A[1] * v[1]) + A[2] * v[2], (A[3] * v[0] + A[4] * v[1]) + A[5] * v[2],
            (A[6] * v[0] + A[7] * v[1]) + A[8] * v[2]]


def _f(a):
    return [float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def ground_sphere(c, side):
    c, side = _f(c), _f(side)
    r = side[0] * 0.5
    qz = c[2] - r
    if not qz < 0:
        return []
    return [np.array([c[0], c[1], qz, 0.0, 0.0, 1.0, -qz])]


def collide_spheres(ci, si, cj, sj):
    ci, si, cj, sj = _f(ci), _f(si), _f(cj), _f(sj)
    ri, rj = si[0] * 0.5, sj[0] * 0.5
    d = [cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]]
    L = float(np.sqrt(_dot3(d, d)))
    s = L - (ri + rj)
    if s > 0:
        return []
    n = [0.0, 0.0, 1.0] if L == 0 else [d[0] / L, d[1] / L, d[2] / L]
    t = ((ri + L) - rj) * 0.5
    return [np.array([ci[k] + n[k] * t for k in range(3)] + n + [-s])]


def collide_sphere_box(cS, sideS, cB, RB, sideB, flip):
    """flip: the sphere is body0, so the reported normal is -n_BS."""
    cS, sideS, cB, RB, sideB = _f(cS), _f(sideS), _f(cB), _f(RB), _f(sideB)
    r = sideS[0] * 0.5
    dc = [cS[0] - cB[0], cS[1] - cB[1], cS[2] - cB[2]]
    p = [(RB[k] * dc[0] + RB[3 + k] * dc[1]) + RB[6 + k] * dc[2] for k in range(3)]
    h = [sideB[k] * 0.5 for k in range(3)]
    q = [min(max(p[k], -h[k]), h[k]) for k in range(3)]
    e = [p[k] - q[k] for k in range(3)]
    L = float(np.sqrt(_dot3(e, e)))
    if L > 0:
        if L - r > 0:
            return []
        w = _mat3_vec(RB, e)
        n = [w[k] / L for k in range(3)]
        depth = r - L
    else:
        g = [h[k] - abs(p[k]) for k in range(3)]
        k = 0
        if g[1] < g[k]:
            k = 1
        if g[2] < g[k]:
            k = 2
        sg = 1.0 if p[k] >= 0 else -1.0
        n = [sg * RB[k], sg * RB[3 + k], sg * RB[6 + k]]
        depth = g[k] + r
        q[k] = sg * h[k]
    bq = _mat3_vec(RB, q)
    fs = -1.0 if flip else 1.0
    pos = [((bq[k] + cB[k]) + (cS[k] - r * n[k])) * 0.5 for k in range(3)]
    return [np.array(pos + [fs * n[k] for k in range(3)] + [depth])]


def pair(pos, R, side, shape, i, j):
    """The contacts of bodies i < j before joint pruning; a box pair comes from the CPU oracle with its own pruning."""
    if shape[i] == SPHERE and shape[j] == SPHERE:
        return collide_spheres(pos[i], side[i], pos[j], side[j])
    if shape[i] == SPHERE:
        return collide_sphere_box(pos[i], side[i], pos[j], R[j], side[j], True)
    if shape[j] == SPHERE:
        return collide_sphere_box(pos[j], side[j], pos[i], R[i], side[i], False)
    from oracle import oracle as orc
    cs, _ = orc.collide_boxes(pos[i], R[i], pos[j], R[j], side[i], side[j])
    return [cs[a] for a in range(len(cs)) if not any(np.linalg.norm(cs[b][:3] - cs[a][:3]) < 1e-6 for b in range(a))]


def contacts(pos, R, side, shape, pairs=None):
    """The whole list in the device's order: ground contacts by body, then the pairs i < j (all of them, or `pairs`)."""
    pos, R, side = (np.asarray(a, np.float64).reshape(-1, k) for a, k in ((pos, 3), (R, 9), (side, 3)))
    n = pos.shape[0]
    b0, b1, data = [], [], []
    for b in range(n):
        if shape[b] == SPHERE:
            cs = ground_sphere(pos[b], side[b])
        else:
            from oracle import oracle as orc
            cs = orc.collide_box_ground(pos[b], R[b], side[b])
        for c in cs:
            b0.append(-1); b1.append(b); data.append(c)
    for i, j in (pairs if pairs is not None else [(i, j) for i in range(n) for j in range(i + 1, n)]):
        for c in pair(pos, R, side, shape, i, j):
            b0.append(i); b1.append(j); data.append(c)
    return np.array(b0, np.int32), np.array(b1, np.int32), np.array(data, np.float64).reshape(-1, 7)


def ball_steps(r, m, v0, steps, dt, erp, g=9.8, num=float, z0=None):
    """A ball (radius r, mass m, I = (2/5) m r^2) on the ground under gravity, started at height z0 (r) with
    velocity (v0, 0, 0) and no spin, through `steps` world steps: detect (sphere - ground), the contact's three rows
    with the friction box [-1, 1]^2 x [0, inf), ODE right-hand side with erp, the rows solved, velocities, midpoint
    positions.  With the normal (0, 0, 1) the rows' frame is the identity and J M^-1 J^T is diagonal
    (1/m + rho^2/I, 1/m + rho^2/I, 1/m, rho = contact z - centre z), so the projected solve is a division and a clamp
    per row: exact, i.e. "solved to 1e-14" with room to spare.  num = float gives fp64, num = mpmath.mpf the same loop
    at mpmath's precision on the same fp64 inputs.  Returns x, z, v_x, v_z, w_y."""
    N = num
    r, m, dt, erp, g = N(r), N(m), N(dt), N(erp), N(g)
    I = N(2) * m * r * r / N(5)
    x, z = N(0), (r if z0 is None else N(z0))
    vx, vz, wy = N(v0), N(0), N(0)
    for _ in range(steps):
        qz = z - r
        l0 = l2 = N(0)
        rho = N(0)
        if qz < 0:
            rho = qz - z
            k = -erp / dt / dt
            u = (vx / dt, vz / dt - g, wy / dt)
            rhs0 = -(u[0] + rho * u[2])            # row 0: linear (1, 0, 0), angular (0, rho, 0)
            rhs2 = k * qz - u[1]                   # row 2: err = -depth = qz
            l0 = rhs0 / (N(1) / m + rho * rho / I)
            l0 = max(N(-1), min(N(1), l0))
            l2 = max(N(0), rhs2 * m)
        nvx = vx + dt * (l0 / m)
        nvz = vz + dt * ((l2 - m * g) / m)
        nwy = wy + dt * (rho * l0 / I)
        x = x + dt * ((vx + nvx) / N(2))
        z = z + dt * ((vz + nvz) / N(2))
        vx, vz, wy = nvx, nvz, nwy
    return x, z, vx, vz, wy
