"""Warm start, restated as plainly as possible in numpy (no GPU): the contact matcher of
eggshell_amd/csrc/warm_start.h, a dense projected Jacobi / GS / backward-SOR that accepts a start, the
reference's residual metric, and the world's step loop with and without a start taken from the previous
step's lambda.  The GPU tests compare the device against these."""
import numpy as np

from oracle import oracle as orc

NO_MATCH, NO_HISTORY = -1, -2


def match_contacts(old_b0, old_b1, old_pos, old_lambda, old_off, valid, new_b0, new_b1, new_pos, new_rhs, new_off, radius):
    """x0 [3 m_new] and source [m_new] for the new list.  Ensemble e owns old contacts old_off[e]:old_off[e+1] and
    new contacts new_off[e]:new_off[e+1].  valid[e] == 0: x0 = rhs rows, source -2.  Otherwise the old contact of the
    same ordered pair (b0, b1) in the same ensemble with the smallest squared distance <= radius^2 (a tie: the lowest
    old index) gives its lambda rows, source = its index; none: x0 = 0, source -1."""
    old_pos = np.asarray(old_pos, np.float64).reshape(-1, 3)
    new_pos = np.asarray(new_pos, np.float64).reshape(-1, 3)
    old_lambda = np.asarray(old_lambda, np.float64).reshape(-1, 3)
    new_rhs = np.asarray(new_rhs, np.float64).reshape(-1, 3)
    m_new = len(new_b0)
    x0 = np.zeros((m_new, 3))
    source = np.full(m_new, NO_MATCH, np.int32)
    r2 = np.float64(radius) * np.float64(radius)
    for e in range(len(valid)):
        for c in range(new_off[e], new_off[e + 1]):
            if not valid[e]:
                x0[c] = new_rhs[c]
                source[c] = NO_HISTORY
                continue
            best = None
            for o in range(old_off[e], old_off[e + 1]):
                if old_b0[o] != new_b0[c] or old_b1[o] != new_b1[c]:
                    continue
                d = new_pos[c] - old_pos[o]
                d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if d2 <= r2 and (best is None or d2 < best):
                    best = d2
                    source[c] = o
            if source[c] >= 0:
                x0[c] = old_lambda[source[c]]      # the rows themselves: -0.0 and denormals survive
    return x0.reshape(-1), source


def residual(A, b, x, is_eq, lo, hi):
    """GetResidualError (sparse_iterations.cc:51-69) of x on the dense system."""
    w = A @ x - b
    eq = np.asarray(is_eq).astype(bool)
    at_lo = ~eq & (x == lo) & (w < 0)
    at_hi = ~eq & (x == hi) & (w > 0)
    inside = ~eq & (x > lo) & (x < hi)
    n = lambda mask: np.sqrt(np.sum(w[mask] ** 2))
    return n(eq) + (n(at_lo) + n(at_hi) + n(inside))


def pgs(A, b, is_eq, lo, hi, method, omega, iters, x0=None, tol=0.0):
    """Scalar projected Jacobi (0) / Gauss-Seidel (1) / backward SOR (2) on a dense matrix, as helpers.numpy_pgs,
    from x0 (None: b, quirk Q7).  tol > 0: the reference's stopping rule (x0 is tested first).  Returns x, sweeps."""
    R = b.shape[0]
    x = (b if x0 is None else np.asarray(x0, np.float64)).copy()
    k = 1.0 / omega
    d = np.diag(A).copy()
    it = 0
    while it < iters and not (tol > 0 and not residual(A, b, x, is_eq, lo, hi) > tol):
        if method == 0:
            xn = x.copy()
            for r in range(R):
                t = (b[r] - (A[r] @ x - d[r] * x[r])) / d[r]
                xn[r] = t if is_eq[r] else min(max(t, lo[r]), hi[r])
            x = xn
        elif method == 1:
            for r in range(R):
                t = (b[r] - (A[r] @ x - d[r] * x[r])) / d[r]
                x[r] = t if is_eq[r] else min(max(t, lo[r]), hi[r])
        else:
            for r in range(R - 1, -1, -1):
                t = (b[r] - (A[r] @ x - d[r] * x[r]) - (1 - k) * d[r] * x[r]) / (k * d[r])
                x[r] = t if is_eq[r] else min(max(t, lo[r]), hi[r])
        it += 1
    return x, it


def stack_scene(n=3, z0=0.15, pitch=0.3):
    """n unit-mass 0.3 cubes on top of each other, resting: R = I, v = 0, I = 0.1."""
    p = np.array([[0.0, 0.0, z0 + pitch * k] for k in range(n)])
    R = np.tile(np.eye(3).reshape(9), (n, 1))
    return p, R


def step_loop(contacts, p, R, steps, warm, method, sweeps, tol=1e-9, dt=0.005, erp=0.2, cfm=0.01, radius=0.01):
    """The world's loop of contacts only (collide, assemble, solve, integrate: tests/test_gpu_fullstep.py) with the
    dense numpy PGS.  warm: a step's solve starts from the previous step's lambda through match_contacts.
    contacts(p, R) -> b0, b1, data.  Returns per step (residual of x0, residual of the result, sweeps, m)."""
    n = p.shape[0]
    v = np.zeros((n, 3)); w = np.zeros((n, 3))
    mass = np.ones(n); I_body = np.tile((np.eye(3) * 0.1).reshape(9), (n, 1))
    Minv = orc.minv_blocks(R, mass, I_body)
    f_ext = orc.external_force(R, w, mass, I_body)
    prev = None
    out = []
    for _ in range(steps):
        b0, b1, data = contacts(p, R)
        m = len(b0)
        v6_old = np.concatenate([v, w], axis=1)
        if m == 0:
            v6 = v6_old + dt * np.einsum("brc,bc->br", Minv.reshape(n, 6, 6), f_ext)
            prev = None
            out.append((0.0, 0.0, 0, 0))
        else:
            kind = np.ones(m, np.int32)
            J0, J1, is_eq, lo, hi, err = orc.assemble(p, R, kind, b0, b1, data)
            s = orc.Sys(Minv, b0, b1, J0, J1, is_eq, lo, hi)
            rhs = orc.ode_rhs(v, w, Minv, f_ext, b0, b1, J0, J1, err, dt, erp)
            A = orc.dense_JMJt(s, cfm)
            x0 = None
            if warm:
                have = prev is not None
                ob0, ob1, opos, olam = prev if have else (b0[:0], b1[:0], data[:0, :3], np.zeros(0))
                x0, _ = match_contacts(ob0, ob1, opos, olam, [0, len(ob0)], [1 if have else 0],
                                       b0, b1, data[:, :3], rhs, [0, m], radius)
            r0 = residual(A, rhs, rhs if x0 is None else x0, is_eq, lo, hi)
            lam, it = pgs(A, rhs, is_eq, lo, hi, method, 1.5, sweeps, x0, tol)
            out.append((r0, residual(A, rhs, lam, is_eq, lo, hi), it, m))
            prev = (b0, b1, data[:, :3].copy(), lam)
            v6 = orc.velocity_update(v, w, Minv, f_ext, b0, b1, J0, J1, lam, dt)
        p, R = orc.position_update(p, R, v6_old, v6, dt)
        v, w = v6[:, :3].copy(), v6[:, 3:].copy()
    return out
