"""A plain sequential restatement of the friction pyramid's sweeps (tests/friction_reference.py) in numpy fp64 / fp32 on
the dense A: every operation of the scalar recurrence rounded once in the working precision, nothing reordered for
speed.  It exists to measure, on the CPU, what a straightforward fp64 / fp32 implementation loses against the 50-digit
reference (the bounds of DESIGN.md section 6d); it is not an oracle for the device's bits."""
import numpy as np

import sweep_reference as ref
from helpers import dense_numpy


def dense_held(s, cfm, f32):
    """(A, J, W, T): helpers.dense_numpy of the inputs as the code under test holds them, in the working type T."""
    import types
    T = np.float32 if f32 else np.float64
    h = types.SimpleNamespace(n=s.n, m=s.m, body0=s.body0, body1=s.body1, Minv=ref.held(s.Minv, f32).reshape(s.n, 36),
                              J0=ref.held(s.J0, f32).reshape(s.m, 18), J1=ref.held(s.J1, f32).reshape(s.m, 18))
    A, J, W = dense_numpy(h, float(ref.held(cfm, f32)))
    return A.astype(T), J.astype(T), W.astype(T), T


def sweeps(s, rhs, cfm, mu, method, omega, K, f32=False, x0=None):
    """K sweeps; returns x, the accumulators W J^T x, w = A x - rhs and the residual of the pyramid's rule, all
    computed in the working precision (the residual's sums in fp64, as the device's)."""
    A, J, W, T = dense_held(s, cfm, f32)
    b = np.asarray(rhs).astype(T)
    x = (b if x0 is None else np.asarray(x0).astype(T)).copy()
    lo, hi, mu = np.asarray(s.lo).astype(T), np.asarray(s.hi).astype(T), np.asarray(mu).astype(T)
    k = T(1) / T(omega) if method == ref.SOR else T(1)
    R = b.shape[0]
    d = np.diag(A).copy()
    order = range(R - 1, -1, -1) if method == ref.SOR else range(R)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(K):
            src = x.copy() if method == ref.JACOBI else x
            for r in order:
                t = src[r] + (b[r] - A[r] @ src) / (k * d[r])
                i, rr = divmod(r, 3)
                if rr < 2 and mu[i] >= 0:
                    xn = src[3 * i + 2]
                    bd = mu[i] * xn if xn > 0 else T(0)
                    t = min(max(t, -bd), bd)
                elif not s.is_eq[r]:
                    t = min(max(t, lo[r]), hi[r])
                x[r] = t
        w = A @ x - b
        a = W @ (J.T @ x)
    return x, a, w, residual(x, w, s.is_eq, lo, hi, mu)


def residual(x, w, is_eq, lo, hi, mu):
    e = qa = qb = qc = 0.0
    for r in range(x.shape[0]):
        wr = float(w[r])
        i, rr = divmod(r, 3)
        if rr < 2 and mu[i] >= 0:
            xn = x[3 * i + 2]
            bd = mu[i] * xn if xn > 0 else type(xn)(0)
            ax = abs(x[r])
            if ax < bd:
                qc += wr * wr
            elif ax > bd:
                qc += (float(ax) - float(bd)) ** 2
            elif bd > 0:
                if x[r] > 0 and wr > 0:
                    qb += wr * wr
                if x[r] < 0 and wr < 0:
                    qa += wr * wr
        elif is_eq[r]:
            e += wr * wr
        else:
            if x[r] == lo[r] and wr < 0:
                qa += wr * wr
            if x[r] == hi[r] and wr > 0:
                qb += wr * wr
            if lo[r] < x[r] < hi[r]:
                qc += wr * wr
    return float(np.sqrt(e) + np.sqrt(qa) + np.sqrt(qb) + np.sqrt(qc))
