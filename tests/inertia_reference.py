"""A 40-digit statement (mpmath) of what Ensemble::Init computes per body from R, I_b and w (ensembles.cc:202-222):
I_g = R I_b R^T, its inverse, and the gyroscopic torque -w x (I_g w) -- and seeded families of inputs to hold the CPU
oracle's minv_blocks / external_force to it.  The device's live_mass_kernel is bit-equal to those oracle functions, so
what is certified here is certified for the device.

Errors are reported in units of kappa(I_b) * u, u = 2^-53:
  inverse:  max |M - M_ref| / max |M_ref|
  torque:   max |t - t_ref| / (max |I_g| * |w|^2), with an absolute floor of 8 * 2^-1074 (w = 1e-170: the products
            underflow; a result below the smallest subnormal rounds to zero, each of the few roundings by at most that)
"""
import mpmath as mp
import numpy as np

U = 2.0 ** -53
TINY = 8 * 2.0 ** -1074
SPINS = (0.0, 1e-170, 1.0, 50.0, 1400.0)


def reference(R, I_body, w):
    """(I_g^-1, gyroscopic torque) of one body as mpmath matrices, 40 digits."""
    with mp.workdps(40):
        Rm = mp.matrix(3, 3)
        Ib = mp.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                Rm[i, j] = mp.mpf(float(R[3 * i + j]))
                Ib[i, j] = mp.mpf(float(I_body[3 * i + j]))
        wv = mp.matrix([mp.mpf(float(x)) for x in w])
        Ig = Rm * Ib * Rm.T
        Lw = Ig * wv
        tq = mp.matrix([-(wv[1] * Lw[2] - wv[2] * Lw[1]), -(wv[2] * Lw[0] - wv[0] * Lw[2]), -(wv[0] * Lw[1] - wv[1] * Lw[0])])
        return mp.inverse(Ig), tq, Ig


def errors(R, I_body, w, Minv_block, torque):
    """The two errors of one body's computed values, in units of kappa(I_b) u; the torque's absolute part separately:
    (err_inverse, err_torque, torque_within_floor)."""
    inv_ref, tq_ref, Ig = reference(R, I_body, w)
    kappa = np.linalg.cond(np.asarray(I_body, np.float64).reshape(3, 3))
    with mp.workdps(40):
        M = np.asarray(Minv_block, np.float64).reshape(6, 6)
        dm = max(abs(mp.mpf(float(M[3 + i, 3 + j])) - inv_ref[i, j]) for i in range(3) for j in range(3))
        sm = max(abs(inv_ref[i, j]) for i in range(3) for j in range(3))
        e_inv = float(dm / sm) / (kappa * U)
        dt = max(abs(mp.mpf(float(torque[k])) - tq_ref[k]) for k in range(3))
        w2 = sum(mp.mpf(float(x)) ** 2 for x in w)
        scale = max(abs(Ig[i, j]) for i in range(3) for j in range(3)) * w2
        if dt <= mp.mpf(TINY):
            return e_inv, 0.0, True
        return e_inv, float(dt / scale) / (kappa * U), False


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])


def box_inertia(a, b, c, m=1.0):
    return np.array([m * (b * b + c * c) / 12.0, m * (a * a + c * c) / 12.0, m * (a * a + b * b) / 12.0])


# principal inertias from kappa = 1 (a cube) to the 0.02 x 0.02 x 1 rod (kappa 1250.5)
PRINCIPAL = (box_inertia(0.3, 0.3, 0.3), box_inertia(0.1, 0.3, 0.6), box_inertia(0.05, 0.2, 0.9), box_inertia(0.02, 0.02, 1.0))


def families(seed=20240607, per_cell=3):
    """Seeded cases (R, I_body, w), each a flat array: every principal set, diagonal and full symmetric, every spin, R
    exactly as the quaternion formula gives it and up to 1e-6 off orthonormal."""
    rng = np.random.default_rng(seed)
    out = []
    for d in PRINCIPAL:
        for full in (False, True):
            for spin in SPINS:
                for off in (0.0, 1e-6):
                    for _ in range(per_cell):
                        if full:
                            Q = _rotation(rng).reshape(3, 3)
                            I = Q @ np.diag(d) @ Q.T
                            I = (I + I.T) / 2.0      # exactly symmetric
                        else:
                            I = np.diag(d)
                        R = _rotation(rng) + off * rng.uniform(-1, 1, 9)
                        ax = rng.normal(size=3)
                        out.append((R, I.reshape(9), spin * ax / np.linalg.norm(ax)))
    return out
