"""Synthetic systems for the direct relaxation solve (egs_relax_blocks_direct): random block systems in every size
class of stabilize_direct.hip (<= 48 rows on one wavefront, <= 126 rows in LDS, <= 1024 rows in a global workspace),
diagonal systems on which every operation of the kernel is exact, and the reference: the minimum-norm solution of
J x = err, which is J^T (J J^T)^+ err, from the SVD of J itself rather than of the squared system."""
import numpy as np

SEED = 43   # chosen so that every case of the table is well conditioned (tests/test_relax_direct_reference_cpu.py)

# (m constraints, n bodies, exact duplicates, both-anchored constraints, consistent err): 3, 3, 48, 48, 51, 126, 129,
# 129, 129, 360, 1023 and 1023 rows -- both sides of 48 and of 126, and the largest system the route accepts
CASES = [(1, 1, 0, 0, False), (1, 2, 0, 0, False), (16, 3, 0, 0, False), (16, 12, 0, 0, False), (17, 4, 0, 0, False),
         (42, 6, 4, 1, False), (43, 8, 0, 0, False), (43, 8, 0, 0, True), (43, 30, 0, 0, False), (120, 20, 10, 0, False),
         (341, 50, 0, 0, False), (341, 50, 20, 0, True)]


def case_id(case):
    m, n, dup, both, consistent = case
    return "m%d-n%d-dup%d-both%d%s" % (m, n, dup, both, "-consistent" if consistent else "")


def dense_J(n, body0, body1, J0, J1):
    m = body0.shape[0]
    J = np.zeros((3 * m, 6 * n))
    for i in range(m):
        for b, blk in ((body0[i], J0[i]), (body1[i], J1[i])):
            if b >= 0:
                J[3 * i:3 * i + 3, 6 * b:6 * b + 6] = blk.reshape(3, 6)
    return J


def block_system(m, n, seed, anchored=0.2, dup=0, both_anchored=0, consistent=False):
    """m constraints on n bodies with standard normal blocks: body0 uniform in [0, n), body1 another body (-1 when
    there is one body only), a fraction `anchored` of the constraints with body0 = -1, `dup` of the m constraints exact
    copies (bodies and blocks) of others, `both_anchored` of them with -1 on both sides (zero rows), all in a shuffled
    order.  err = J (standard normal) when consistent, otherwise standard normal.
    Returns body0, body1, J0 [m,18], J1 [m,18], err [3m] and the dense J [3m, 6n]."""
    rng = np.random.default_rng(seed)
    base = m - dup - both_anchored
    assert base >= 1 or dup == 0
    body0 = np.zeros(m, np.int32)
    body1 = np.zeros(m, np.int32)
    J0 = rng.standard_normal((m, 18))
    J1 = rng.standard_normal((m, 18))
    for i in range(base):
        a = int(rng.integers(0, n))
        if n == 1:
            b = -1
        else:
            b = int(rng.integers(0, n - 1))
            b += b >= a
            if rng.uniform() < anchored:
                a = -1
        body0[i], body1[i] = a, b
    for i in range(base, base + dup):
        src = int(rng.integers(0, base))
        body0[i], body1[i], J0[i], J1[i] = body0[src], body1[src], J0[src], J1[src]
    body0[base + dup:] = -1
    body1[base + dup:] = -1
    order = rng.permutation(m)
    body0, body1, J0, J1 = body0[order], body1[order], J0[order], J1[order]
    J0[body0 < 0] = 0.0
    J1[body1 < 0] = 0.0
    J = dense_J(n, body0, body1, J0, J1)
    err = J @ rng.standard_normal(6 * n) if consistent else rng.standard_normal(3 * m)
    return body0, body1, J0, J1, err, J


def diag_system(scales):
    """One constraint per body, body0 = -1, body1 = i, J0 = 0 and row r of J1 = scales[3 i + r] e_r, so that
    J J^T = diag(scales^2).  Returns body0, body1, J0, J1 and the dense J."""
    scales = np.asarray(scales, np.float64)
    n = scales.shape[0] // 3
    assert scales.shape[0] == 3 * n
    body0 = np.full(n, -1, np.int32)
    body1 = np.arange(n, dtype=np.int32)
    J0 = np.zeros((n, 18))
    J1 = np.zeros((n, 18))
    for i in range(n):
        for r in range(3):
            J1[i, 6 * r + r] = scales[3 * i + r]
    return body0, body1, J0, J1, dense_J(n, body0, body1, J0, J1)


def min_norm(J, err):
    """The minimum-norm least-squares solution of J x = err: J^T (J J^T)^+ err without forming J J^T."""
    return np.linalg.lstsq(J, err, rcond=1e-9)[0]


DIAG_ROWS = (3, 48, 51, 126, 129, 1023)
DIAG_TOL = 2.0 ** -20
# exponents e of the scales 2^e.  The pivots are 4^e against a first pivot of 4^3: e = -7 gives exactly DIAG_TOL times
# the first pivot (truncated: the test is <=), e = -6 the next power above it (kept), e = -9 lies below; all of them
# are above the default 1e-10 (4^-12 = 6e-8 of the first pivot).  Every value but the largest comes in runs: ties.
DIAG_EXPONENTS = (3, 2, 2, 0, 0, 0, -1, -6, -6, -7, -7, -9)


def diag_scales(rows, seed=SEED):
    """Powers of two in a shuffled order that hold every exponent of DIAG_EXPONENTS (3 rows: the largest, the one at
    the threshold and the one above it, the largest not in front), and a standard normal err."""
    rng = np.random.default_rng(seed + rows)
    if rows == 3:
        e = np.array([-7, 3, -6])
    else:
        e = np.concatenate([np.array(DIAG_EXPONENTS), rng.choice(np.array(DIAG_EXPONENTS[1:]), rows - len(DIAG_EXPONENTS))])
        e = e[rng.permutation(rows)]
        if e[0] == 3:
            e[[0, rows - 1]] = e[[rows - 1, 0]]
    return np.ldexp(1.0, e), rng.standard_normal(rows)


def diag_closed_form(scales, err, rank_tol):
    """What the truncated solve gives on diag(scales^2): y_i = err_i / scales_i^2 where scales_i^2 > rank_tol * max,
    0 elsewhere; every operation is exact but the division, which is the same correctly rounded one."""
    d = scales * scales
    keep = d > rank_tol * d.max()
    y = np.zeros_like(err)
    y[keep] = err[keep] / d[keep]
    return y, int(keep.sum())


TIED_BODIES = (12, 13, 32, 255)   # 48, 54, 129 and 1020 rows


def tied_pair_system(n, seed=SEED):
    """diag_system of n bodies with every third constraint given once more (same body, same block) and small
    integer err: pairs of exactly equal rows, of which the pivot search must take the one at the lower position and
    the elimination leaves an exact zero on the other; the completion's Gram matrix is diag(1 or 2).  Every operation
    is exact in fp64, so any correct implementation of the stated pivot rule gives the same bits.
    Returns n, body0, body1, J0, J1, err, J."""
    rng = np.random.default_rng(seed + 1000 + n)
    scales = np.ldexp(1.0, rng.integers(-3, 4, 3 * n))
    body0, body1, J0, J1, _ = diag_system(scales)
    again = np.arange(0, n, 3)
    order = rng.permutation(n + again.shape[0])
    body0 = np.concatenate([body0, body0[again]])[order]
    body1 = np.concatenate([body1, body1[again]])[order]
    J0 = np.concatenate([J0, J0[again]])[order]
    J1 = np.concatenate([J1, J1[again]])[order]
    err = rng.integers(1, 9, 3 * body0.shape[0]).astype(np.float64) * rng.choice([-1.0, 1.0], 3 * body0.shape[0])
    return n, body0, body1, J0, J1, err, dense_J(n, body0, body1, J0, J1)
