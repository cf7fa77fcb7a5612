"""CPU: the synthetic systems that tests/test_gpu_relax_direct_synthetic.py sends through egs_relax_blocks_direct are
fair, and their reference is accurate, before a device sees them.  For every case of the shared table the numpy
restatement of the device's factorisation (truncated_ldlt_solve) finds the SVD rank of J, J is well conditioned on its
range, the restatement's J^T y agrees with the minimum-norm solution of J x = err to 1e-13, and no pivot lies anywhere
near the 1e-10 threshold; the fp64 reference itself is pinned against a 40-digit SVD; on diagonal systems the
restatement reproduces the closed form bit for bit; and the two cairns of the world-level test have the row counts
that put them at the LDS limit and above it."""
import numpy as np
import pytest

from eggshell_amd import scenes
from relax_direct_cases import (CASES, DIAG_ROWS, DIAG_TOL, SEED, block_system, case_id, diag_closed_form, diag_scales,
                                diag_system, min_norm, tied_pair_system, TIED_BODIES)
from test_world_stabilize_direct_cpu import detect, system, truncated_ldlt_solve

ROWS = [3, 3, 48, 48, 51, 126, 129, 129, 129, 360, 1023, 1023]


def pivots(A, rank_tol=1e-10):
    """|pivot| / |first pivot| of the restatement's factorisation, the rejected one last (none rejected: all kept)."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    out = []
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
        d = A[k, k]
        out.append(abs(d))
        if not abs(d) > rank_tol * out[0]:
            break
        col = A[k + 1:, k].copy()
        A[k + 1:, k + 1:] -= np.outer(col / d, col)
    return np.array(out) / out[0] if out[0] > 0 else np.array(out)


def test_the_table_has_the_row_counts_of_every_class_boundary():
    assert [3 * c[0] for c in CASES] == ROWS


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_is_fair_and_the_restatement_solves_it(case):
    m, n, dup, both, consistent = case
    body0, body1, J0, J1, err, J = block_system(m, n, SEED, dup=dup, both_anchored=both, consistent=consistent)
    assert body0.shape == body1.shape == (m,) and J0.shape == J1.shape == (m, 18) and err.shape == (3 * m,)
    assert J.shape == (3 * m, 6 * n)
    assert np.count_nonzero((body0 < 0) & (body1 < 0)) == both
    assert not np.any((body0 >= 0) & (body0 == body1))
    sv = np.linalg.svd(J, compute_uv=False)
    svd_rank = int(np.count_nonzero(sv > 1e-9 * sv[0]))
    cond = sv[0] / sv[svd_rank - 1]
    A = J @ J.T
    y, rank = truncated_ldlt_solve(A, err)
    want = min_norm(J, err)
    d = np.abs(J.T @ y - want).max()
    piv = pivots(A)
    print("%s: rows %d rank %d cond %.1f  max |J^T y - min_norm| %.3e  smallest kept pivot %.2e  rejected %s"
          % (case_id(case), 3 * m, rank, cond, d, piv[:rank].min(), "%.2e" % piv[rank] if rank < 3 * m else "none"))
    assert rank == svd_rank
    assert cond <= 100.0
    assert d <= 1e-13
    assert piv[:rank].min() >= 1e-6
    if rank < 3 * m:
        assert piv.shape[0] == rank + 1 and piv[rank] <= 1e-13
    if dup:
        # every copy is exact: its rows vanish exactly in the elimination
        assert rank <= 3 * (m - dup - both)
    if rank < 3 * m and not consistent:
        y_plain, _ = truncated_ldlt_solve(A, err, complete=False)
        assert np.abs(J.T @ y_plain - want).max() > 1e-2
    if consistent:
        assert np.abs(J @ want - err).max() < 1e-12


@pytest.mark.parametrize("case,rank", [(CASES[2], 18), (CASES[4], 24)], ids=["48 rows", "51 rows"])
def test_min_norm_against_forty_digits(case, rank):
    """V S^+ U^T err from a 40-digit SVD of J: the fp64 reference is good to 1e-13."""
    import mpmath
    m, n, dup, both, consistent = case
    _, _, _, _, err, J = block_system(m, n, SEED, dup=dup, both_anchored=both, consistent=consistent)
    saved = mpmath.mp.dps
    mpmath.mp.dps = 40
    try:
        U, S, V = mpmath.svd_r(mpmath.matrix(J.tolist()), full_matrices=False, compute_uv=True)
        s = [S[i] for i in range(len(S))]
        keep = [i for i in range(len(s)) if s[i] > mpmath.mpf(10) ** -20 * s[0]]
        assert len(keep) == rank
        b = mpmath.matrix(err.tolist())
        x = mpmath.zeros(J.shape[1], 1)
        for i in keep:
            c = sum(U[r, i] * b[r] for r in range(J.shape[0])) / s[i]
            for q in range(J.shape[1]):
                x[q] += V[i, q] * c
        exact = np.array([float(x[q]) for q in range(J.shape[1])])
    finally:
        mpmath.mp.dps = saved
    d = np.abs(min_norm(J, err) - exact).max()
    print("%s: max |min_norm - 40 digits| %.3e" % (case_id(case), d))
    assert d <= 1e-13


@pytest.mark.parametrize("rows", DIAG_ROWS)
def test_diagonal_system_closed_form_bit_for_bit(rows):
    scales, err = diag_scales(rows)
    body0, body1, J0, J1, J = diag_system(scales)
    assert np.array_equal(J @ J.T, np.diag(scales * scales))
    assert np.all(body0 == -1) and np.array_equal(body1, np.arange(rows // 3)) and not J0.any()
    d = scales * scales
    assert scales[0] != scales.max()                                       # the first step swaps
    assert np.any(d == DIAG_TOL * d.max()) and np.any(d == 4.0 * DIAG_TOL * d.max())   # at the threshold, and next above
    assert rows == 3 or np.any(d < DIAG_TOL * d.max())
    assert np.all(np.log2(scales) == np.round(np.log2(scales)))
    want, want_rank = diag_closed_form(scales, err, DIAG_TOL)
    assert 0 < want_rank < rows and np.all(err[want == 0.0] != 0.0)
    y, rank = truncated_ldlt_solve(J @ J.T, err, DIAG_TOL)
    assert rank == want_rank and y.tobytes() == want.tobytes()
    full, full_rank = diag_closed_form(scales, err, 1e-10)
    assert full_rank == rows
    y, rank = truncated_ldlt_solve(J @ J.T, err)
    assert rank == rows and y.tobytes() == full.tobytes()


@pytest.mark.parametrize("n", TIED_BODIES)
def test_tied_pairs_keep_the_row_at_the_lower_position(n):
    """Exactly equal rows in pairs, every operation exact: the solution is err's mean over the pair on the row the
    lowest-index rule takes and an exact zero on the other; taking the other row of a pair would give other bits."""
    n, body0, body1, J0, J1, err, J = tied_pair_system(n)
    m = body0.shape[0]
    assert m == n + (n + 2) // 3 and 3 * m in (48, 54, 129, 1020)
    y, rank = truncated_ldlt_solve(J @ J.T, err)
    assert rank == 3 * n and np.count_nonzero(y) <= rank
    x = J.T @ y
    # closed form: per column of J (body b, axis r) the rows that hold it share one scale s; x = mean(err) / s
    for b in range(n):
        rows = [3 * i + r for i in np.nonzero(body1 == b)[0] for r in range(3)]
        for r in range(3):
            rr = [q for q in rows if q % 3 == r]
            s = J[rr[0], 6 * b + r]
            assert x[6 * b + r] == err[rr].mean() / s
            assert np.count_nonzero(y[rr]) <= 1


@pytest.mark.parametrize("n,rows,rank", [(10, 138, 54), (9, 126, 48)])
def test_cairn_row_counts_of_the_world_level_test(n, rows, rank):
    sc = scenes.cairn(n, seed=11)
    b0, b1, data = detect(sc["p"], sc["R"])
    sc = dict(sc, kind=np.ones(b0.shape[0], np.int32), body0=b0, body1=b1, data=data)
    J, A, err = system(sc)
    if n == 10:
        assert err.shape[0] > 126
    assert err.shape[0] == rows
    y, got = truncated_ldlt_solve(A, err)
    assert got == rank
    assert np.abs(J.T @ y - min_norm(J, err)).max() < 1e-12
