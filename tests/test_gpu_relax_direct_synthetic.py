"""GPU (-m gpu): the direct relaxation solve (stabilize_direct.hip) on synthetic systems in each of its three size
classes -- one wavefront (<= 48 rows), four wavefronts in LDS (<= 126 rows), eight wavefronts on a global workspace
(<= 1024 rows) -- at both sides of each boundary and at the largest size accepted.  Random block systems (rank
deficient, inconsistent err, exact duplicates, both-anchored constraints) against the minimum-norm solution of
J x = err from numpy's SVD-based lstsq on J itself; diagonal and tied-pair systems on which every operation is exact,
bit for bit against the closed form and the numpy restatement; rank 0; one system through all three kernels; and at
world level two cairns with an inconsistent err at the LDS limit and above it.
tests/test_relax_direct_reference_cpu.py proves on the CPU that each case has a wide rank gap, is well conditioned
and that the reference holds to 1e-13."""
import numpy as np
import pytest

from eggshell_amd import scenes
from relax_direct_cases import (CASES, DIAG_ROWS, DIAG_TOL, SEED, TIED_BODIES, block_system, case_id,
                                diag_closed_form, diag_scales, diag_system, min_norm, tied_pair_system)
from test_gpu_world_dense import make_world
from test_gpu_world_stabilize import loose_ensemble, state
from test_gpu_world_stabilize_direct import INIT, numpy_pass
from test_world_stabilize_direct_cpu import truncated_ldlt_solve

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_block_system_against_the_minimum_norm_solution(ctx, case):
    """Bound 1e-12: the one the project holds this kernel to against lstsq.  The solutions are O(1), the numpy
    restatement is within 2e-14 of the reference on every case, and the device differs from the restatement by FMA
    contraction and summation order only."""
    m, n, dup, both, consistent = case
    body0, body1, J0, J1, err, J = block_system(m, n, SEED, dup=dup, both_anchored=both, consistent=consistent)
    _, want_rank = truncated_ldlt_solve(J @ J.T, err)
    want = min_norm(J, err)
    y, rank = ctx.relax_blocks_direct(n, body0, body1, J0, J1, err)
    d = np.abs(J.T @ y - want).max()
    print("block system %s: rows %d rank %d  max |J^T y - min_norm| %.3e  (max |min_norm| %.2f)"
          % (case_id(case), 3 * m, rank, d, np.abs(want).max()))
    assert y.shape == (3 * m,) and np.all(np.isfinite(y))
    assert rank == want_rank
    assert np.count_nonzero(y) <= rank
    zero_rows = np.repeat((body0 < 0) & (body1 < 0), 3)
    assert np.count_nonzero(zero_rows) == 3 * both
    assert not y[zero_rows].any()
    assert d < 1e-12


@pytest.mark.parametrize("rows", DIAG_ROWS)
def test_diagonal_system_bit_for_bit(ctx, rows):
    """J J^T = diag(powers of four) in a shuffled order: swaps at nearly every step, ties, a pivot exactly at
    rank_tol * first (truncated) and one at the next power above (kept); err is non-zero on the truncated rows, so the
    completion runs with h = 0 and G = I.  Every operation is exact: y and rank are the closed form's."""
    scales, err = diag_scales(rows)
    body0, body1, J0, J1, _ = diag_system(scales)
    want, want_rank = diag_closed_form(scales, err, DIAG_TOL)
    y, rank = ctx.relax_blocks_direct(rows // 3, body0, body1, J0, J1, err, rank_tol=DIAG_TOL)
    print("diagonal %d rows: rank %d of %d, %d rows differ" % (rows, rank, rows, np.count_nonzero(y != want)))
    assert rank == want_rank < rows
    assert y.tobytes() == want.tobytes()
    full, full_rank = diag_closed_form(scales, err, 1e-10)
    y, rank = ctx.relax_blocks_direct(rows // 3, body0, body1, J0, J1, err)      # the default rank_tol keeps them
    assert rank == full_rank == rows
    assert y.tobytes() == full.tobytes()


@pytest.mark.parametrize("n", TIED_BODIES)
def test_tied_pairs_bit_for_bit(ctx, n):
    """Pairs of exactly equal rows with integer err on power-of-two diagonals: the lowest-index rule decides which row
    of a pair is kept, the other becomes an exact zero pivot, and the completion (G = diag(1 or 2)) averages err over
    the pair.  Every operation is exact, so y equals the numpy restatement's bit for bit; another pivot order, or a
    scatter through a wrong perm, moves the non-zeros."""
    n, body0, body1, J0, J1, err, J = tied_pair_system(n)
    want, want_rank = truncated_ldlt_solve(J @ J.T, err)
    y, rank = ctx.relax_blocks_direct(n, body0, body1, J0, J1, err)
    print("tied pairs %d rows: rank %d, %d rows differ" % (err.shape[0], rank, np.count_nonzero(y != want)))
    assert rank == want_rank == 3 * n
    assert y.tobytes() == want.tobytes()


@pytest.mark.parametrize("m", [1, 43])
def test_rank_zero(ctx, m):
    rng = np.random.default_rng(SEED + m)
    body0 = np.zeros(m, np.int32)
    body1 = np.ones(m, np.int32)
    body0[::3] = -1
    y, rank = ctx.relax_blocks_direct(2, body0, body1, np.zeros((m, 18)), np.zeros((m, 18)), rng.standard_normal(3 * m))
    assert rank == 0
    assert not np.isnan(y).any()
    assert y.shape == (3 * m,) and not y.any()


def test_one_system_through_all_three_kernels(ctx):
    """The 48-row, rank-18 case alone (one wavefront), then as the first 16 constraints of 17 (LDS class) and of 43
    (global class), the added constraints anchored on both sides: zero rows that no pivot order can prefer."""
    m, n, dup, both, consistent = CASES[2]
    body0, body1, J0, J1, err, J = block_system(m, n, SEED, dup=dup, both_anchored=both, consistent=consistent)
    assert 3 * m == 48
    y48, rank48 = ctx.relax_blocks_direct(n, body0, body1, J0, J1, err)
    x48 = J.T @ y48
    assert rank48 == 18 and np.abs(x48 - min_norm(J, err)).max() < 1e-12
    rng = np.random.default_rng(SEED)
    for total in (17, 43):
        k = total - m
        pad = lambda a, fill: np.concatenate([a, np.full((k,) + a.shape[1:], fill, a.dtype)])
        e2 = np.concatenate([err, rng.standard_normal(3 * k)])
        y, rank = ctx.relax_blocks_direct(n, pad(body0, -1), pad(body1, -1), pad(J0, 0.0), pad(J1, 0.0), e2)
        d = np.abs(J.T @ y[:48] - x48).max()
        print("48 rows inside %d: rank %d  max |J^T y - the 48-row J^T y| %.3e" % (3 * total, rank, d))
        assert rank == rank48
        assert not y[48:].any()
        assert d < 1e-12


def cairn(n, origin=(0.0, 0.0)):
    return loose_ensemble(scenes.cairn(n, seed=11, origin=origin))


@pytest.mark.parametrize("n", [10, 9])
def test_cairn_with_an_inconsistent_err_one_pass(ctx, n):
    """cairn(10): 138 rows, the global-workspace class with a completion that matters; cairn(9): exactly 126 rows, the
    largest ensemble held in LDS.  The reference is the numpy pass of tests/test_gpu_world_stabilize_direct.py on the
    contacts detected at the start; its bound 1e-12 is that file's."""
    e = cairn(n)
    w, _ = make_world(ctx, [e])
    try:
        ref, err, corr = numpy_pass(ctx, e["p"], e["R"])
        w.stabilize_direct(INIT, max_steps=1)
        info, rk = w.stabilize_info(), w.stabilize_rank()
        pos, R, v, wv = w.bodies()
        dp, dR = np.abs(pos - ref["p"]).max(), np.abs(R - ref["R"]).max()
        print("cairn(%d): rows solved %d, after the move %d, rank %d  max |dp| %.3e  max |dR| %.3e  correction %.3e"
              % (n, err.shape[0], rk["rows"][0], rk["rank"][0], dp, dR, np.abs(0.5 * corr).max()))
        assert info["steps"][0] == 1
        # the pass solved the list detected at the start (err's); rows reports the list detected after the move
        if n == 10:
            assert err.shape[0] > 126 and rk["rows"][0] > 126
        else:
            assert err.shape[0] == 126
        assert 0 < rk["rank"][0] < err.shape[0]
        assert 0 < rk["rank"][0] < rk["rows"][0]
        assert dp < 1e-12 and dR < 1e-12
        assert np.array_equal(v, e["v"]) and np.array_equal(wv, e["w"])
    finally:
        w.close()


def test_cairn_batch_matches_worlds_of_one(ctx):
    ens = [cairn(10), cairn(9, origin=(3.0, 0.0)), cairn(5, origin=(0.0, 3.0))]
    bw, boff = make_world(ctx, ens)
    singles = [make_world(ctx, [e]) for e in ens]
    try:
        bw.stabilize_direct(INIT, max_steps=1)
        binfo, brk = bw.stabilize_info(), bw.stabilize_rank()
        print("cairn batch: rows %s rank %s" % (brk["rows"], brk["rank"]))
        assert brk["rows"][0] > 126 and 48 < brk["rows"][2] <= 126
        for e, (sw, soff) in enumerate(singles):
            sw.stabilize_direct(INIT, max_steps=1)
            sinfo, srk = sw.stabilize_info(), sw.stabilize_rank()
            assert binfo["steps"][e] == sinfo["steps"][0] == 1, e
            assert binfo["err_sq"][e].tobytes() == sinfo["err_sq"][0].tobytes(), e
            assert brk["rows"][e] == srk["rows"][0] and brk["rank"][e] == srk["rank"][0], e
            assert 0 < brk["rank"][e] < brk["rows"][e], e
            for a, b in zip(state(bw, boff, e), state(sw, soff, 0)):
                assert a.tobytes() == b.tobytes(), e
            assert not np.array_equal(state(bw, boff, e)[0], ens[e]["p"]), e      # the pass moved it
    finally:
        bw.close()
        for sw, _ in singles:
            sw.close()
