"""GPU (-m gpu): the fused batch entries on the batches [1] and [3, 1, 2], the sizes at which the sections of their packed
block (csrc/packed_block.h) meet their padding: an odd number of matrix entries leaves the next section 8 mod 16, and a
single row leaves the int32 sections 4 mod 8.  Every problem of a batch against the single-problem entry on it, bit for
bit.

The direct solvers' single entries factor with other kernels than the fused ones, so the matrices here are F F^T with
small integer F whose diagonal is a power of two, the equality resp. unbounded rows in front: every factor, solve and
Schur complement is then exact in binary64 whatever the order of the sums, and the bits must agree.  The pyramid form
has no single-problem entry in the C ABI: a problem with a pyramid row is compared with the batch that holds it alone,
the one without with the plain single entry."""
import numpy as np
import pytest

from eggshell_amd import capi

pytestmark = pytest.mark.gpu
BIG = np.finfo(np.float64).max
F3 = np.array([[2.0, 0, 0], [2, 1, 0], [-2, 2, 4]])
F2 = np.array([[1.0, 0], [3, 2]])
F1 = np.array([[2.0]])
FACTORS = {1: F1, 2: F2, 3: F3}
BATCHES = ([1], [3, 1, 2])


def exact_problem(n, salt):
    """A = F F^T, b small integers; the rows before the last are equality / unbounded rows, the last one is a box row."""
    A = FACTORS[n] @ FACTORS[n].T
    b = np.array([4.0, -2.0, 8.0][:n]) * (1 + salt)
    Ceq = np.array([1] * (n - 1) + [0], np.uint8)
    lo = np.array([-BIG] * (n - 1) + [-0.25])
    hi = np.array([BIG] * (n - 1) + [0.5])
    return A, b, Ceq, lo, hi


@pytest.mark.parametrize("sizes", BATCHES, ids=str)
@pytest.mark.parametrize("use_bounds", [0, 1])
def test_mixed_constraints_batch_against_the_single_entry(ctx, sizes, use_bounds):
    probs = [exact_problem(n, k) for k, n in enumerate(sizes)]
    if not use_bounds:
        probs = [(A, b, Ceq, np.zeros(len(b)), np.full(len(b), np.inf)) for A, b, Ceq, lo, hi in probs]
    oks, xs, ws, pivs = ctx.mixed_constraints_solve_batch(*[list(c) for c in zip(*probs)], use_bounds=use_bounds)
    for k, p in enumerate(probs):
        ok, x, w, piv = ctx.mixed_constraints_solve(*p, use_bounds=use_bounds)
        assert ok and oks[k] and piv == pivs[k], (k, ok, oks[k], piv, pivs[k])
        assert np.array_equal(x, xs[k]) and np.array_equal(w, ws[k]), (k, x, xs[k], w, ws[k])
        assert np.abs(p[0] @ x - p[1] - w).max() == 0.0, k


def friction_pack(probs):
    ns = np.array([len(p[1]) for p in probs], np.int32)
    cat = lambda i, dt=np.float64: np.concatenate([np.asarray(p[i], dt).ravel() for p in probs])
    return dict(ns=ns, A=cat(0), b=cat(1), C=cat(2, np.uint8), lo=cat(3), hi=cat(4), normal_row=cat(5, np.int32), mu=cat(6))


@pytest.mark.parametrize("sizes", BATCHES, ids=str)
def test_mixed_friction_batch_against_the_problems_alone(ctx, sizes):
    probs = []
    for k, n in enumerate(sizes):
        A, b, Ceq, lo, hi = exact_problem(n, k)
        nrow, mu = np.full(n, -1, np.int32), np.zeros(n)
        if n == 3:     # the one problem with a pyramid row: row 0 follows the normal row 2
            Ceq = np.zeros(3, np.uint8); lo = np.array([0.0, -BIG, 0.0]); hi = np.array([0.0, BIG, BIG])
            b = np.array([1.0, -2.0, 8.0])
            nrow[0] = 2; mu[0] = 0.5
        probs.append((A, b, Ceq, lo, hi, nrow, mu))
    got = ctx.mixed_friction_solve_batch_packed(**friction_pack(probs))
    assert got["ok"].all()
    offs = np.concatenate([[0], np.cumsum([len(p[1]) for p in probs])])
    for k, p in enumerate(probs):
        rows = slice(offs[k], offs[k + 1])
        one = ctx.mixed_friction_solve_batch_packed(**friction_pack([p]))
        for key in ("x", "w", "beta"):
            assert np.array_equal(one[key], got[key][rows]), (k, key, one[key], got[key][rows])
        for key in ("ok", "pivots", "outer", "change"):
            assert one[key][0] == got[key][k], (k, key)
        if (p[5] >= 0).any():
            assert got["beta"][rows][0] > 0.0 and abs(got["x"][rows][0]) <= got["beta"][rows][0] and not got["beta"][rows][1:].any()
        else:          # no pyramid row: the plain single entry under use_bounds = 1
            ok, x, w, piv = ctx.mixed_constraints_solve(*p[:5], use_bounds=1)
            assert ok and np.array_equal(x, got["x"][rows]) and np.array_equal(w, got["w"][rows]), (k, x, got["x"][rows])
            assert not got["beta"][rows].any()


@pytest.mark.parametrize("sizes", BATCHES, ids=str)
@pytest.mark.parametrize("alg", [0, 1])
def test_box_schur_batch_against_the_single_entry(ctx, sizes, alg):
    probs = [exact_problem(n, k) for k, n in enumerate(sizes)]
    As = [np.tril(p[0]) + np.triu(np.full(p[0].shape, 555.0), 1) for p in probs]     # the upper triangle is never touched
    ok, x, w, Ap, perm, nub, piv = ctx.box_lcp_schur_batch(As, [p[1] for p in probs], [p[3] for p in probs], [p[4] for p in probs],
                                                           algorithm=alg)
    for k, p in enumerate(probs):
        s = ctx.box_lcp_schur(As[k], p[1], p[3], p[4], algorithm=alg)
        assert s[0] and ok[k] and s[5] == nub[k] == len(p[1]) - 1, (k, s[0], ok[k], s[5], nub[k])
        assert np.array_equal(s[4], perm[k]) and np.array_equal(s[3], Ap[k]), k
        assert np.array_equal(s[1], x[k]) and np.array_equal(s[2], w[k]), (k, s[1], x[k], s[2], w[k])


@pytest.mark.parametrize("sizes", BATCHES, ids=str)
@pytest.mark.parametrize("history", [False, True])
def test_dense_iterate_batch_against_the_single_entry(ctx, sizes, history):
    rng = np.random.default_rng(11)
    probs = []
    for n in sizes:
        A = rng.uniform(-1, 1, (n, n)) + 4.0 * np.eye(n)
        probs.append((A, rng.uniform(-1, 1, n), rng.integers(0, 2, n).astype(np.uint8), np.full(n, -0.2), np.full(n, 0.3)))
    for method in (capi.JACOBI, capi.GAUSS_SEIDEL, capi.SOR):
        prm = capi.params(method=method, max_iters=12, tol=1e-12)
        out = ctx.dense_iterate_batch(*[list(c) for c in zip(*probs)][:2], prm, *[list(c) for c in zip(*probs)][2:], history=history)
        for k, p in enumerate(probs):
            x, st = ctx.dense_iterate(p[0], p[1], prm, p[2], p[3], p[4])
            assert st.iterations == out[1][k] and st.residual == out[2][k] and np.array_equal(x, out[0][k]), (k, method)
            if history:
                h = out[3][k]
                assert h.shape == (13,) and h[st.iterations] == st.residual and np.isnan(h[st.iterations + 1:]).all(), (k, method)
