"""GPU (-m gpu): lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747) on the device through the C ABI
(egs_box_lcp_schur) against the oracle's restatement (oracle/lcp_toolkit.c::otk_box_schur, itself held against the
reference's own test in tests/test_oracle_lcp_toolkit.py): the reference's test restated (n = 20, lower triangle
only, nub hook n and n / 2, full box problems, 100 random partitions), x / w and the permuted matrix compared, both
inner algorithms, quirk Q6, sizes whose bounded part needs the in-memory instantiation, and the give-up limits."""
import numpy as np
import pytest

from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
BIG = np.finfo(np.float64).max


def spd(rng, n, ridge=0.0):
    A0 = rng.uniform(-1, 1, (n, n))
    return A0 @ A0.T + ridge * np.eye(n)


def marked(A):
    return np.tril(A) + np.triu(np.full(A.shape, 555.0), 1)     # the upper triangle must be neither read nor written


def same_as_oracle(ctx, A, b, lo, hi, tol=1e-9, **kw):
    r = ctx.box_lcp_schur(marked(A), b, lo, hi, **kw)
    okw = dict(kw); okw["q6"] = okw.pop("reference_quirks", True)
    okw.pop("max_seconds", None)
    if okw.get("max_iterations", 0) == 0:
        okw.pop("max_iterations", None)
    o = orc.tk_box_schur(np.tril(A), b, lo, hi, **okw)
    ok, x, w, Ap, perm, nub, piv = r
    oko, xo, wo, Ao, permo, nubo, ito = o
    assert ok == oko and nub == nubo and np.array_equal(perm, permo)
    assert np.array_equal(np.triu(Ap, 1), np.triu(marked(A), 1))
    if ok:
        assert np.abs(x - xo).max() < tol and np.abs(w - wo).max() < tol
        assert np.array_equal(np.tril(Ap), np.tril(Ao))          # the permuted lower triangle, bit for bit
        if 0 < nub:
            assert np.array_equal(np.tril(Ap), np.tril(A[np.ix_(perm, perm)]))
    return r


def test_reference_test_restated(ctx):      # toolkit/lcp.cc:1084-1200
    rng = np.random.default_rng(21)
    n = 20
    A = spd(rng, n)
    b = rng.uniform(-1, 1, n)
    x_full = np.linalg.solve(A, b)
    lo = np.full(n, -BIG); hi = np.full(n, BIG)
    for nub in (n, n // 2):                  # :1102-1144
        ok, x, w, Ap, perm, nub_out, piv = same_as_oracle(ctx, A, b, lo, hi, nub=nub)
        assert ok and nub_out == nub and np.linalg.norm(x - x_full) < 1e-6 and np.all(w == 0)
    for start, end in ((0, n), (n // 4, n // 4 + n // 2)):      # :1146-1173
        lo = np.full(n, -BIG); hi = np.full(n, BIG)
        lo[start:end] = -rng.uniform(0, 1, end - start) * 10.0
        hi[start:end] = rng.uniform(0, 1, end - start) * 10.0
        ok, x, w, Ap, perm, nub_out, piv = same_as_oracle(ctx, A, b, lo, hi)
        assert ok and np.linalg.norm(A @ x - b - w) < 1e-6 and np.all(x >= lo) and np.all(x <= hi)
        assert nub_out == n - (end - start)
    for _ in range(100):                     # :1176-1199
        lo = np.full(n, -BIG); hi = np.full(n, BIG)
        pick = rng.integers(0, 2, n) == 1
        lo[pick] = -rng.uniform(0, 1, pick.sum()) * 10.0
        hi[pick] = rng.uniform(0, 1, pick.sum()) * 10.0
        ok, x, w, Ap, perm, nub_out, piv = same_as_oracle(ctx, A, b, lo, hi)
        assert ok and np.linalg.norm(A @ x - b - w) < 1e-6 and np.all(x >= lo) and np.all(x <= hi)
        assert nub_out == n - pick.sum()


@pytest.mark.parametrize("n,frac,alg", [(5, 0.5, 0), (64, 0.5, 1), (130, 0.4, 0), (300, 0.5, 0), (300, 0.6, 1), (500, 0.3, 0)])
def test_sizes_and_both_inner_algorithms(ctx, n, frac, alg):
    rng = np.random.default_rng(1000 + n + alg)
    A = spd(rng, n, 0.05)
    b = rng.uniform(-1, 1, n)
    lo = np.full(n, -np.inf); hi = np.full(n, np.inf)
    pick = rng.uniform(size=n) < frac
    lo[pick] = -rng.uniform(0.01, 0.3, pick.sum()); hi[pick] = rng.uniform(0.01, 0.3, pick.sum())
    ok, x, w, Ap, perm, nub, piv = same_as_oracle(ctx, A, b, lo, hi, algorithm=alg, tol=1e-8)
    assert ok and nub == n - pick.sum()
    assert np.linalg.norm(A @ x - b - w) < 1e-6
    inside = pick & (x > lo) & (x < hi)
    assert np.abs(w[inside]).max(initial=0) == 0 and np.all(w[~pick] == 0)
    assert np.all(w[pick & (x == lo)] >= 0) and np.all(w[pick & (x == hi)] <= 0)


def test_quirk_q6_and_its_correction(ctx):
    rng = np.random.default_rng(33)
    n = 8
    A = spd(rng, n, 0.1)
    b = rng.uniform(0.5, 1, n) * 5
    lo = np.full(n, -BIG); hi = np.full(n, BIG)
    lo[:4] = -1.0; hi[:4] = 1.0
    hi[6] = 0.01                              # lo = -infinity with a finite hi
    r = same_as_oracle(ctx, A, b, lo, hi, reference_quirks=True)
    assert r[0] and r[5] == 4                 # toolkit/lcp.cc:664, 669: the lower bound alone decides
    r = same_as_oracle(ctx, A, b, lo, hi, reference_quirks=False)
    assert r[0] and r[5] == 3 and r[1][6] <= 0.01 + 1e-15


def test_limits_and_refusals(ctx):
    rng = np.random.default_rng(44)
    n = 40
    A = spd(rng, n, 0.05); b = rng.uniform(-1, 1, n)
    lo = np.full(n, -0.05); hi = np.full(n, 0.05)
    lo[::3] = -BIG; hi[::3] = BIG
    full = ctx.box_lcp_schur(np.tril(A), b, lo, hi)
    assert full[0] and full[6] > 1
    capped = ctx.box_lcp_schur(np.tril(A), b, lo, hi, max_iterations=1)          # Settings::max_iterations (toolkit/lcp.cc:391)
    assert not capped[0]
    with pytest.raises(capi.EgsError) as e:
        ctx.box_lcp_schur(np.tril(A), b, lo, hi, nub=n + 1)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.EgsError) as e:                                       # lo <= 0 <= hi on the bounded rows
        ctx.box_lcp_schur(np.tril(A), b, np.where(lo > -1, 0.5, lo), np.where(hi < 1, 1.0, hi))
    assert e.value.status == capi.ERR_INVALID
    Abad = A.copy(); Abad[0, 0] = -1.0        # Z not positive definite
    assert not ctx.box_lcp_schur(np.tril(Abad), b, lo, hi)[0]


@pytest.mark.parametrize("n,unbounded", [(1100, 0.0), (1200, 0.05)])
def test_block_rule_beyond_the_incremental_solver(ctx, n, unbounded):
    """More bounded rows than the incremental-factor solver takes (1 024): the box LCP goes to the pivot loop with the
    block rule, on the matrix itself when every row is bounded (n = 1 100) and on the Schur complement otherwise
    (n = 1 200, 62 unbounded and 1 138 bounded rows).  The recipe of
    test_gpu_dense_block.py::test_block_rule_between_the_round_sizes and its flat tolerances.  Seed n + 1: in float64 on
    the host (tests/lcp_reference.py: find_set) both problems are solvable and no bounded row has |x - bound| and |w|
    below 1.5e-4; seed n = 1 100 has one at 8e-6."""
    rng = np.random.default_rng(n + 1)
    M = rng.uniform(-1, 1, (n, n))
    A = M.T @ M + 1e-2 * np.eye(n)
    b = rng.uniform(-1, 1, n) * 3.0
    lo = np.where(rng.uniform(size=n) < 0.5, -0.2, 0.0)
    hi = np.where(rng.uniform(size=n) < 0.5, 0.3, np.inf)
    free = rng.uniform(size=n) < unbounded
    lo[free] = -BIG; hi[free] = BIG
    ok, x, w, Ap, perm, nub, piv = ctx.box_lcp_schur(np.tril(A), b, lo, hi)
    assert ok
    assert nub == free.sum() and np.array_equal(np.sort(perm), np.arange(n))
    assert np.linalg.norm(A @ x - b - w) <= 1e-6 * max(1.0, np.linalg.norm(A @ x))
    assert not w[free].any()
    xi, wi, li, hi_i = x[~free], w[~free], lo[~free], hi[~free]
    tol = 1e-7
    assert (xi >= li - tol).all() and (xi <= hi_i + tol).all()
    inside = (xi > li + tol) & (xi < hi_i - tol)
    assert np.abs(wi[inside]).max(initial=0.0) < 1e-6
    assert (wi[np.abs(xi - li) <= tol] >= -1e-6).all() and (wi[np.abs(xi - hi_i) <= tol] <= 1e-6).all()
    # (flat and loose on purpose: the measured bounds in units of u are test_gpu_lcp_reference.py's)
