"""GPU (-m gpu): egs_box_lcp_schur_batch -- lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747) on many independent
problems, those of n <= 96 rows fused into one launch -- through the C ABI against the oracle's restatement
(oracle/lcp_toolkit.c::otk_box_schur) problem by problem: a ragged batch of 256 with both inner algorithms, each
problem alone and the batch twice (bit for bit), the single entry, the reference's own test submitted as one batch,
quirk Q6, sizes on both sides of the fused limit, the give-up limits and the refusals."""
import numpy as np
import pytest

from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
BIG = np.finfo(np.float64).max
FRACS = (0.0, 0.3, 0.5, 0.8, 1.0)


def spd(rng, n, ridge=0.0):
    A0 = rng.uniform(-1, 1, (n, n))
    return A0 @ A0.T + ridge * np.eye(n)


def marked(A):
    return np.tril(A) + np.triu(np.full(A.shape, 555.0), 1)     # the upper triangle must be neither read nor written


def problem(rng, n, frac):
    A = spd(rng, n, 0.05)
    b = rng.uniform(-1, 1, n)
    lo = np.full(n, -BIG); hi = np.full(n, BIG)
    pick = rng.uniform(size=n) < frac
    lo[pick] = -rng.uniform(0.01, 0.3, pick.sum()); hi[pick] = rng.uniform(0.01, 0.3, pick.sum())
    return A, b, lo, hi


def ragged(count=256, seed=7):
    rng = np.random.default_rng(seed)
    return [problem(rng, int(rng.integers(1, 97)), FRACS[k % len(FRACS)]) for k in range(count)]


def run_batch(ctx, probs, **kw):
    return ctx.box_lcp_schur_batch([marked(p[0]) for p in probs], [p[1] for p in probs], [p[2] for p in probs],
                                   [p[3] for p in probs], **kw)


def against_oracle(probs, res, tol=1e-9, require_ok=True, nubs=None, **okw):
    """Every problem of a batch result against orc.tk_box_schur; returns the largest |x - x_o|, |w - w_o| met."""
    ok, x, w, Ap, perm, nub, piv = res
    worst = 0.0
    for k, (A, b, lo, hi) in enumerate(probs):
        kw = dict(okw)
        if nubs is not None:
            kw["nub"] = int(nubs[k])
        oko, xo, wo, Ao, permo, nubo, ito = orc.tk_box_schur(np.tril(A), b, lo, hi, **kw)
        if require_ok:
            assert oko, "the oracle itself does not solve problem %d" % k
        assert ok[k] == oko and nub[k] == nubo and np.array_equal(perm[k], permo), k
        assert np.array_equal(np.triu(Ap[k], 1), np.triu(marked(A), 1)), k          # the sentinel is intact
        if oko:
            assert piv[k] == ito, k
            assert np.array_equal(np.tril(Ap[k]), np.tril(Ao)), k                    # the permuted lower triangle, bit for bit
            d = max(np.abs(x[k] - xo).max(), np.abs(w[k] - wo).max())
            worst = max(worst, d)
            assert d < tol, (k, d)
    return worst


@pytest.fixture(scope="module")
def batch():
    return ragged()


@pytest.fixture(scope="module")
def batch_results(ctx, batch):
    return {alg: run_batch(ctx, batch, algorithm=alg) for alg in (0, 1)}


@pytest.mark.parametrize("alg", [0, 1])
def test_ragged_batch(batch, batch_results, alg):
    res = batch_results[alg]
    assert all(res[0])
    worst = against_oracle(batch, res, algorithm=alg)
    nubs = np.array(res[5]); ns = np.array([len(p[1]) for p in batch])
    print("ragged batch, algorithm %d: max |x - x_oracle|, |w - w_oracle| = %.3e; nub = 0: %d, nub = n: %d, most inner steps %d"
          % (alg, worst, (nubs == 0).sum(), (nubs == ns).sum(), max(res[6])))
    assert (nubs == 0).sum() > 0 and (nubs == ns).sum() > 0 and ((nubs > 0) & (nubs < ns)).sum() > 0


@pytest.mark.parametrize("alg", [0, 1])
def test_each_problem_alone_and_the_batch_again(ctx, batch, batch_results, alg):
    ok, x, w, Ap, perm, nub, piv = batch_results[alg]
    for k, p in enumerate(batch):
        o1, x1, w1, A1, p1, n1, v1 = run_batch(ctx, [p], algorithm=alg)
        assert o1[0] == ok[k] and n1[0] == nub[k] and v1[0] == piv[k], k
        assert np.array_equal(x1[0], x[k]) and np.array_equal(w1[0], w[k]) and np.array_equal(A1[0], Ap[k]) and np.array_equal(p1[0], perm[k]), k
    again = run_batch(ctx, batch, algorithm=alg)                 # no state survives a call
    assert again[0] == ok and again[5] == nub and again[6] == piv
    for a, r in zip(again[1:5], (x, w, Ap, perm)):
        assert all(np.array_equal(u, v) for u, v in zip(a, r))


@pytest.mark.parametrize("alg", [0, 1])
def test_against_the_single_entry(ctx, batch, batch_results, alg):
    ok, x, w, Ap, perm, nub, piv = batch_results[alg]
    for k in range(0, 256, 16):
        A, b, lo, hi = batch[k]
        s = ctx.box_lcp_schur(marked(A), b, lo, hi, algorithm=alg)
        assert s[0] == ok[k] and s[5] == nub[k] and np.array_equal(s[4], perm[k]), k
        assert np.array_equal(np.tril(s[3]), np.tril(Ap[k])), k
        assert np.abs(s[1] - x[k]).max() < 1e-9 and np.abs(s[2] - w[k]).max() < 1e-9, k


def test_reference_test_restated_as_one_batch(ctx):      # toolkit/lcp.cc:1084-1200
    rng = np.random.default_rng(21)
    n = 20
    A = spd(rng, n)
    b = rng.uniform(-1, 1, n)
    x_full = np.linalg.solve(A, b)
    probs, nubs, want_nub = [], [], []
    free_lo = np.full(n, -BIG); free_hi = np.full(n, BIG)
    for hook in (n, n // 2):                  # :1102-1144
        probs.append((A, b, free_lo, free_hi)); nubs.append(hook); want_nub.append(hook)
    for start, end in ((0, n), (n // 4, n // 4 + n // 2)):      # :1146-1173
        lo = free_lo.copy(); hi = free_hi.copy()
        lo[start:end] = -rng.uniform(0, 1, end - start) * 10.0
        hi[start:end] = rng.uniform(0, 1, end - start) * 10.0
        probs.append((A, b, lo, hi)); nubs.append(-1); want_nub.append(n - (end - start))
    for _ in range(100):                     # :1176-1199
        lo = free_lo.copy(); hi = free_hi.copy()
        pick = rng.integers(0, 2, n) == 1
        lo[pick] = -rng.uniform(0, 1, pick.sum()) * 10.0
        hi[pick] = rng.uniform(0, 1, pick.sum()) * 10.0
        probs.append((A, b, lo, hi)); nubs.append(-1); want_nub.append(n - pick.sum())
    res = run_batch(ctx, probs, nubs=nubs)
    against_oracle(probs, res, nubs=nubs)
    ok, x, w, Ap, perm, nub, piv = res
    assert all(ok) and list(nub) == [int(v) for v in want_nub]
    for k in (0, 1):
        assert np.linalg.norm(x[k] - x_full) < 1e-6 and np.all(w[k] == 0)
    for k in range(2, len(probs)):
        lo, hi = probs[k][2], probs[k][3]
        assert np.linalg.norm(A @ x[k] - b - w[k]) < 1e-6 and np.all(x[k] >= lo) and np.all(x[k] <= hi)


def test_quirk_q6_and_its_correction(ctx):
    rng = np.random.default_rng(33)
    n = 8
    A = spd(rng, n, 0.1)
    b = rng.uniform(0.5, 1, n) * 5
    lo = np.full(n, -BIG); hi = np.full(n, BIG)
    lo[:4] = -1.0; hi[:4] = 1.0
    hi[6] = 0.01                              # lo = -infinity with a finite hi
    probs = [(A, b, lo, hi)] * 3
    r = run_batch(ctx, probs, reference_quirks=True)
    against_oracle(probs, r, q6=True)
    assert all(r[0]) and r[5] == [4, 4, 4]    # toolkit/lcp.cc:664, 669: the lower bound alone decides
    r = run_batch(ctx, probs, reference_quirks=False)
    against_oracle(probs, r, q6=False)
    assert all(r[0]) and r[5] == [3, 3, 3] and all(x[6] <= 0.01 + 1e-15 for x in r[1])


@pytest.mark.parametrize("alg", [0, 1])
def test_mixed_sizes(ctx, alg):               # 97, 130 and 300 rows take the route that is not fused
    rng = np.random.default_rng(2000 + alg)
    probs = [problem(rng, n, 0.5) for n in (5, 96, 97, 130, 300)]
    res = run_batch(ctx, probs, algorithm=alg)
    assert all(res[0])
    worst = against_oracle(probs, res, tol=1e-8, algorithm=alg)
    print("mixed sizes, algorithm %d: max difference %.3e" % (alg, worst))
    for (A, b, lo, hi), x, w in zip(probs, res[1], res[2]):
        assert np.linalg.norm(A @ x - b - w) < 1e-6 and np.all(x >= lo) and np.all(x <= hi)


def test_limits(ctx):
    probs = ragged(40, seed=11)
    res = run_batch(ctx, probs, max_iterations=1)               # Settings::max_iterations, applied to each problem
    want = [orc.tk_box_schur(np.tril(A), b, lo, hi, max_iterations=1)[0] for A, b, lo, hi in probs]
    assert res[0] == want
    assert any(want) and not all(want)
    for k, (A, b, lo, hi) in enumerate(probs):
        if res[5][k] == len(b):
            assert res[0][k]                                    # nothing to iterate on
    # Z not positive definite in one problem fails that problem alone
    rng = np.random.default_rng(44)
    n = 40
    A = spd(rng, n, 0.05); b = rng.uniform(-1, 1, n)
    lo = np.full(n, -0.05); hi = np.full(n, 0.05)
    lo[::3] = -BIG; hi[::3] = BIG
    Abad = A.copy(); Abad[0, 0] = -1.0
    three = [(A, b, lo, hi), (Abad, b, lo, hi), (A, b, lo, hi)]
    res = run_batch(ctx, three)
    assert res[0] == [True, False, True]
    against_oracle(three, res, require_ok=False)


def test_refusals_write_nothing(ctx):
    rng = np.random.default_rng(45)
    probs = [problem(rng, n, 0.5) for n in (12, 30, 7)]
    ns, A, b, lo, hi = capi.pack_lcp_batch([marked(p[0]) for p in probs], *[[p[i] for p in probs] for i in (1, 2, 3)])

    def refused(ns, A, b, lo, hi, nubs=None):
        lib = capi.load()
        import ctypes as C
        A2 = A.copy()
        tot = int(np.sum(ns))
        x = np.full(tot, 7.0); w = np.full(tot, 7.0); perm = np.full(tot, 7, np.int32)
        ok = np.full(len(ns), 7, np.int32); nub = np.full(len(ns), 7, np.int32); piv = np.full(len(ns), 7, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        st = lib.egs_box_lcp_schur_batch(ctx.h, C.c_int32(0), C.c_int32(len(ns)), p(ns), p(A2), p(b), p(lo), p(hi), p(nubs), C.c_int32(1),
                                         C.c_int32(0), C.c_double(0.0), p(x), p(w), p(perm), p(ok), p(nub), p(piv))
        assert st == capi.ERR_INVALID
        assert np.array_equal(A2, A) and np.all(x == 7.0) and np.all(w == 7.0) and np.all(perm == 7)
        assert np.all(ok == 7) and np.all(nub == 7) and np.all(piv == 7)

    refused(ns, A, b, lo, hi, nubs=np.array([-1, 31, -1], np.int32))              # nub[k] > n[k]
    refused(np.array([12, 0, 7], np.int32), A, b, lo, hi)                          # n = 0
    bad_lo = lo.copy()
    k = 12 + int(np.argmax(lo[12:42] > -1))                                        # a bounded row of the second problem
    bad_lo[k] = 0.5
    refused(ns, A, b, bad_lo, hi)
    with pytest.raises(capi.EgsError) as e:
        ctx.box_lcp_schur_batch([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], [p[3] for p in probs], nubs=[0, 31, 0])
    assert e.value.status == capi.ERR_INVALID
    # count = 0 is fine
    r = ctx.box_lcp_schur_batch([], [], [], [])
    assert r[0] == [] and r[1] == []
