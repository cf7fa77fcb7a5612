"""GPU (-m gpu): egs_dense_iterate_batch -- sparse::{Jacobi,GaussSeidel,SOR}Iteration on an explicit matrix
(sparse_iterations.cc:72-144) for many systems in one device pipeline -- through the C ABI against the oracle's
restatement (oracle/dense_iter.c), problem by problem and bit for bit: sweep count, x, final residual and every entry of
the residual history, in both size classes (one wavefront with the matrix in LDS up to 96 rows, the single call's
workgroup beyond), in ragged batches in any order, with more workgroups than CUs, and the refusals."""
import numpy as np
import pytest

from eggshell_amd import capi
from oracle import oracle as orc
from test_oracle_dense_iter import check_mixed, diag_dominant, spd

pytestmark = pytest.mark.gpu
TOL = 1e-9
METHODS = (capi.JACOBI, capi.GAUSS_SEIDEL, capi.SOR)
RAGGED = [0, 1, 2, 3, 24, 24, 48, 63, 64, 65, 95, 96, 97, 128]


def recipe(seed, n):
    """R(seed, n): the systems of test_gpu_dense_iter.py::test_sizes_beyond_one_wavefront."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1, 1, (n, n))
    A = m.T @ m + (0.5 * n ** 0.5 + 1.0) * np.eye(n)
    b = rng.uniform(-1, 1, n)
    C = rng.integers(0, 2, n).astype(bool)
    return A, b, C, np.full(n, -0.05), np.full(n, 0.08)


def systems(sizes, seed0):
    return [recipe(seed0 + k, n) for k, n in enumerate(sizes)]


def oracle_all(probs, method, cap, mixed=True):
    return [orc.dense_iterate(A, b, method, *((C, lo, hi) if mixed else ()), max_iters=cap) for A, b, C, lo, hi in probs]


def run_batch(ctx, probs, method, cap, history=False, mixed=True):
    prm = capi.params(method=method, max_iters=cap, tol=TOL)
    cols = list(zip(*probs))
    extra = (list(cols[2]), list(cols[3]), list(cols[4])) if mixed else (None, None, None)
    return ctx.dense_iterate_batch(list(cols[0]), list(cols[1]), prm, *extra, history=history)


def assert_equal_to(got, want):
    """got: x, iterations, residual lists of the batch; want: per problem (x, iterations, residual)."""
    xs, its, res = got[:3]
    assert len(xs) == len(want)
    for k, (xo, ito, reso) in enumerate(want):
        assert its[k] == ito, (k, its[k], ito)
        assert np.array_equal(xs[k], xo), k
        assert res[k] == reso, (k, res[k], reso)


@pytest.fixture(scope="module")
def ragged():
    probs = systems(RAGGED, 1000)
    return probs, {m: oracle_all(probs, m, 60) for m in METHODS}


@pytest.mark.parametrize("method", METHODS)
def test_ragged_batch_both_classes(ctx, ragged, method):
    probs, want = ragged
    counts = [w[1] for w in want[method]]
    if method != capi.JACOBI:       # one batch covers "no sweep", "stops on the tolerance" and "hits the cap"
        assert 0 in counts and 60 in counts and any(0 < c < 60 for c in counts), counts
    assert_equal_to(run_batch(ctx, probs, method, 60), want[method])


@pytest.fixture(scope="module")
def large():
    probs = systems([200, 700, 1024], 2000)
    return probs, {m: oracle_all(probs, m, 12) for m in METHODS}


@pytest.mark.parametrize("method", METHODS)
def test_large_medium_class(ctx, large, method):
    probs, want = large
    assert [w[1] for w in want[method]] == [12, 12, 12]
    assert_equal_to(run_batch(ctx, probs, method, 12), want[method])


@pytest.mark.parametrize("method", METHODS)
def test_batch_equals_single(ctx, ragged, method):
    probs, _ = ragged
    xs, its, res = run_batch(ctx, probs, method, 60)
    prm = capi.params(method=method, max_iters=60, tol=TOL)
    for k, p in enumerate(probs):
        x1, it1, res1 = run_batch(ctx, [p], method, 60)                 # alone, as a batch of one
        assert it1[0] == its[k] and res1[0] == res[k] and np.array_equal(x1[0], xs[k]), k
        xs1, st = ctx.dense_iterate(p[0], p[1], prm, p[2], p[3], p[4])   # and through the single entry
        assert st.iterations == its[k] and st.residual == res[k] and np.array_equal(xs1, xs[k]), k
    xr, itr, resr = run_batch(ctx, probs[::-1], method, 60)
    assert itr == its[::-1] and resr == res[::-1]
    for a, c in zip(xr, xs[::-1]):
        assert np.array_equal(a, c)


def test_more_workgroups_than_cus(ctx):
    sizes = [200 if k % 50 == 0 else 24 for k in range(600)]
    probs = [recipe(7000 + k, n) for k, n in enumerate(sizes)]
    want = oracle_all(probs, capi.SOR, 40)
    assert min(w[1] for w in want) >= 37 and max(w[1] for w in want) == 40
    assert_equal_to(run_batch(ctx, probs, capi.SOR, 40), want)


@pytest.mark.parametrize("method", [capi.GAUSS_SEIDEL, capi.SOR])
def test_residual_history(ctx, ragged, method):
    probs, want = ragged
    pick = [k for k, n in enumerate(RAGGED) if n in (24, 48, 96, 128)]
    assert [RAGGED[k] for k in pick] == [24, 24, 48, 96, 128]
    sub = [probs[k] for k in pick]
    xs, its, res, hist = run_batch(ctx, sub, method, 60, history=True)
    assert_equal_to((xs, its, res), [want[method][k] for k in pick])
    for k, (A, b, C, lo, hi) in enumerate(sub):
        assert hist[k].shape == (61,)
        for s in range(its[k] + 1):
            xo, ito, reso = orc.dense_iterate(A, b, method, C, lo, hi, max_iters=s)
            assert ito == s and hist[k][s] == reso, (k, s, hist[k][s], reso)
        assert np.all(np.isnan(hist[k][its[k] + 1:]))
        assert hist[k][its[k]] == res[k]
    x2, it2, res2 = run_batch(ctx, sub, method, 60, history=False)
    assert it2 == its and res2 == res and all(np.array_equal(a, c) for a, c in zip(x2, xs))


def test_reference_tests_as_one_batch(ctx):
    """sparse_iterations.cc:355-513: ten instances, dimension 3..50, in the 2-argument and the mixed form."""
    rng = np.random.default_rng(13)
    inf = np.inf
    eq = {m: [] for m in METHODS}          # (A, b) per method, 2-argument form
    mixed = {capi.GAUSS_SEIDEL: [], capi.SOR: []}
    for inst in range(10):
        n = int(rng.integers(3, 51))
        b = rng.uniform(-1, 1, n)
        A = diag_dominant(rng, n)
        for m in METHODS:
            eq[m].append((A, b))
        eq[capi.GAUSS_SEIDEL].append((spd(rng, n, 1.0), b))
        eq[capi.SOR].append((spd(rng, n, 2.0), b))
        C = rng.integers(0, 2, n).astype(bool)
        S = spd(rng, n, 0.5)
        mixed[capi.GAUSS_SEIDEL].append((S, b, C, np.full(n, -inf), np.full(n, inf)))
        mixed[capi.GAUSS_SEIDEL].append((S, b, C, np.full(n, -0.5), np.full(n, 0.5)))
        mixed[capi.SOR].append((spd(rng, n, 2.0), b, C, np.full(n, -10.0), np.full(n, 10.0)))
    for m in METHODS:
        probs = [(A, b, None, None, None) for A, b in eq[m]]
        got = run_batch(ctx, probs, m, 500, mixed=False)
        assert_equal_to(got, oracle_all(probs, m, 500, mixed=False))
        for (A, b), x in zip(eq[m], got[0]):
            assert np.linalg.norm(A @ x - b) < TOL
    for m, probs in mixed.items():
        got = run_batch(ctx, probs, m, 500)
        assert_equal_to(got, oracle_all(probs, m, 500))
        for (A, b, C, lo, hi), x in zip(probs, got[0]):
            check_mixed(A, b, x, C, lo, hi)


def raw(ctx, ns, A, b, prm, x):
    """The C ABI itself, without the binding's own checks: the status."""
    import ctypes as ct
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    it = np.zeros(len(ns), np.int32); res = np.zeros(len(ns))
    p = lambda a: a.ctypes.data_as(ct.c_void_p)
    return capi.load().egs_dense_iterate_batch(ctx.h, ct.c_int32(len(ns)), p(ns), p(A), p(b), None, None, None, ct.byref(prm),
                                               p(x), p(it), p(res), None), it, res


def test_edges_and_refusals(ctx):
    import ctypes as ct
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=5)
    none = np.zeros(0)
    assert capi.load().egs_dense_iterate_batch(ctx.h, ct.c_int32(0), None, None, None, None, None, None, ct.byref(prm), None, None,
                                               None, None) == capi.OK
    x, it, res = ctx.dense_iterate_batch_packed([], none, none, prm)
    assert len(x) == 0 and len(it) == 0
    x, it, res, hist = ctx.dense_iterate_batch_packed([0, 0, 0], none, none, prm, history=True)       # nothing but empty problems
    assert list(it) == [0, 0, 0] and list(res) == [0.0, 0.0, 0.0]
    assert np.all(hist[:, 0] == 0.0) and np.all(np.isnan(hist[:, 1:]))
    # 1024 rows are accepted, 1025 anywhere are not
    A, b = np.eye(1024) * 2.0, np.ones(1024)
    xs, its, rs = ctx.dense_iterate_batch([np.eye(3), A], [np.ones(3), b], prm)
    xo, ito, reso = orc.dense_iterate(A, b, capi.GAUSS_SEIDEL, max_iters=5)
    assert its == [0, ito] and rs[1] == reso and np.array_equal(xs[1], xo)

    def refused(ns, A, b, prm):
        x = np.full(int(np.maximum(ns, 0).sum()) + 1, 777.0)
        st, it, res = raw(ctx, ns, np.ascontiguousarray(A, dtype=float), np.ascontiguousarray(b, dtype=float), prm, x)
        assert st == capi.ERR_INVALID and np.all(x == 777.0) and not it.any() and not res.any()
        return capi.load().egs_last_error(ctx.h).decode()

    eye = lambda n: np.eye(n).reshape(-1)
    refused([2, 1025, 2], np.concatenate([eye(2), eye(1025), eye(2)]), np.ones(1029), prm)
    refused([2, -1, 2], np.concatenate([eye(2), eye(2)]), np.ones(4), prm)
    assert raw(ctx, [-1], none, none, prm, np.zeros(1))[0] == capi.ERR_INVALID
    assert capi.load().egs_dense_iterate_batch(ctx.h, ct.c_int32(-1), None, None, None, None, None, None, ct.byref(prm), None, None,
                                               None, None) == capi.ERR_INVALID
    two = (np.concatenate([eye(2), eye(3)]), np.ones(5))
    refused([2, 3], *two, capi.params(method=3))
    refused([2, 3], *two, capi.params(method=capi.SOR, omega=2.0))
    refused([2, 3], *two, capi.params(method=capi.GAUSS_SEIDEL, omega=0.0))      # the single entry refuses it for every method
    refused([2, 3], *two, capi.params(method=capi.GAUSS_SEIDEL, max_iters=-1))
    # a zero on the diagonal of problem 3 of 5: named, and nothing is written
    mats = [np.eye(n) * 2.0 for n in (2, 100, 3, 4, 2)]
    mats[3][2, 2] = 0.0
    msg = refused([2, 100, 3, 4, 2], np.concatenate([m.reshape(-1) for m in mats]), np.ones(111), prm)
    assert "problem 3" in msg
    # the divergent 2 x 2 Jacobi splitting of test_gpu_dense_iter.py, between neighbours that converge
    rng = np.random.default_rng(5)
    good = [diag_dominant(rng, 7), diag_dominant(rng, 120)]
    As = [good[0], np.array([[1.0, 3.0], [3.0, 1.0]]), good[1]]
    bs = [rng.uniform(-1, 1, 7), np.ones(2), rng.uniform(-1, 1, 120)]
    xs, its, rs = ctx.dense_iterate_batch(As, bs, capi.params(method=capi.JACOBI, max_iters=25, tol=TOL))
    want = [orc.dense_iterate(A, b, capi.JACOBI, max_iters=25) for A, b in zip(As, bs)]
    assert_equal_to((xs, its, rs), want)
    assert its[1] == 25 and not rs[1] <= TOL
    assert 0 < its[0] < 25 and rs[0] <= TOL
