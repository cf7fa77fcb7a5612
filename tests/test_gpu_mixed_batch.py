"""GPU (-m gpu): egs_mixed_constraints_solve_batch -- Lcp::MixedConstraintsSolver (lcp.cc:276-336) on many explicit
problems in one fused pipeline -- through the C ABI against the oracle's restatement (oracle/lcp_dense.c) and numpy KKT
residuals: a ragged batch on both sides of every size class and of the fused cap, the batch as the sum of its parts
(bit for bit), the reference's own test (100 problems of 50 rows, lcp.cc:412-528) as one call, ensemble matrices,
failures that stay where they are, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from eggshell_amd import capi, scenes
from helpers import ode_rhs_from_scene, system_from_scene
from oracle import oracle as orc
from test_oracle_lcp import A1, B1, W1, X1, _spd

pytestmark = pytest.mark.gpu
INF = np.inf
SIZES = [0, 1, 2, 3, 5, 7, 24, 31, 32, 33, 50, 63, 64, 65, 96, 111, 112, 113, 128]
FUSED_MAX = 112
KINDS = ("random", "equality", "inequality")


def ragged_problems(use_bounds):
    """Every size three times -- random C, all-equality, all-inequality on one matrix and right-hand side -- from
    default_rng(2024)."""
    rng = np.random.default_rng(2024)
    probs = []
    for n in SIZES:
        A = _spd(rng, n) if n else np.zeros((0, 0))
        if use_bounds:
            A = A + 0.5 * np.eye(n)
        b = rng.uniform(-3, 3, n) if use_bounds else rng.uniform(-1, 1, n)
        lo, hi = (np.full(n, -0.3), np.full(n, 0.4)) if use_bounds else (np.zeros(n), np.full(n, INF))
        for kind in KINDS:
            Ceq = rng.integers(0, 2, n).astype(np.uint8) if kind == "random" else np.full(n, 1 if kind == "equality" else 0, np.uint8)
            probs.append((A, b, Ceq, lo, hi))
    return probs


def oracle_all(probs, use_bounds):
    return [orc.mixed_constraints(*p, use_bounds=use_bounds) if p[1].size else (True, np.zeros(0), np.zeros(0), 0) for p in probs]


def run_batch(ctx, probs, use_bounds, max_pivots=0):
    cols = [list(c) for c in zip(*probs)]
    return ctx.mixed_constraints_solve_batch(*cols, use_bounds=use_bounds, max_pivots=max_pivots)


@pytest.fixture(scope="module")
def ragged():
    """use_bounds -> (problems, the oracle's answers); computed once, never changed."""
    out = {}
    for ub in (0, 1):
        probs = ragged_problems(ub)
        out[ub] = (probs, oracle_all(probs, ub))
    return out


@pytest.fixture(scope="module")
def ragged_gpu(ctx, ragged):
    """use_bounds -> the batch's answer on the ragged problems (one call each)."""
    return {ub: run_batch(ctx, ragged[ub][0], ub) for ub in (0, 1)}


def check_against_oracle(probs, got, want, use_bounds, single_pivots=None, tol=1e-8):
    """Every problem of the batch: ok, pivots, x, w against the oracle, the residual, w on the equality rows, bounds."""
    oks, xs, ws, pivs = got
    assert len(oks) == len(xs) == len(ws) == len(pivs) == len(probs)
    for k, ((A, b, Ceq, lo, hi), (oko, xo, wo, pivo)) in enumerate(zip(probs, want)):
        n = b.size
        eq = Ceq.astype(bool)
        assert oko, k                                  # the inputs are solvable: the oracle says so
        assert oks[k] == oko, (k, n)
        if (~eq).any():
            assert pivs[k] == pivo, (k, n, pivs[k], pivo)
        else:      # no inequality row: the device paths skip the loop (the oracle counts 1 under use_bounds = 1)
            assert pivs[k] == (single_pivots[k] if single_pivots is not None else 0), (k, n, pivs[k])
        x, w = xs[k], ws[k]
        assert x.shape == (n,) and w.shape == (n,)
        scale = max(1.0, np.abs(xo).max(initial=0.0))
        assert np.abs(x - xo).max(initial=0.0) <= tol * scale, (k, n, np.abs(x - xo).max())
        assert np.abs(w - wo).max(initial=0.0) <= tol * scale, (k, n, np.abs(w - wo).max())
        assert np.linalg.norm(A @ x - b - w) < 1e-9, (k, n, np.linalg.norm(A @ x - b - w))
        assert (w[eq] == 0).all(), k
        if use_bounds:
            assert (x[~eq] >= lo[~eq]).all() and (x[~eq] <= hi[~eq]).all(), k
        else:
            assert (x[~eq] >= 0).all(), k


@pytest.mark.parametrize("use_bounds", [0, 1])
def test_ragged_batch_against_the_oracle(ctx, ragged, ragged_gpu, use_bounds):
    probs, want = ragged[use_bounds]
    # what the single entry counts where there is no inequality row (0: it skips the loop)
    single = [ctx.mixed_constraints_solve(*p, use_bounds=use_bounds)[3] if p[1].size and p[2].all() else None for p in probs]
    assert all(v == 0 for v in single if v is not None)
    check_against_oracle(probs, ragged_gpu[use_bounds], want, use_bounds, [v if v is not None else 0 for v in single])


def same_bits(a, b, k):
    """problem k of answer a == problem 0 ... of answer b given as (ok, x, w, pivots) tuples"""
    assert a[0] == b[0] and a[3] == b[3], (k, a[0], b[0], a[3], b[3])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), k


def slot(got, k):
    return got[0][k], got[1][k], got[2][k], got[3][k]


@pytest.mark.parametrize("use_bounds", [0, 1])
def test_the_batch_is_the_sum_of_its_parts(ctx, ragged, ragged_gpu, use_bounds):
    probs, _ = ragged[use_bounds]
    got = ragged_gpu[use_bounds]
    again = run_batch(ctx, probs, use_bounds)
    back = run_batch(ctx, probs[::-1], use_bounds)
    for k, p in enumerate(probs):
        same_bits(slot(again, k), slot(got, k), k)
        same_bits(slot(back, len(probs) - 1 - k), slot(got, k), k)
        n = p[1].size
        if n <= FUSED_MAX:      # alone in a batch: the bits of its slot
            same_bits(slot(run_batch(ctx, [p], use_bounds), 0), slot(got, k), k)
        else:                   # beyond the fused cap: the single path, bit for bit
            ok, x, w, piv = ctx.mixed_constraints_solve(*p, use_bounds=use_bounds)
            same_bits((ok, x, w, piv), slot(got, k), k)


def test_block_pivoting_problems_are_the_single_path(ctx, ragged):
    """bit 1 (block principal pivoting) is never fused: every problem equals the single entry bit for bit."""
    for ub in (2, 3):
        probs = [p for p in ragged[ub & 1][0] if p[1].size in (0, 7, 50, 113)]
        got = run_batch(ctx, probs, ub)
        for k, p in enumerate(probs):
            if p[1].size == 0:
                assert got[0][k] and got[3][k] == 0
                continue
            same_bits(tuple(ctx.mixed_constraints_solve(*p, use_bounds=ub)), slot(got, k), k)


def test_the_references_own_test_as_one_call(ctx):
    """lcp.cc:412-528: 100 random mixed problems of 50 rows; Murty KAT 1 (no equality rows) rides along as problem 101."""
    rng = np.random.default_rng(7)
    probs = []
    for _ in range(100):
        A = _spd(rng, 50)
        b = rng.uniform(-1, 1, 50)
        Ceq = rng.integers(0, 2, 50).astype(np.uint8)
        probs.append((A, b, Ceq, np.zeros(50), np.full(50, INF)))
    probs.append((A1, B1, np.zeros(5, np.uint8), np.zeros(5), np.full(5, INF)))
    got = run_batch(ctx, probs, 0)
    assert all(got[0]) and len(got[0]) == 101
    check_against_oracle(probs[:100], tuple(v[:100] for v in got), oracle_all(probs[:100], 0), 0)
    x, w = got[1][100], got[2][100]
    assert np.linalg.norm(x - X1) <= 5e-4 and np.linalg.norm(w - W1) <= 5e-4
    assert np.linalg.norm(A1 @ x - B1 - w) < 1e-9


def grounded(sc):
    """the scene with the ground contacts of its boxes behind its joints"""
    kind, b0, b1, data = [sc["kind"]], [sc["body0"]], [sc["body1"]], [sc["data"]]
    for b in range(sc["p"].shape[0]):
        cs = orc.collide_box_ground(sc["p"][b], sc["R"][b])
        kind.append(np.full(len(cs), capi.CONTACT_BOX, np.int32)); b0.append(np.full(len(cs), -1, np.int32))
        b1.append(np.full(len(cs), b, np.int32)); data.append(cs.reshape(-1, 7))
    out = dict(sc)
    out.update(kind=np.concatenate(kind).astype(np.int32), body0=np.concatenate(b0).astype(np.int32),
               body1=np.concatenate(b1).astype(np.int32), data=np.concatenate(data))
    return out


def ensemble_problem(sc, cfm=None):
    s, err = system_from_scene(sc)
    rhs, _ = ode_rhs_from_scene(sc, s, err, 1e-3)
    A = orc.dense_JMJt(s, 0.0)
    if cfm is None:
        cfm = 0.0 if np.linalg.cond(A) < 1e7 else 0.01      # ensembles.cc:513-521
    return orc.dense_JMJt(s, cfm), rhs, s.is_eq.astype(np.uint8), s.lo, s.hi


def test_ensemble_matrices(ctx):
    """J M^-1 J^T of Chain(8) (24 equality rows), of a grounded Chain(4) (joints and contacts) and of a 2x2x2 pile with
    cfm = 0.01 (96 rows), one batch per use_bounds, against the oracle at 1e-8."""
    chain8 = ensemble_problem(scenes.chain(8))
    low = grounded(scenes.chain(4, anchor=(0.0, 0.0, 0.205)))
    assert (low["kind"] == capi.CONTACT_BOX).sum() >= 1 and (low["kind"] == capi.JOINT_BALL).sum() == 4
    chain4 = ensemble_problem(low)
    pile = ensemble_problem(scenes.box_stack(2, 2, 2), cfm=0.01)
    assert chain8[1].size == 24 and chain8[2].all() and pile[1].size == 96
    # Chain(8) has no inequality row: it runs the same under either mask
    got0 = run_batch(ctx, [chain8], 0)
    check_against_oracle([chain8], got0, oracle_all([chain8], 0), 0)
    probs = [chain8, chain4, pile]
    got = run_batch(ctx, probs, 1)
    want = oracle_all(probs, 1)
    oks, xs, ws, pivs = got
    for k, ((A, b, Ceq, lo, hi), (oko, xo, wo, pivo)) in enumerate(zip(probs, want)):
        eq = Ceq.astype(bool)
        assert oko and oks[k], k
        assert pivs[k] == (pivo if (~eq).any() else 0), (k, pivs[k], pivo)
        scale = max(1.0, np.abs(xo).max())
        assert np.abs(xs[k] - xo).max() <= 1e-8 * scale and np.abs(ws[k] - wo).max() <= 1e-8 * scale, k
        assert (ws[k][eq] == 0).all(), k
        assert (xs[k][~eq] >= lo[~eq]).all() and (xs[k][~eq] <= hi[~eq]).all(), k


def test_failure_stays_where_it_is(ctx, ragged, ragged_gpu):
    probs = list(ragged[0][0])
    good = ragged_gpu[0]
    ka = 3 * SIZES.index(24)            # 24 rows, random C: a negative diagonal on an equality row
    kb = 3 * SIZES.index(50) + 2        # 50 rows, all inequality: an indefinite block
    A, b, Ceq, lo, hi = probs[ka]
    e = int(np.nonzero(Ceq)[0][0])
    Abad = A.copy(); Abad[e, e] = -1.0
    probs[ka] = (Abad, b, Ceq, lo, hi)
    A, b, Ceq, lo, hi = probs[kb]
    assert not Ceq.any()
    Aind = A - (np.linalg.eigvalsh(A)[0] + 0.5) * np.eye(50)
    assert np.linalg.eigvalsh(Aind)[0] < -0.4
    probs[kb] = (Aind, b, Ceq, lo, hi)
    got = run_batch(ctx, probs, 0)      # returns: the status was EGS_OK
    for k in range(len(probs)):
        if k in (ka, kb):
            assert not got[0][k], k
        else:
            same_bits(slot(got, k), slot(good, k), k)


@pytest.mark.parametrize("use_bounds", [0, 1])
def test_max_pivots_tightens_the_cap(ctx, ragged, use_bounds):
    probs, _ = ragged[use_bounds]
    got = run_batch(ctx, probs, use_bounds, max_pivots=1)
    some_fail = False
    for k, p in enumerate(probs):
        alone = ctx.mixed_constraints_solve(*p, use_bounds=use_bounds, max_pivots=1)[0] if p[1].size else True
        assert got[0][k] == alone, (k, p[1].size)
        some_fail |= not alone
    assert some_fail


def raw_call(ctx, ns, A, b, Ceq, lo, hi, use_bounds, max_pivots, x, w, ok, piv, count=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ns = np.ascontiguousarray(ns, np.int32)
    return capi.load().egs_mixed_constraints_solve_batch(ctx.h, len(ns) if count is None else count, p(ns), p(A), p(b), p(Ceq), p(lo), p(hi),
                                                         use_bounds, max_pivots, p(x), p(w), p(ok), p(piv))


def test_refusals(ctx):
    rng = np.random.default_rng(11)
    sizes = [4, 0, 9, 6, 3]
    As = [_spd(rng, n) + 0.2 * np.eye(n) if n else np.zeros((0, 0)) for n in sizes]
    tot = sum(sizes)
    ns = np.array(sizes, np.int32)
    A = np.concatenate([a.reshape(-1) for a in As])
    b = rng.uniform(-1, 1, tot)
    Ceq = rng.integers(0, 2, tot).astype(np.uint8)
    lo, hi = np.zeros(tot), np.full(tot, INF)
    SENT = -777.25

    def refused(what, ns_=ns, A_=A, ub=0, mp=0, count=None, **null):
        x, w = np.full(tot, SENT), np.full(tot, SENT)
        ok, piv = np.full(len(sizes), -7, np.int32), np.full(len(sizes), -7, np.int32)
        arrs = dict(A=A_, b=b, Ceq=Ceq, lo=lo, hi=hi, x=x, w=w)
        for name in null:
            arrs[name] = None
        st = raw_call(ctx, ns_, arrs["A"], arrs["b"], arrs["Ceq"], arrs["lo"], arrs["hi"], ub, mp, arrs["x"], arrs["w"], ok, piv, count)
        assert st == capi.ERR_INVALID, what
        assert (x == SENT).all() and (w == SENT).all() and (ok == -7).all() and (piv == -7).all(), what
        return capi.load().egs_last_error(ctx.h).decode()

    refused("count < 0", count=-1)
    bad = ns.copy(); bad[2] = -1
    refused("n < 0", ns_=bad)
    refused("use_bounds = 4", ub=4)
    refused("use_bounds = -1", ub=-1)
    refused("max_pivots < 0", mp=-1)
    for name in ("A", "b", "Ceq", "lo", "hi", "x", "w"):
        refused("NULL " + name, **{name: None})
    Abad = A.copy()
    off = 4 * 4 + 0 + 9 * 9          # problem 3 (6 rows) starts here
    Abad[off + 4 * 6 + 1] += 1e-3
    msg = refused("asymmetric", A_=Abad)
    assert "problem 3" in msg, msg
    # the same arrays are accepted; count = 0 is EGS_OK and touches nothing
    x, w = np.full(tot, SENT), np.full(tot, SENT)
    ok, piv = np.full(len(sizes), -7, np.int32), np.full(len(sizes), -7, np.int32)
    assert raw_call(ctx, ns, A, b, Ceq, lo, hi, 0, 0, x, w, ok, piv, count=0) == capi.OK
    assert (x == SENT).all() and (ok == -7).all()
    assert raw_call(ctx, ns, A, b, Ceq, lo, hi, 0, 0, x, w, ok, None) == capi.OK      # pivots may be NULL
    assert (ok == 1).all() and not (x == SENT).any()
    ok2, x2, w2, piv2 = ctx.mixed_constraints_solve_batch_packed(ns, A, b, Ceq, lo, hi)
    assert ok2.all() and np.array_equal(x2, x) and np.array_equal(w2, w) and piv2[1] == 0
    # nothing but empty problems, and an empty batch through the wrapper
    ok3, x3, w3, piv3 = ctx.mixed_constraints_solve_batch_packed([0, 0], np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), np.zeros(0), np.zeros(0))
    assert ok3.all() and x3.size == 0 and not piv3.any()
    assert ctx.mixed_constraints_solve_batch([], [], [], [], []) == ([], [], [], [])
