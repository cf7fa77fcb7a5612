"""CPU: tests/lcp_reference.py against the mathematics (Fraction, mpmath at 50 digits, the reference's own KAT), and
the CPU statements of the dense direct solvers -- the oracle where it runs, a plain numpy Cholesky solve of the
certified system at every size -- against it, on the cases the GPU tests use.  The figures
printed by test_cpu_statements_against_the_reference are the ones the constants of lcp_reference.BOUNDS come from."""
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import lcp_reference as lr
from oracle import oracle as orc
from test_oracle_lcp import A1, B1, W1, X1

INF = np.inf


def _mixed(rng, n, eq_frac=0.4):
    M = rng.uniform(-1, 1, (n, n))
    A = M.T @ M / n + 0.5 * np.eye(n)
    b = rng.uniform(-3, 3, n)
    Ceq = (rng.uniform(size=n) < eq_frac).astype(np.uint8)
    lo = np.where(rng.uniform(size=n) < 0.5, -0.2, 0.0)
    hi = np.where(rng.uniform(size=n) < 0.5, 0.3, INF)
    return A, b, Ceq, lo, hi


def test_two_prod_is_exact():
    """p + e == a b as rationals on seeded pairs, entries with all 53 significant bits among them."""
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-1, 1, 200), rng.standard_normal(200) * 1e3, np.ldexp(rng.integers(2 ** 52, 2 ** 53, 200).astype(np.float64), -40),
                        [1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 0.0, -3.0]])
    b = np.concatenate([rng.uniform(-1, 1, 200), rng.standard_normal(200) * 1e-3, np.ldexp(rng.integers(2 ** 52, 2 ** 53, 200).astype(np.float64), -60),
                        [1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 5.0, 1.0 / 3.0]])
    p, e = lr.two_prod(a, b)
    assert np.array_equal(p, a * b)
    assert (e != 0).sum() > 500
    for ai, bi, pi, ei in zip(a.tolist(), b.tolist(), p.tolist(), e.tolist()):
        assert Fraction(pi) + Fraction(ei) == Fraction(ai) * Fraction(bi)


def test_exact_rows_equals_mpmath_after_one_rounding():
    """A x - b from a three-part x at n = 40, and with the extra column: the exact sum, rounded once, is mpmath's
    50-digit value rounded once."""
    rng = np.random.default_rng(2)
    n = 40
    A = rng.standard_normal((n, n))
    b = rng.standard_normal(n)
    parts = [rng.standard_normal(n), rng.standard_normal(n) * 1e-16, rng.standard_normal(n) * 1e-32]
    parts[0][::7] = 0.0
    extra = rng.standard_normal(n)
    got = lr.exact_rows(A, b, parts, np.arange(n))
    got_e = lr.exact_rows(A, b, parts, np.arange(5, n), extra=extra)
    with mp.workdps(50):
        x = [sum(mp.mpf(float(p[c])) for p in parts) for c in range(n)]
        want = [sum(mp.mpf(float(A[r, c])) * x[c] for c in range(n)) - mp.mpf(float(b[r])) for r in range(n)]
        assert got.tolist() == [float(v) for v in want]
        assert got_e.tolist() == [float(want[r] + mp.mpf(float(extra[r]))) for r in range(5, n)]
        d = lr.error_units(b, parts)
        assert d.tolist() == [float(mp.mpf(float(b[c])) - x[c]) for c in range(n)]


@pytest.mark.parametrize("n", [7, 64, 130])
def test_certify_equals_mpmath_cholesky_solve(n):
    """The parts of certify() sum to mpmath's cholesky_solve of the same set's system to 1e-28 relative."""
    A, b, Ceq, lo, hi = _mixed(np.random.default_rng(20 + n), n)
    ref = lr.solve(A, b, Ceq, lo, hi)
    S = np.flatnonzero(ref.state <= lr.FREE)
    Cl = np.flatnonzero(ref.state >= lr.LO)
    assert S.size > n // 3 and Cl.size > 0
    with mp.workdps(50):
        xC = [mp.mpf(float(v)) for v in ref.parts[0]]
        rhs = mp.matrix([mp.mpf(float(b[r])) - sum(mp.mpf(float(A[r, c])) * xC[c] for c in Cl) for r in S])
        ASS = mp.matrix([[mp.mpf(float(A[r, c])) for c in S] for r in S])
        want = mp.cholesky_solve(ASS, rhs)
        got = [sum(mp.mpf(float(p[r])) for p in ref.parts) for r in S]
        scale = max(abs(v) for v in want)
        assert max(abs(g - v) for g, v in zip(got, want)) <= mp.mpf("1e-28") * scale
        assert ref.x[S].tolist() == [float(v) for v in got]


def test_known_answer_of_the_reference():
    """lcp.cc:367-389: A1, B1 -> X1, W1 to the 5e-4 of its four printed digits."""
    n = 5
    ref = lr.solve(A1, B1, np.zeros(n, np.uint8), np.zeros(n), np.full(n, INF))
    assert np.linalg.norm(ref.x - X1) <= 5e-4 and np.linalg.norm(ref.w - W1) <= 5e-4
    assert ref.state.tolist() == [lr.FREE, lr.LO, lr.LO, lr.LO, lr.FREE]


def test_all_equality_rows_equal_a_linear_solve():
    rng = np.random.default_rng(3)
    n = 50
    A, b, _, lo, hi = _mixed(rng, n)
    ref = lr.solve(A, b, np.ones(n, np.uint8), lo, hi)
    assert (ref.state == lr.EQ).all()
    assert np.abs(ref.x - np.linalg.solve(A, b)).max() <= 1e-12 * np.abs(ref.x).max()
    assert np.abs(ref.w).max() <= 1e-25


def test_wrong_sets_are_refused():
    """One row flipped, in every direction a row can be flipped, and certify raises."""
    A, b, Ceq, lo, hi = _mixed(np.random.default_rng(4), 30)
    state = lr.find_set(A, b, Ceq, lo, hi)
    lr.certify(A, b, Ceq, lo, hi, state)
    flips = 0
    for r in range(30):
        for to in (lr.EQ, lr.FREE, lr.LO, lr.HI):
            if to == state[r]:
                continue
            bad = state.copy()
            bad[r] = to
            with pytest.raises(lr.NotCertified):
                lr.certify(A, b, Ceq, lo, hi, bad)
            flips += 1
    assert flips == 90
    with pytest.raises(lr.NotCertified):
        lr.certify(A + np.triu(np.full((30, 30), 1e-13), 1), b, Ceq, lo, hi, state)      # not symmetric
    with pytest.raises(lr.NotCertified):
        lr.certify(A - 2.0 * np.eye(30), b, Ceq, lo, hi, state)                            # not positive definite


def test_find_set_on_an_ill_conditioned_matrix():
    """kappa_2(A) = 1e12, where a block rule may cycle: with the single-index fallback the set is found, and the
    refinement still reaches 30 digits (it runs until the correction is small, not for a fixed count)."""
    rng = np.random.default_rng(5)
    n = 60
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.exp(rng.uniform(np.log(1e-12), 0.0, n))
    A = (Q * ev) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.uniform(-1, 1, n)
    ref = lr.solve(A, b, np.zeros(n, np.uint8), np.zeros(n), np.full(n, INF))
    assert (ref.state == lr.LO).any() and (ref.state == lr.FREE).any()


@pytest.mark.parametrize("cid", lr.CASES)
def test_margins_of_every_case(cid):
    """Strict complementarity with room: the smallest distance of a free inequality row from its bounds is at least
    2^10 x the case's bound on x, the smallest |w| on a clamped row at least 2^10 C_w u mag_r.  Asserted on the
    reference alone; a seed that missed was replaced when the list was written (lcp_reference.SEED_SHIFT), so no
    case is skipped at run time."""
    c, ref = lr.case(cid), lr.reference(cid)
    for cls in {c.cls, lr.lcp_class(c, True)}:
        C = lr.BOUNDS[cls]
        xb = C["x"] * ref.kappa * lr.U * max(1.0, np.abs(ref.x).max())
        print("%s [%s]: kappa %.3g, free margin / x bound %.3g, clamped |w| / (C_w u mag) %.3g" %
              (cid, cls, ref.kappa, ref.margin_x / xb, ref.margin_w / C["w"]))
        assert lr.margins_ok(ref, cls)


def cpu_statements(c, ref):
    """(name, class, ok, x, w, pivots) of every CPU statement of a case."""
    out = [("numpy", c.cls, True) + lr.numpy_statement(ref, c.A, c.b) + (None,)]
    if c.cls.startswith("incr"):
        if c.nub == 0:
            r = orc.tk_box_dantzig(c.A, c.b, c.lo, c.hi)
            out.append(("dantzig", c.cls, r[0], r[1], r[2], r[5]))
            r = orc.tk_box_murty(c.A, c.b, c.lo, c.hi)
            out.append(("murty", lr.lcp_class(c, True), r[0], r[1], r[2], r[5]))
        for alg in (0, 1):
            r = orc.tk_box_schur(c.A, c.b, c.lo, c.hi, algorithm=alg)
            assert r[5] == c.nub
            out.append(("schur%d" % alg, lr.lcp_class(c, alg == 0), r[0], r[1], r[2], r[6]))
    elif c.n <= 300:
        r = orc.mixed_constraints(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=c.use_bounds)
        out.append(("mixed", c.cls, r[0], r[1], r[2], r[3]))
    return out


@pytest.mark.parametrize("cid", lr.CASES)
def test_cpu_statements_against_the_reference(cid):
    """Every CPU statement of every case: ok, the certified active set row for row, and x, backward error and w within
    the constants these very figures produced (x 8, rounded up to a power of two).  find_set's state is the state read
    off the oracle's x on every case the oracle's rule finishes."""
    c, ref = lr.case(cid), lr.reference(cid)
    assert np.array_equal(lr.find_set(c.A, c.b, c.Ceq, c.lo, c.hi), ref.state)
    for name, cls, ok, x, w, piv in cpu_statements(c, ref):
        assert ok, (cid, name)
        fig = lr.measure(ref, c.A, c.b, c.Ceq, c.lo, c.hi, x, w)
        print("%s %s [%s]: x %.3g  b %.3g  wf %.3g  wc %.3g" % (cid, name, cls, fig["x"], fig["b"], fig["wf"], fig["wc"]))
        assert np.array_equal(lr.state_of(x, c.Ceq, c.lo, c.hi), ref.state), (cid, name)
        assert not lr.within(fig, cls), (cid, name, lr.within(fig, cls), fig)


def test_pile_without_bounds_is_degenerate():
    """use_bounds = 0 on a pile (quirk Q3: every inequality row gets lo = 0, hi = inf): the tangential rows of the
    symmetric pile have x = 0 AND w = 0 in exact arithmetic, so there is no strict complementarity, no certificate,
    and the reference's rule runs into its 1000-pivot cap.  The piles are cases with
    use_bounds = 1 only."""
    c = lr.case("pile222-cfm0.01")
    ok, _, _, piv = orc.mixed_constraints(c.A, c.b, c.Ceq, c.lo, c.hi, use_bounds=0)
    assert not ok and piv == 1000
