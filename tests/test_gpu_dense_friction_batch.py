"""GPU (-m gpu): egs_mixed_friction_solve_batch -- the Coulomb pyramid on the dense direct solver, many explicit
problems in one call -- against the certified fixed-point iteration of dense_friction_reference.py (DESIGN.md sections 4g
and 7e): the random cases on both sides of the 32 / 64 / 112 class edges and of the fused limit in one ragged batch, the
batch as the sum of its parts, the plain batch's bits without pyramid rows, a run that does not converge, the refusals."""
import ctypes as C

import numpy as np
import pytest

import dense_friction_reference as dfr
from eggshell_amd import capi

pytestmark = pytest.mark.gpu


def pack(cases):
    ns = np.array([c.n for c in cases], np.int32)
    cat = lambda vs, dt: np.concatenate([np.asarray(v, dtype=dt).reshape(-1) for v in vs]) if vs else np.zeros(0, dt)
    return dict(ns=ns, A=cat([c.A for c in cases], np.float64), b=cat([c.b for c in cases], np.float64),
                C=cat([c.Ceq for c in cases], np.uint8), lo=cat([c.lo for c in cases], np.float64),
                hi=cat([c.hi for c in cases], np.float64), normal_row=cat([c.nrow for c in cases], np.int32),
                mu=cat([c.mu for c in cases], np.float64))


def run(ctx, cases, **kw):
    """The batch's answer split per problem: a list of dicts (ok, x, w, beta, pivots, outer, change, converged)."""
    out = ctx.mixed_friction_solve_batch_packed(**pack(cases), **kw)
    at = np.concatenate([[0], np.cumsum([c.n for c in cases])])
    return [dict(ok=bool(out["ok"][k]), pivots=int(out["pivots"][k]), outer=int(out["outer"][k]), change=float(out["change"][k]),
                 converged=bool(out["converged"][k]), **{q: out[q][at[k]:at[k + 1]] for q in ("x", "w", "beta")})
            for k in range(len(cases))]


def same_bits(a, b):
    return all(a[q] == b[q] for q in ("ok", "pivots", "outer")) and np.float64(a["change"]).tobytes() == np.float64(b["change"]).tobytes() \
        and all(a[q].tobytes() == b[q].tobytes() for q in ("x", "w", "beta"))


@pytest.fixture(scope="module")
def random_cases():
    return [dfr.case(cid) for cid in dfr.RANDOM]


@pytest.fixture(scope="module")
def batch(ctx, random_cases):
    return run(ctx, random_cases)


def test_the_ragged_batch_against_the_reference(random_cases, batch):
    """Per problem: ok, the reference's solve count, converged, x within C kappa u max(1, |x_ref|), pinned rows exactly 0,
    rows the reference has at +-beta at the device's own beta bit for bit, w = 0 bit for bit on equality rows,
    change <= tol."""
    bad = []
    for c, got in zip(random_cases, batch):
        ref = dfr.solved(c.id)
        ratio = dfr.x_ratio(ref, got["x"]) if got["ok"] else np.inf
        print("%s: ok %s outer %d (reference %d) change %.3g pivots %d x %.3g / %g" %
              (c.id, got["ok"], got["outer"], ref.outer, got["change"], got["pivots"], ratio, dfr.BOUNDS[c.cls]))
        eq = (c.Ceq != 0) & (c.nrow < 0)
        pyr = c.nrow >= 0
        at_bound = pyr & (ref.beta > 0) & (np.abs(ref.x) == ref.beta)
        checks = {
            "ok": got["ok"],
            "outer": got["outer"] == ref.outer,
            "converged": got["converged"] and got["change"] <= dfr.TOL,
            "x": ratio <= dfr.BOUNDS[c.cls],
            "pinned": (got["x"][ref.pinned].view(np.uint64) == 0).all() and (got["beta"][ref.pinned] == 0).all(),
            "at bound": (np.abs(got["x"][at_bound]) == got["beta"][at_bound]).all() and (got["beta"][at_bound] > 0).all(),
            "side": (np.sign(got["x"][at_bound]) == np.sign(ref.x[at_bound])).all(),
            "w eq": (got["w"][eq].view(np.uint64) == 0).all(),
            "beta plain": (got["beta"][~pyr] == 0).all(),
        }
        bad += [(c.id, k) for k, v in checks.items() if not v]
    assert not bad, bad


def test_each_problem_alone_in_the_batch_and_in_the_reversed_batch(ctx, random_cases, batch):
    rev = run(ctx, random_cases[::-1])[::-1]
    for k, c in enumerate(random_cases):
        alone = run(ctx, [c])[0]
        assert same_bits(alone, batch[k]), c.id
        assert same_bits(rev[k], batch[k]), c.id


def test_without_pyramid_rows_the_plain_batch_bits(ctx, random_cases):
    """normal_row = -1 everywhere: x, w, ok and pivots of egs_mixed_constraints_solve_batch(use_bounds = 1), outer 1."""
    plain = [dfr.Case(c.id, c.cls, c.A, c.b, c.Ceq, c.lo, c.hi, np.full(c.n, -1, np.int32), c.mu) for c in random_cases]
    got = run(ctx, plain)
    p = pack(plain)
    ok, x, w, piv = ctx.mixed_constraints_solve_batch_packed(p["ns"], p["A"], p["b"], p["C"], p["lo"], p["hi"], use_bounds=1)
    at = np.concatenate([[0], np.cumsum(p["ns"])])
    for k, c in enumerate(plain):
        g = got[k]
        assert g["ok"] == bool(ok[k]) and g["ok"], c.id
        assert g["pivots"] == piv[k] and g["outer"] == 1 and g["change"] == 0.0, c.id
        assert g["x"].tobytes() == x[at[k]:at[k + 1]].tobytes() and g["w"].tobytes() == w[at[k]:at[k + 1]].tobytes(), c.id
        assert (g["beta"] == 0).all()


def test_not_converging_is_not_a_failure(ctx):
    """max_outer = 2 on the mu = 0.5 pile: ok = 1, converged = 0, outer = 2, and the iterate is the reference's second."""
    c = dfr.case(dfr.NOT_CONVERGED)
    ref = dfr.solved(c.id, 2)
    got = run(ctx, [c], max_outer=2)[0]
    assert not ref.converged and ref.outer == 2
    assert got["ok"] and not got["converged"] and got["outer"] == 2
    assert got["change"] > dfr.TOL and abs(got["change"] - ref.change) <= 1e-6 * ref.change
    assert dfr.x_ratio(ref, got["x"]) <= dfr.BOUNDS[c.cls]


def _raw(ctx, p, max_pivots=0, max_outer=32, tol=1e-10, count=None):
    """The C entry itself with sentinel outputs: (status, outputs)."""
    tot = int(np.maximum(p["ns"], 0).sum())
    cnt = len(p["ns"]) if count is None else count
    outs = dict(x=np.full(tot, 7.0), w=np.full(tot, 7.0), beta=np.full(tot, 7.0), ok=np.full(max(cnt, 1), 7, np.int32),
                pivots=np.full(max(cnt, 1), 7, np.int32), outer=np.full(max(cnt, 1), 7, np.int32), change=np.full(max(cnt, 1), 7.0))
    ptr = capi._p
    st = capi.load().egs_mixed_friction_solve_batch(ctx.h, cnt, ptr(p["ns"]), ptr(p["A"]), ptr(p["b"]), ptr(p["C"]), ptr(p["lo"]),
                                                   ptr(p["hi"]), ptr(p["normal_row"]), ptr(p["mu"]), max_pivots, max_outer, tol,
                                                   *(ptr(outs[q]) for q in ("x", "w", "beta", "ok", "pivots", "outer", "change")))
    return st, outs


def _untouched(outs):
    return all((v == 7).all() for v in outs.values())


def test_refusals_leave_the_outputs_untouched(ctx):
    cases = [dfr.case("rnd-n6"), dfr.case("rnd-n30")]
    base = pack(cases)
    st, outs = _raw(ctx, base)
    assert st == capi.OK and not _untouched(outs)

    def changed(**kw):
        p = {k: v.copy() for k, v in base.items()}
        for k, (i, v) in kw.items():
            p[k][i] = v
        return p

    c1 = cases[1]
    pyr_row = 6 + int(np.flatnonzero(c1.nrow >= 0)[0])              # a pyramid row of the second problem
    eq_row = int(np.flatnonzero(c1.Ceq != 0)[0])                    # an equality row of it, as an index within the problem
    other_pyr = int(np.flatnonzero(c1.nrow >= 0)[-1])
    asym = changed()
    asym["A"][36 + 1] += 1.0
    refusals = {
        "normal_row too large": (changed(normal_row=(pyr_row, c1.n)), {}),
        "normal_row below -1": (changed(normal_row=(pyr_row, -2)), {}),
        "normal_row in another problem's range": (changed(normal_row=(0, 6)), {}),
        "normal_row at an equality row": (changed(normal_row=(pyr_row, eq_row)), {}),
        "normal_row at a pyramid row": (changed(normal_row=(pyr_row, other_pyr)), {}),
        "mu negative": (changed(mu=(pyr_row, -0.1)), {}),
        "mu NaN": (changed(mu=(pyr_row, np.nan)), {}),
        "max_outer < 0": (base, dict(max_outer=-1)),
        "tol < 0": (base, dict(tol=-1e-10)),
        "tol NaN": (base, dict(tol=float("nan"))),
        "max_pivots < 0": (base, dict(max_pivots=-1)),
        "count < 0": (base, dict(count=-1)),
        "n < 0": (changed(ns=(0, -6)), {}),
        "asymmetric": (asym, {}),
    }
    for what, (p, kw) in refusals.items():
        st, outs = _raw(ctx, p, **kw)
        assert st == capi.ERR_INVALID, what
        assert _untouched(outs), what
    # a negative or NaN mu on a PLAIN row is not looked at
    plain_row = int(np.flatnonzero(cases[0].nrow < 0)[0])
    st, outs = _raw(ctx, changed(mu=(plain_row, -1.0)))
    assert st == capi.OK
    # a NULL among the required arrays
    lib = capi.load()
    p = base
    st = lib.egs_mixed_friction_solve_batch(ctx.h, 2, capi._p(p["ns"]), capi._p(p["A"]), capi._p(p["b"]), capi._p(p["C"]), capi._p(p["lo"]),
                                            capi._p(p["hi"]), None, capi._p(p["mu"]), 0, 32, 1e-10, *([None] * 7))
    assert st == capi.ERR_INVALID
