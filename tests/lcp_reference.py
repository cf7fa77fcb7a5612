"""The mixed box LCP as mathematics: a CERTIFIED reference for the dense direct solvers (dense_lcp.hip on
dense_factor.hip and dense_murty.hip, dantzig.hip, mixed_solve_device.h / mixed_batch.hip, the fused solve of
dense_world.hip).  numpy and math.fsum only; nothing from oracle/ takes part in a reference value, and no pivot rule is
restated.

  find x, w = A x - b with     w_r = 0                    on an equality row (x_r free)
                               lo_r <= x_r <= hi_r and    w_r = 0 inside, w_r >= 0 on lo_r, w_r <= 0 on hi_r   otherwise

With A symmetric positive definite the problem has exactly one solution (it is the minimiser of a strictly convex
quadratic over a box).  So the reference needs no pivot rule, only a CERTIFICATE: a state per row (equality / free /
at lo / at hi) whose linear system, solved to 30 digits, satisfies every condition STRICTLY.  Such a state is the
solution's, whoever proposed it.

  find_set  (untrusted)  block principal pivoting in plain fp64, with the single-index fallback when the number of
                         violated rows stops falling (without it the rule cycles on ill-conditioned matrices).
  certify   (trusted)    S = equality and free rows.  A_SS x_S = b_S - A_SC x_C by iterative refinement: corrections
                         from an fp64 Cholesky factor, residuals EXACT -- every product split into p + e by
                         Dekker / Veltkamp two_prod, every row summed by math.fsum -- and x kept as an unevaluated sum
                         of fp64 parts [x_C, d0, d1, ...] until a correction falls below 2^-100 |x|_inf.  Then
                         w = A x - b the same way, and the strict checks; any failure raises.

Beside every value stands mag_r = sum_c |A_rc| |x_c| + |b_r|, the quantity a rounding bound scales with.  Bounds
(u = 2^-53; kappa = kappa_2(A_SS) of the certified set):

  x                      |x - x_ref|_inf <= C_x kappa u max(1, |x_ref|_inf)
  backward error         |A_SS x_S - (b_S - A_SC x_C)|_inf <= C_b u (|A_SS|_inf |x|_inf + |b|_inf), exact at the result's x
  w, free rows           |w_r| <= C_w u mag_r
  w, clamped rows        |w_r - (A x - b)_r| <= C_w u mag_r, exact at the result's own x
  active set             the state read off x equals the certified state row for row; clamped x equal their bound
                         bit for bit; w = 0 bit for bit on equality rows

The constants are not derived from operation counts: per class the worst ratio of the CPU statements (the oracle where
it runs; a plain numpy Cholesky solve of the certified system everywhere) was measured, multiplied by 8 and rounded up
to a power of two (BOUNDS).  The factor 8 is the room a kernel with another summation order, another factorisation or
an rsq-based reciprocal may use.  Device figures never set a constant.

The seeded cases at the end are shared by the CPU tests (reference against the mathematics, oracle against the
reference) and the GPU tests, so both see identical inputs."""
import functools
import math

import numpy as np

U = 2.0 ** -53
INF = np.inf
EQ, FREE, LO, HI = 0, 1, 2, 3
_SPLIT = 134217729.0          # 2^27 + 1


class NotCertified(Exception):
    """certify(): the proposed state is not the solution's (or cannot be told from it at this precision)."""


# ---- exact arithmetic on fp64 data -----------------------------------------------------------------------------------
def two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product with Veltkamp's split; no overflow or
    underflow at the magnitudes used here).  Works element-wise on arrays."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_rows(A, b, parts, rows, extra=None, chunk=64):
    """fl(sum_c A_rc (sum_k parts[k]_c) - b_r [+ extra_r]) for r in rows, each row rounded ONCE: the sum itself is
    exact (two_prod, math.fsum).  parts: fp64 vectors whose unevaluated sum is x."""
    rows = np.asarray(rows, dtype=np.intp)
    out = np.zeros(rows.shape[0])
    cols = [np.flatnonzero(p) for p in parts]
    for at in range(0, rows.shape[0], chunk):
        rr = rows[at:at + chunk]
        blocks = [-b[rr][:, None]]
        if extra is not None:
            blocks.append(np.asarray(extra, dtype=np.float64)[rr][:, None])
        for p, c in zip(parts, cols):
            if c.size:
                blocks.extend(two_prod(A[np.ix_(rr, c)], p[c][None, :]))
        T = np.concatenate(blocks, axis=1)
        out[at:at + chunk] = [math.fsum(t) for t in T.tolist()]
    return out


def error_units(x_dev, parts):
    """fl(x_dev_i - sum_k parts[k]_i) per row, the difference exact before its one rounding: the 30-digit reference
    is never rounded before the comparison."""
    cols = [np.asarray(x_dev, dtype=np.float64)] + [-np.asarray(p) for p in parts]
    return np.array([math.fsum(t) for t in np.stack(cols, axis=1).tolist()])


# ---- the untrusted proposer --------------------------------------------------------------------------------------------
def _solve_state(A, b, lo, hi, state):
    free = state <= FREE
    x = np.where(state == LO, lo, np.where(state == HI, hi, 0.0))
    if free.any():
        rhs = b[free] - A[np.ix_(free, ~free)] @ x[~free]
        x[free] = np.linalg.solve(A[np.ix_(free, free)], rhs)
    w = A @ x - b
    w[free] = 0.0
    return x, w


def find_set(A, b, Ceq, lo, hi, max_rounds=2000):
    """A state per row (EQ / FREE / LO / HI) from block principal pivoting in fp64 (Judice & Pires): flip every
    violated row while the count of violated rows falls, allow three rounds without progress, then flip only the
    violated row of the highest index until it falls again.  UNTRUSTED: certify() decides."""
    A, b, lo, hi = (np.asarray(v, dtype=np.float64) for v in (A, b, lo, hi))
    eq = np.asarray(Ceq).astype(bool)
    state = np.where(eq, EQ, np.where(np.isfinite(lo), LO, np.where(np.isfinite(hi), HI, FREE))).astype(np.int8)
    best, patience = b.shape[0] + 1, 3
    for _ in range(max_rounds):
        x, w = _solve_state(A, b, lo, hi, state)
        to_lo = (state == FREE) & (x < lo)
        to_hi = (state == FREE) & (x > hi)
        to_free = ((state == LO) & (w < 0)) | ((state == HI) & (w > 0))
        bad = np.flatnonzero(to_lo | to_hi | to_free)
        if bad.size == 0:
            return state
        if bad.size < best:
            best, patience = bad.size, 3
        elif patience > 0:
            patience -= 1
        else:
            bad = bad[-1:]
        for r in bad:
            state[r] = LO if to_lo[r] else (HI if to_hi[r] else FREE)
    raise RuntimeError("find_set: no feasible state in %d rounds" % max_rounds)


# ---- the certificate ---------------------------------------------------------------------------------------------------
class Reference:
    """parts: fp64 vectors whose unevaluated sum is the solution (30 digits); x, w: their one rounding; mag; state;
    kappa = kappa_2(A_SS); norm_SS = |A_SS|_inf; rounds: the residuals' norms, round by round; margin_x: min over free
    inequality rows of min(x - lo, hi - x); margin_w: min over clamped rows of |w_r| / (u mag_r)."""


def certify(A, b, Ceq, lo, hi, state, max_parts=12):
    A, b, lo, hi = (np.asarray(v, dtype=np.float64) for v in (A, b, lo, hi))
    eq = np.asarray(Ceq).astype(bool)
    state = np.asarray(state).astype(np.int8)
    n = b.shape[0]
    if A.shape != (n, n) or not np.array_equal(A, A.T):
        raise NotCertified("A is not a symmetric n x n matrix")
    if not np.array_equal(state == EQ, eq):
        raise NotCertified("equality rows and state disagree")
    if not (np.isfinite(lo[state == LO]).all() and np.isfinite(hi[state == HI]).all()):
        raise NotCertified("a row is clamped to an infinite bound")
    S = np.flatnonzero(state <= FREE)
    Cl = np.flatnonzero(state >= LO)
    xC = np.where(state == LO, lo, np.where(state == HI, hi, 0.0))
    parts = [xC]
    rounds = []
    w = np.zeros(n)
    if S.size:
        try:
            L = np.linalg.cholesky(A[np.ix_(S, S)])
        except np.linalg.LinAlgError:
            raise NotCertified("A_SS is not positive definite")
        Linv = np.linalg.solve(L, np.eye(S.size))
        ev = np.linalg.eigvalsh(A[np.ix_(S, S)])
        kappa, norm_SS = float(ev[-1] / ev[0]), float(np.abs(A[np.ix_(S, S)]).sum(axis=1).max())
        while True:
            r = -exact_rows(A, b, parts, S)                    # b_S - A_S: x, exact before its one rounding
            rounds.append(float(np.abs(r).max()))
            d = np.zeros(n)
            d[S] = Linv.T @ (Linv @ r)
            xmax = max(np.abs(sum(parts)).max(), np.abs(d).max())
            if np.abs(d).max() <= 2.0 ** -100 * xmax:
                w[S] = -r
                break
            if len(parts) >= max_parts:
                raise NotCertified("refinement did not converge: residuals %r" % rounds)
            parts.append(d)
    else:
        kappa, norm_SS = 1.0, 0.0
    w[Cl] = exact_rows(A, b, parts, Cl)
    x = error_units(np.zeros(n), [-p for p in parts])
    mag = np.abs(A) @ np.abs(x) + np.abs(b)
    # the strict checks.  The last correction was below 2^-100 |x|_inf, so x is off by about that and A x - b by about
    # 2^-100 |A|_inf |x|_inf: the residual must confirm it (2^-90 of its scale), and a sign is certified only if the
    # value clears 2^-60 of its scale -- far above either error and far below any bound of the tests.
    tiny = 2.0 ** -60
    xs = max(1.0, float(np.abs(x).max()))
    ws = float(np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
    if S.size and not (np.abs(w[S]) <= 2.0 ** -90 * ws).all():
        raise NotCertified("residual of the free rows is not at the 30-digit level")
    fr = state == FREE
    if not ((x[fr] - lo[fr] > tiny * xs).all() and (hi[fr] - x[fr] > tiny * xs).all()):
        raise NotCertified("a free row is not strictly inside its bounds")
    if not (w[state == LO] > tiny * ws).all():
        raise NotCertified("a row at lo has w <= 0")
    if not (w[state == HI] < -tiny * ws).all():
        raise NotCertified("a row at hi has w >= 0")
    ref = Reference()
    ref.parts, ref.x, ref.w, ref.mag, ref.state, ref.kappa, ref.norm_SS, ref.rounds = parts, x, w, mag, state, kappa, norm_SS, rounds
    ref.margin_x = float(np.minimum(x[fr] - lo[fr], hi[fr] - x[fr]).min(initial=INF))
    ref.margin_w = float((np.abs(w[Cl]) / (U * mag[Cl])).min(initial=INF))
    return ref


def solve(A, b, Ceq, lo, hi):
    """The certified solution: find_set proposes, certify decides."""
    return certify(A, b, Ceq, lo, hi, find_set(A, b, Ceq, lo, hi))


# ---- a result under test, in units of the bounds -------------------------------------------------------------------------
def state_of(x, Ceq, lo, hi):
    """The state read off a result: equality rows EQ; x == lo -> LO, x == hi -> HI (bit for bit), FREE otherwise."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.asarray(Ceq).astype(bool), EQ, np.where(x == lo, LO, np.where(x == hi, HI, FREE))).astype(np.int8)


def measure(ref, A, b, Ceq, lo, hi, x, w):
    """The figures of one result (x, w) against the certified reference:
      set   the state read off x equals the certified state, row for row
      weq   w == 0 bit for bit on every equality row
      x     |x - x_ref|_inf / (kappa u max(1, |x_ref|_inf))
      b     |A_SS x_S - (b_S - A_SC x_C)|_inf / (u (|A_SS|_inf |x|_inf + |b|_inf)), exact at the result's x
      wf    max over free inequality rows of |w_r| / (u mag_r)
      wc    max over clamped rows of |w_r - (A x - b)_r| / (u mag_r), exact at the result's own x
    and row_x, row_b, row_wf, row_wc: the row where each worst figure stands (-1: no such row)."""
    A, b, lo, hi, x, w = (np.asarray(v, dtype=np.float64) for v in (A, b, lo, hi, x, w))
    out = {"set": bool(np.array_equal(state_of(x, Ceq, lo, hi), ref.state)),
           "weq": bool((w[ref.state == EQ] == 0).all())}
    if not (np.isfinite(x).all() and np.isfinite(w).all()):
        out.update(x=INF, b=INF, wf=INF, wc=INF, row_x=-1, row_b=-1, row_wf=-1, row_wc=-1)
        return out

    def worst(rows, v):
        if not len(rows):
            return 0.0, -1
        k = int(np.argmax(v))
        return float(v[k]), int(rows[k])

    every = np.arange(b.shape[0])
    out["x"], out["row_x"] = worst(every, np.abs(error_units(x, ref.parts)) / (ref.kappa * U * max(1.0, np.abs(ref.x).max())))
    S = np.flatnonzero(ref.state <= FREE)
    Cl = np.flatnonzero(ref.state >= LO)
    r = exact_rows(A, b, [x], S)
    out["b"], out["row_b"] = worst(S, np.abs(r) / (U * (ref.norm_SS * np.abs(x).max() + np.abs(b).max())))
    F = np.flatnonzero(ref.state == FREE)
    out["wf"], out["row_wf"] = worst(F, np.abs(w[F]) / (U * ref.mag[F]))
    d = exact_rows(A, b, [x], Cl, extra=-w)                     # (A x - b)_r - w_r, exact before its one rounding
    out["wc"], out["row_wc"] = worst(Cl, np.abs(d) / (U * ref.mag[Cl]))
    return out


def numpy_statement(ref, A, b):
    """A CPU statement available at every size: the certified linear system solved by np.linalg.cholesky in plain fp64
    (two triangular solves), clamped rows at their bounds, w = A @ x - b, zero on equality rows."""
    x = ref.parts[0].copy()
    S = ref.state <= FREE
    if S.any():
        L = np.linalg.cholesky(A[np.ix_(S, S)])
        rhs = b[S] - A[np.ix_(S, ~S)] @ x[~S]
        x[S] = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    w = A @ x - b
    w[ref.state == EQ] = 0.0
    return x, w


# ---- bounds: C = 8 x the CPU statements' measured worst ratio, rounded up to a power of two -----
# class -> quantity: x (times kappa), b backward error, w rows of A x - b (free and clamped).  Classes: "single" the
# single-workgroup and fused kernels (n <= 112, the batch), "panel" the multi-panel factorisations (n >= 113), "incr"
# the incremental-factor Dantzig / Murty / Schur entries; "-hard" the spectrum and pile families, kept apart so that
# neither loosens the other (their x constants are the smaller ones: kappa is pessimistic there); "reducer-hard"
# BoxMurty on the spectrum family (lcp_class).  The measured ratios behind every figure are in DESIGN.md section 7d.
C_SINGLE = dict(x=32, b=16, w=32)
C_PANEL = dict(x=64, b=32, w=32)
C_INCR = dict(x=128, b=64, w=64)
C_SINGLE_HARD = dict(x=4, b=8, w=64)
C_PANEL_HARD = dict(x=2, b=8, w=64)
C_INCR_HARD = dict(x=2, b=8, w=32)
C_REDUCER_HARD = dict(x=32768, b=65536, w=16)
BOUNDS = {"single": C_SINGLE, "panel": C_PANEL, "incr": C_INCR,
          "single-hard": C_SINGLE_HARD, "panel-hard": C_PANEL_HARD, "incr-hard": C_INCR_HARD, "reducer-hard": C_REDUCER_HARD}


def lcp_class(c, reducer):
    """The class of a box LCP entry's result: BoxMurty on the LinearReducer (alone or inside BoxSchur) has a class of
    its own on the spectrum family, where its error follows kappa(A) and not kappa(A_SS)."""
    return "reducer-hard" if reducer and c.cls == "incr-hard" else c.cls
MARGIN = 2.0 ** 10      # strict complementarity: every case keeps this factor between its margins and its bounds


def within(fig, cls):
    """The assertions of one measured result against its class's constants; returns the list of what fails."""
    C = BOUNDS[cls]
    bad = [k for k in ("set", "weq") if not fig[k]]
    bad += [k for k, c in (("x", C["x"]), ("b", C["b"]), ("wf", C["w"]), ("wc", C["w"])) if not fig[k] <= c]
    return bad


def margins_ok(ref, cls):
    """min free margin >= 2^10 x the case's bound on x, min |w| on clamped rows >= 2^10 C_w u mag_r."""
    C = BOUNDS[cls]
    return (ref.margin_x >= MARGIN * C["x"] * ref.kappa * U * max(1.0, np.abs(ref.x).max())
            and ref.margin_w >= MARGIN * C["w"])


# ---- seeded cases (identical inputs for the CPU and the GPU tests) -----------------------------------------------------
class Case:
    """A, b, Ceq, lo, hi: the problem as handed to the code under test; use_bounds: the reference-rule flag of the
    mixed entry (0: bounds ignored, quirk Q3 -- lo = 0, hi = inf are what the case holds; 1: the box); cls: the class
    of BOUNDS; nub: leading rows without bounds (Schur cases)."""

    def __init__(self, cid, cls, A, b, Ceq, lo, hi, use_bounds=0, nub=0):
        self.id, self.cls, self.A, self.b, self.Ceq, self.lo, self.hi = cid, cls, A, b, Ceq, lo, hi
        self.use_bounds, self.nub = use_bounds, nub
        self.n = b.shape[0]


def _path(n):
    return "single" if n <= 112 else "panel"


def _c5(n, seed, eps=1e-3):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    A = M.T @ M + eps * np.eye(n)
    b = rng.uniform(-1, 1, n)
    Ceq = rng.integers(0, 2, n).astype(np.uint8)
    return A, b, Ceq, np.zeros(n), np.full(n, INF)


def _box_bounds(rng, n, eq_frac):
    Ceq = (rng.uniform(size=n) < eq_frac).astype(np.uint8)
    lo = np.where(rng.uniform(size=n) < 0.5, -0.2, 0.0)
    hi = np.where(rng.uniform(size=n) < 0.5, 0.3, INF)
    return Ceq, lo, hi


def _box(n, seed, eq_frac=0.4):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    A = M.T @ M / n + 0.5 * np.eye(n)
    b = rng.uniform(-3, 3, n)
    return (A, b) + _box_bounds(rng, n, eq_frac)


def _spectrum(n, seed, target, box, eq_frac=0.5):
    """Q diag(ev) Q^T symmetrised, log-uniform ev in [1 / target, 1] with the extremes pinned."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.exp(rng.uniform(np.log(1.0 / target), 0.0, n))
    ev[0] = 1.0
    if n > 1:
        ev[1] = 1.0 / target
    A = (Q * ev) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.uniform(-1, 1, n)
    if box:
        return (A, b) + _box_bounds(rng, n, eq_frac)
    Ceq = (rng.uniform(size=n) < eq_frac).astype(np.uint8)
    return A, b, Ceq, np.zeros(n), np.full(n, INF)


PILE_DT, PILE_ERP = 5e-3, 0.2


def _pile(dims, cfm):
    """J M^-1 J^T + cfm I of a box pile with its true ode_rhs (the oracle's assembly makes INPUTS only).  The upper
    triangle is mirrored from the lower one, which is what the factorisations read: the assembled matrix is symmetric
    only to rounding, and the certificate wants one matrix."""
    from eggshell_amd import scenes
    from helpers import ode_rhs_from_scene, system_from_scene
    from oracle import oracle as orc
    sc = scenes.box_stack(*dims)
    s, err = system_from_scene(sc)
    rhs, _ = ode_rhs_from_scene(sc, s, err, PILE_DT, PILE_ERP)
    A = orc.dense_JMJt(s, cfm)
    A = np.tril(A) + np.tril(A, -1).T
    return A, rhs, s.is_eq.copy(), s.lo.copy(), s.hi.copy()


def _with_unbounded(prob, nub):
    """The first nub rows lose their bounds (lo = -inf, hi = inf): what the Schur entries eliminate first."""
    A, b, Ceq, lo, hi = prob
    lo, hi = lo.copy(), hi.copy()
    lo[:nub], hi[:nub] = -INF, INF
    return A, b, Ceq, lo, hi


# id -> (builder, class, use_bounds, nub).  Seeds: 7000 + n for c5, 8000 + n for box, 9000 + n for spectrum, plus the
# replacement offset of a seed that missed the margins when the list was written (SEED_SHIFT).
SEED_SHIFT = {}
_BUILDERS = {}


def _seed(cid, base):
    return base + 100000 * SEED_SHIFT.get(cid, 0)


def _add(cid, build, cls, use_bounds=0, nub=0):
    _BUILDERS[cid] = (build, cls, use_bounds, nub)
    return cid


def _reg(kind, n, **kw):
    """Registers one case of a family at size n and returns its id."""
    if kind == "c5":
        cid = "c5-n%d" % n
        return _add(cid, lambda: _c5(n, _seed(cid, 7000 + n)), _path(n), 0)
    if kind == "box":
        cid = "box-n%d" % n
        return _add(cid, lambda: _box(n, _seed(cid, 8000 + n)), _path(n), 1)
    if kind == "c5i":                       # no equality rows: n IS the size the pivot loop sees
        cid = "c5i-n%d" % n
        return _add(cid, lambda: _c5(n, _seed(cid, 7500 + n))[:2] + (np.zeros(n, np.uint8), np.zeros(n), np.full(n, INF)), _path(n), 0)
    if kind == "boxi":
        cid = "boxi-n%d" % n
        return _add(cid, lambda: _box(n, _seed(cid, 8300 + n), eq_frac=0.0), _path(n), 1)
    if kind == "boxeq":                     # more than 1024 equality rows
        cid = "boxeq-n%d" % n
        return _add(cid, lambda: _box(n, _seed(cid, 8500 + n), eq_frac=0.9), _path(n), 1)
    if kind == "spec":
        target, box = kw["target"], kw["box"]
        cid = "spec%s%s-n%d" % ("1e3" if target == 1e3 else "5e6", "box" if box else "", n)
        return _add(cid, lambda: _spectrum(n, _seed(cid, 9000 + n + (1 if box else 0)), target, box), _path(n) + "-hard", 1 if box else 0)
    if kind == "pile":                      # 2x2x2: 96 rows, 2x2x3: 144 rows
        dims, cfm = kw["dims"], kw["cfm"]
        cid = "pile%d%d%d-cfm%g" % (dims + (cfm,))
        return _add(cid, lambda: _pile(dims, cfm), _path(n) + "-hard", 1)
    if kind == "lcpbox":                    # no equality rows: the box LCP entries
        cid = "lcpbox-n%d" % n
        return _add(cid, lambda: _box(n, _seed(cid, 8700 + n), eq_frac=0.0), "incr", 1)
    if kind == "lcpspec":
        target = kw["target"]
        cid = "lcpspec%s-n%d" % ("1e3" if target == 1e3 else "5e6", n)
        return _add(cid, lambda: _spectrum(n, _seed(cid, 9500 + n), target, True, eq_frac=0.0), "incr-hard", 1)
    if kind == "schur":
        nub = max(1, n // 4)
        cid = "schur-n%d" % n
        return _add(cid, lambda: _with_unbounded(_box(n, _seed(cid, 8900 + n), eq_frac=0.0), nub), "incr", 1, nub)
    raise KeyError(kind)


# Lcp::MixedConstraintsSolver under the reference's rule (use_bounds 0 / 1).  The equality rows are eliminated first
# and the pivot loop sees the inequality rows only: murty_small_kernel up to 112 of them, launch per pivot above with
# one (113, 128), two (129) and three-plus (193, 300) panels, ragged last panels.  "boxi" and "c5i" have no equality
# row, so their n is the loop's size exactly; "c5" and "box" at the same n put the Schur stage in front of it.
MIXED_REF_SIZES = (1, 2, 63, 64, 65, 111, 112, 113, 128, 129, 193, 300)
MIXED_REF = [_reg(k, n) for n in MIXED_REF_SIZES for k in ("c5", "boxi")]
MIXED_REF += [_reg("c5i", n) for n in (112, 113, 129)] + [_reg("box", n) for n in (65, 300)]
MIXED_REF += [_reg("spec", n, target=t, box=bx) for n, t, bx in ((64, 1e3, False), (112, 5e6, True), (129, 5e6, False), (193, 1e3, True))]
MIXED_REF += [_reg("pile", 96, dims=(2, 2, 2), cfm=c) for c in (1e-2, 1e-6)] + [_reg("pile", 144, dims=(2, 2, 3), cfm=c) for c in (1e-2, 1e-6)]
# the same entry under the block rule (use_bounds 2 / 3 = the case's flag + 2): 1023 .. 1025 the split upload and the
# 1024 limits of the cond and back-solve kernels; 1200 with more than 1024 equality rows; C5 itself at 2048.
MIXED_BLOCK = [_reg(k, n) for n in (113, 129, 300, 1023, 1024, 1025, 1100) for k in ("c5", "box")]
MIXED_BLOCK += [_reg("boxeq", 1200), _reg("boxi", 193), _reg("spec", 193, target=5e6, box=True), _reg("spec", 1100, target=1e3, box=False),
                _reg("pile", 144, dims=(2, 2, 3), cfm=1e-6)]
C5_ID = "c5-n2048"
_add(C5_ID, lambda: _c5(2048, 0), "panel", 0)      # the bench recipe, seed 0 (test_gpu_dense_block.test_config5_n2048)
MIXED_BLOCK.append(C5_ID)
# one ragged batch through egs_mixed_constraints_solve_batch: the three fused classes and the fall-through
BATCH_SIZES = (31, 32, 33, 63, 64, 65, 111, 112, 113)
BATCH = [_reg("box", n) for n in BATCH_SIZES] + [_reg("spec", n, target=1e3, box=True) for n in (33, 65, 113)] \
    + [_reg("spec", n, target=5e6, box=True) for n in (32, 64)]
# the box LCP entries (no equality rows): one wavefront in LDS up to 96 rows, four wavefronts above
LCP_SIZES = (24, 95, 96, 97)
LCP_BOX = [_reg("lcpbox", n) for n in LCP_SIZES + (200,)] + [_reg("lcpspec", 96, target=1e3), _reg("lcpspec", 97, target=5e6)]
LCP_SCHUR = [_reg("schur", n) for n in LCP_SIZES + (200,)]
LCP_BATCH = [c for c in LCP_BOX + LCP_SCHUR if not c.endswith("-n200")]
CASES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(cid):
    """The seeded case, built once per process and shared; callers must leave it unchanged."""
    build, cls, use_bounds, nub = _BUILDERS[cid]
    A, b, Ceq, lo, hi = build()
    for v in (A, b, Ceq, lo, hi):
        v.setflags(write=False)
    return Case(cid, cls, A, b, Ceq, lo, hi, use_bounds, nub)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The certified solution of a case, computed once per process."""
    c = case(cid)
    return solve(c.A, c.b, c.Ceq, c.lo, c.hi)
