"""The projected Jacobi / Gauss-Seidel / backward-SOR sweeps as mathematics, in mpmath at 50 digits: an INDEPENDENT
reference for lambda, the per-body accumulators, w = A x - rhs, the stopping rule's residual and the sweep count of a
tolerance-terminated run -- what oracle/pgs_fast.inc restates in fp64 / fp32 with per-body accumulators and the device
mirrors bit for bit.  Nothing here uses oracle/, carries an accumulator from sweep to sweep or follows pgs_fast.inc's
operation order: A is formed once as a sparse row list and every sweep is the scalar recurrence on its rows.

  A = J M^-1 J^T + cfm I                 rows coupled through shared bodies; a world side contributes nothing
  Jacobi        t = x_r + (b_r - (A x_old)_r) / A_rr
  Gauss-Seidel  t = x_r + (b_r - (A x)_r) / A_rr            rows 0 .. 3m-1, x the running iterate
  backward SOR  t = x_r + (b_r - (A x)_r) / (k A_rr)        rows 3m-1 .. 0, k = 1 / omega
  x_r <- t on an equality row, min(max(t, lo_r), hi_r) otherwise (+-inf bounds honoured)

(sparse_iterations.cc:72-226 with corrected semantics: no quirk Q1; start = rhs, quirk Q7, or a given x0.)  The
residual is GetResidualError with Q8: equality rows always count, a row on lo counts
with w < 0, a row on hi with w > 0, a row strictly inside always, a row outside the box not at all.  It is evaluated
at a GIVEN x, so the membership tests are exact comparisons of floating-point values, and w^2 is continuous at
w = 0: the function has no knife edge.  The clamp is Lipschitz-1, so lambda has none either and no case is excluded;
only the sweep count of a tolerance-terminated run has one (gap_condition).

Inputs are the exact fp64 values handed to the code under test; for an fp32 case (f32=True) every one of them -- M^-1,
J, rhs, bounds, start, cfm, omega -- rounded to fp32 first, because that is what the device holds.

Beside every value stands mag, the sum of the absolute values of the terms that form it: the quantity a rounding bound
scales with.  The bounds (u = 2^-53 or 2^-24):

  lambda, accumulators   |x - x_ref|_inf <= C u max(1, |x_ref|_inf)
  w                      |w_r - w_ref_r| <= C_w u mag_r          row by row, at the x of the code under test
  residual               |res - res_ref| <= C_r u |mag|_2        absolute, at the x of the code under test

The constants are not derived from operation counts: for each family class and precision the oracle's worst ratio was
measured on the CPU, multiplied by 8 and rounded up to a power of two (BOUNDS below; the measured ratios are in
DESIGN.md).  The factor 8 is the room a kernel that reorders a sum may use.

The seeded case generators at the end are shared by the CPU tests (oracle against this reference) and the GPU tests
(device against this reference), so both see identical inputs; they use the oracle's assembly to make INPUTS only."""
import functools
import math

import mpmath as mp
import numpy as np

DPS = 50
JACOBI, GAUSS_SEIDEL, SOR = 0, 1, 2
U = {False: 2.0 ** -53, True: 2.0 ** -24}


def held(a, f32):
    """The fp64 array as the code under test holds it: itself, or rounded to fp32."""
    a = np.asarray(a, dtype=np.float64)
    if f32:
        with np.errstate(over="ignore"):
            a = a.astype(np.float32).astype(np.float64)
    return a


def _v(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


class System:
    """A = J M^-1 J^T + cfm I as a sparse row list: cols[r] / vals[r] hold row r's non-zero pattern (diagonal
    included, cfm added), diag[r] = A_rr.  J and W are kept for accumulators()."""

    def __init__(self, n, m, f32, cols, vals, diag, J, W, body):
        self.n, self.m, self.f32 = n, m, f32
        self.cols, self.vals, self.diag = cols, vals, diag
        self.J, self.W, self.body = J, W, body

    def hold(self, a):
        return held(a, self.f32)

    def mag(self, x, rhs):
        """mag_r = sum_c |A_rc| |x_c| + |rhs_r| for a given x (floats or mpf)."""
        with mp.workdps(DPS):
            ax = [abs(t) for t in self._mp(x)]
            b = _v(self.hold(rhs))
            return [sum(abs(a) * ax[c] for c, a in zip(self.cols[r], self.vals[r])) + abs(b[r]) for r in range(3 * self.m)]

    def _mp(self, x):
        return list(x) if len(x) and isinstance(x[0], mp.mpf) else _v(x)

    def dense(self):
        with mp.workdps(DPS):
            A = mp.zeros(3 * self.m)
            for r in range(3 * self.m):
                for c, a in zip(self.cols[r], self.vals[r]):
                    A[r, c] = a
            return A


def system(s, cfm, f32=False):
    """The System of a flat constraint list s (attributes n, m, Minv [n][36], body0, body1, J0, J1 [m][18])."""
    with mp.workdps(DPS):
        n, m = int(s.n), int(s.m)
        Minv, J0, J1 = held(s.Minv, f32).reshape(n, 36), held(s.J0, f32).reshape(m, 18), held(s.J1, f32).reshape(m, 18)
        cfm = mp.mpf(float(held(cfm, f32)))
        body = (np.asarray(s.body0).astype(int), np.asarray(s.body1).astype(int))
        W = []
        for b in range(n):
            w = _v(Minv[b])
            W.append([[(c, w[6 * k + c]) for c in range(6) if w[6 * k + c] != 0] for k in range(6)])
        J = {}
        sides = [[] for _ in range(n)]
        for i in range(m):
            for side, blk in ((0, J0), (1, J1)):
                b = body[side][i]
                if b < 0:
                    continue
                j = _v(blk[i])
                J[(i, side)] = [j[0:6], j[6:12], j[12:18]]
                sides[b].append((i, side))
        rows = [dict() for _ in range(3 * m)]
        for b in range(n):
            # WJ[(i, side)][r][k] = (W_b J_r^T)_k; A[3i+r, 3j+q] += J_j,q . W_b J_i,r^T, once per unordered pair
            WJ = {key: [[sum(w * J[key][r][c] for c, w in W[b][k]) for k in range(6)] for r in range(3)] for key in sides[b]}
            for ia, ka in enumerate(sides[b]):
                for kb in sides[b][ia:]:
                    for r in range(3):
                        wj = WJ[ka][r]
                        for q in range(3):
                            jq = J[kb][q]
                            val = jq[0] * wj[0] + jq[1] * wj[1] + jq[2] * wj[2] + jq[3] * wj[3] + jq[4] * wj[4] + jq[5] * wj[5]
                            R, Q = 3 * ka[0] + r, 3 * kb[0] + q
                            rows[R][Q] = rows[R].get(Q, 0) + val
                            if ka != kb:
                                rows[Q][R] = rows[Q].get(R, 0) + val
        cols, vals, diag = [], [], []
        for r in range(3 * m):
            rows[r][r] = rows[r].get(r, mp.mpf(0)) + cfm
            cs = sorted(c for c in rows[r] if c == r or rows[r][c] != 0)      # exact zeros (orthogonal axes) are no coupling
            cols.append(tuple(cs)); vals.append(tuple(rows[r][c] for c in cs)); diag.append(rows[r][r])
        return System(n, m, f32, cols, vals, diag, J, W, body)


def sweeps(A, rhs, is_eq, lo, hi, method, omega, K, x0=None, history=False):
    """K sweeps from x0 (None: rhs).  Returns the iterate (list of mpf), or with history=True the K + 1 iterates
    x^0 .. x^K.  K = 0 returns the start."""
    with mp.workdps(DPS):
        R = 3 * A.m
        b = _v(A.hold(rhs))
        x = list(b) if x0 is None else _v(A.hold(x0))
        lo_, hi_ = A.hold(lo), A.hold(hi)
        box = [None if is_eq[r] else (None if lo_[r] == -np.inf else mp.mpf(float(lo_[r])),
                                      None if hi_[r] == np.inf else mp.mpf(float(hi_[r]))) for r in range(R)]
        k = 1 / mp.mpf(float(held(omega, A.f32))) if method == SOR else mp.mpf(1)
        den = [k * d for d in A.diag]
        cols, vals = A.cols, A.vals
        order = range(R - 1, -1, -1) if method == SOR else range(R)
        out = [list(x)]
        for _ in range(K):
            src = list(x) if method == JACOBI else x        # Jacobi reads the old iterate, the others the running one
            for r in order:
                ax = mp.mpf(0)
                for c, a in zip(cols[r], vals[r]):
                    ax += a * src[c]
                t = src[r] + (b[r] - ax) / den[r]
                if box[r] is not None:
                    l, h = box[r]
                    if l is not None and t < l:
                        t = l
                    elif h is not None and t > h:
                        t = h
                x[r] = t
            if history:
                out.append(list(x))
        return out if history else x


def wres(A, rhs, x):
    """(w, mag): w = A x - rhs row by row at the given x and mag_r = sum_c |A_rc| |x_c| + |rhs_r|."""
    with mp.workdps(DPS):
        xm = A._mp(x)
        b = _v(A.hold(rhs))
        w = [sum(a * xm[c] for c, a in zip(A.cols[r], A.vals[r])) - b[r] for r in range(3 * A.m)]
        return w, A.mag(xm, rhs)


def residual(A, rhs, x, is_eq, lo, hi, w=None):
    """(res, |mag|_2): the GetResidualError rule with Q8 at the given x (floats, or mpf iterates of sweeps())."""
    with mp.workdps(DPS):
        xm = A._mp(x)
        if w is None:
            w, mag = wres(A, rhs, xm)
        else:
            w, mag = w
        lo_, hi_ = A.hold(lo), A.hold(hi)
        e = qa = qb = qc = mp.mpf(0)
        for r in range(3 * A.m):
            if is_eq[r]:
                e += w[r] * w[r]
                continue
            l, h = mp.mpf(float(lo_[r])), mp.mpf(float(hi_[r]))
            if xm[r] == l and w[r] < 0:
                qa += w[r] * w[r]
            if xm[r] == h and w[r] > 0:
                qb += w[r] * w[r]
            if l < xm[r] < h:
                qc += w[r] * w[r]
        return mp.sqrt(e) + mp.sqrt(qa) + mp.sqrt(qb) + mp.sqrt(qc), mp.sqrt(sum(g * g for g in mag))


def accumulators(A, x):
    """(a, mag) [6n]: a_b = M_b^-1 sum_i J_ib^T x_i per body and the sums of absolute values behind each component."""
    with mp.workdps(DPS):
        xm = A._mp(x)
        g = [[mp.mpf(0)] * 6 for _ in range(A.n)]
        gm = [[mp.mpf(0)] * 6 for _ in range(A.n)]
        for (i, side), j in A.J.items():
            b = A.body[side][i]
            for r in range(3):
                for c in range(6):
                    t = j[r][c] * xm[3 * i + r]
                    g[b][c] = g[b][c] + t
                    gm[b][c] = gm[b][c] + abs(t)
        a, mag = [], []
        for b in range(A.n):
            for k in range(6):
                a.append(sum(w * g[b][c] for c, w in A.W[b][k]) + mp.mpf(0))
                mag.append(sum(abs(w) * gm[b][c] for c, w in A.W[b][k]) + mp.mpf(0))
        return a, mag


def velocity_after(case, J0, J1, lam):
    """v + dt (M^-1 f + M^-1 J^T lambda) [6n] as a model_reference.Checked (values and mag), for the blocks and the
    lambda given: the statement model_reference already makes."""
    import model_reference
    return model_reference.velocity_reference(case, J0, J1, lam)


def mixed_lcp_violation(A, rhs, x, is_eq, lo, hi):
    """check_mixed_solution's rule (sparse_iterations.cc:308-353) in mpmath: the largest violation of
    w = 0 (equality, strictly inside), w >= 0 (on lo), w <= 0 (on hi); inf for a row outside its box."""
    with mp.workdps(DPS):
        xm = A._mp(x)
        w, _ = wres(A, rhs, xm)
        lo_, hi_ = A.hold(lo), A.hold(hi)
        worst = mp.mpf(0)
        for r in range(3 * A.m):
            l, h = mp.mpf(float(lo_[r])), mp.mpf(float(hi_[r]))
            if is_eq[r] or l < xm[r] < h:
                v = abs(w[r])
            elif xm[r] == l:
                v = max(-w[r], 0)
            elif xm[r] == h:
                v = max(w[r], 0)
            else:
                return mp.inf
            worst = max(worst, v)
        return worst


# ---- errors of a result under test, in units of the bounds' scale -----------------------------------------------------
def _ratio(d, scale):
    return 0.0 if d == 0 else (math.inf if scale == 0 else float(d / scale))


def err_vector(got, ref, f32=False):
    """|got - ref|_inf / (u max(1, |ref|_inf)): the form of the lambda and accumulator bounds."""
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    assert g.shape[0] == len(ref)
    if not np.isfinite(g).all():
        return math.inf
    with mp.workdps(DPS):
        d = max([abs(mp.mpf(float(a)) - b) for a, b in zip(g, ref)] + [mp.mpf(0)])
        scale = max([abs(b) for b in ref] + [mp.mpf(1)])
        return _ratio(d, U[f32] * scale)


def err_rows(got, ref, mag, f32=False):
    """max_r |got_r - ref_r| / (u mag_r): the form of the w bound."""
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    assert g.shape[0] == len(ref)
    if not np.isfinite(g).all():
        return math.inf
    with mp.workdps(DPS):
        return max([_ratio(abs(mp.mpf(float(a)) - b), U[f32] * s) for a, b, s in zip(g, ref, mag)] + [0.0])


def err_scalar(got, ref, scale, f32=False):
    """|got - ref| / (u scale): the form of the residual bound, scale = |mag|_2."""
    if not math.isfinite(got):
        return math.inf
    with mp.workdps(DPS):
        return _ratio(abs(mp.mpf(float(got)) - ref), U[f32] * scale)


def measure(A, rhs, is_eq, lo, hi, x_ref, got_x, got_a=None, got_w=None, got_res=None):
    """The four error ratios of one result: lambda against x_ref; accumulators, w and the reported residual against
    the mathematics AT THE RESULT'S OWN x.  Missing parts are left out."""
    out = {"x": err_vector(got_x, x_ref, A.f32)}
    if got_a is not None:
        out["a"] = err_vector(got_a, accumulators(A, got_x)[0], A.f32)
    if got_w is not None or got_res is not None:
        wm = wres(A, rhs, got_x)
        if got_w is not None:
            out["w"] = err_rows(got_w, wm[0], wm[1], A.f32)
        if got_res is not None:
            res, scale = residual(A, rhs, got_x, is_eq, lo, hi, w=wm)
            out["r"] = err_scalar(got_res, res, scale, A.f32)
    return out


def gap_condition(residuals, tol, factor=1.01):
    """The sweep count K at which a run with this tol stops (the first k with res_k <= tol, the start included), and
    whether the reference's residuals keep clear of tol by `factor` at every sweep up to and including the crossing:
    res_k >= factor tol for k < K and res_K <= tol / factor.  (K, clear); K = None if tol is never reached."""
    with mp.workdps(DPS):
        tol = mp.mpf(float(tol))
        for k, r in enumerate(residuals):
            if r <= tol:
                return k, all(q >= factor * tol for q in residuals[:k]) and r * factor <= tol
        return None, False


# ---- bounds: C = 8 x the oracle's measured worst ratio, rounded up to a power of two ----------
# class -> precision (f32 flag) -> quantity: x lambda, a accumulators, w rows of A x - rhs, r reported residual.
# The singular pile has its own row so that it cannot loosen the others.
C_REGULAR_F64 = dict(x=256, a=512, w=256, r=64)
C_REGULAR_F32 = dict(x=128, a=512, w=128, r=64)
C_PILE_F64 = dict(x=1024, a=1024, w=2048, r=128)
C_PILE_F32 = dict(x=512, a=512, w=128, r=128)
C_SINGULAR_F64 = dict(x=4096, a=16384, w=4096, r=2048)
C_SINGULAR_F32 = dict(x=256, a=256, w=128, r=64)
BOUNDS = {("regular", False): C_REGULAR_F64, ("regular", True): C_REGULAR_F32,
          ("pile", False): C_PILE_F64, ("pile", True): C_PILE_F32,
          ("singular", False): C_SINGULAR_F64, ("singular", True): C_SINGULAR_F32}


# ---- seeded cases (identical inputs for the CPU and the GPU tests) ---------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
OMEGAS = (1.0, 1.5, 1.9)
CFMS = (0.0, 0.01, 0.3)
ALL = (JACOBI, GAUSS_SEIDEL, SOR)
DT, ERP = 5e-3, 0.2


class Case:
    """s: the flat system (fp64 arrays); rhs; cfm; omega; runs: {method: sweep counts}; x0 (None: rhs); cls: the
    family class of BOUNDS; scene: the scene dict behind a contact / joint case."""

    def __init__(self, s, rhs, cfm, omega, runs, cls, x0=None, scene=None):
        self.s, self.rhs, self.cfm, self.omega, self.runs, self.cls, self.x0, self.scene = s, rhs, cfm, omega, runs, cls, x0, scene


def _scene_case(sc, cfm, runs, cls):
    from helpers import ode_rhs_from_scene, system_from_scene
    s, err = system_from_scene(sc)
    rhs, _ = ode_rhs_from_scene(sc, s, err, DT, ERP)
    return Case(s, rhs, cfm, 1.5, runs, cls, scene=sc)


def joint_contact_scene():
    """A column of three boxes with two ball joints in the same island, listed between the contacts: body 0 to body 2
    and body 1 to a world anchor.  A list of mixed types is where quirk Q1 (not reproduced) would show."""
    from eggshell_amd import scenes
    sc = scenes.box_stack(1, 1, 3)
    kind, b0, b1, data = list(sc["kind"]), list(sc["body0"]), list(sc["body1"]), [row for row in sc["data"]]
    for at, (a, b, d) in ((2, (0, 2, [0.15, 0.15, 0.3, 0.15, 0.15, -0.298, 0.0])),
                          (7, (1, -1, [-0.15, 0.1, 0.0, -0.151, 0.1, 0.45, 0.0]))):
        kind.insert(at, scenes.JOINT_BALL); b0.insert(at, a); b1.insert(at, b); data.insert(at, np.array(d))
    sc.update(kind=np.array(kind, np.int32), body0=np.array(b0, np.int32), body1=np.array(b1, np.int32),
              data=np.array(data, np.float64).reshape(-1, 7))
    return sc


def oversize_island(rng):
    """One connected island of low degree (n = m / 2 bodies, the first n - 1 constraints a chain), grown in steps of 64
    constraints until the plan puts constraints on the cross-workgroup path (n_global > 0) at both tile sizes the
    solve may choose for it: an island of up to 512 constraints still gets one workgroup of its own."""
    from eggshell_amd import capi
    from helpers import random_system
    m = 256 + 64
    while True:
        state = rng.bit_generator.state
        s, rhs = random_system(rng, m // 2, m, connected=True)
        if all(capi.debug_plan(s.n, s.body0, s.body1, tile)["n_global"] > 0 for tile in (256, 512)):
            return s, rhs
        rng.bit_generator.state = state
        m += 64


def _concat(parts):
    """Independent systems as one list (body indices offset): one island each."""
    from oracle import oracle as orc
    off = np.concatenate([[0], np.cumsum([s.n for s, _ in parts])])
    cat = lambda f: np.concatenate([f(s, o) for (s, _), o in zip(parts, off)])
    s = orc.Sys(cat(lambda s, o: s.Minv), cat(lambda s, o: np.where(s.body0 >= 0, s.body0 + o, -1)),
                cat(lambda s, o: np.where(s.body1 >= 0, s.body1 + o, -1)), cat(lambda s, o: s.J0), cat(lambda s, o: s.J1),
                cat(lambda s, o: s.is_eq), cat(lambda s, o: s.lo), cat(lambda s, o: s.hi))
    return s, np.concatenate([rhs for _, rhs in parts])


def _isotropic(which):
    """Three islands of 120, 250 and 9 constraints on isotropic bodies: more than one tile, and none beyond the 256
    constraints up to which the solve keeps the 256-constraint tiles that the isotropic kernels need."""
    from helpers import random_system
    from test_gpu_solve_start import isotropic
    rng = np.random.default_rng(711)
    base, rhs = _concat([random_system(rng, n, m, world_frac=0.15) for n, m in ((25, 120), (40, 250), (5, 9))])
    if which == "linsym":      # the LINSYM form wants a body on side 1 of every constraint: world sides go to side 0
        from oracle import oracle as orc
        w1 = base.body1 < 0
        b0, b1, J0, J1 = base.body0.copy(), base.body1.copy(), base.J0.copy(), base.J1.copy()
        b0[w1], b1[w1], J0[w1], J1[w1] = -1, base.body0[w1], 0.0, base.J0[w1]
        base = orc.Sys(base.Minv, b0, b1, J0, J1, base.is_eq, base.lo, base.hi)
    return Case(isotropic(rng, base, which == "linsym"), rhs, 0.05, 1.5, {me: (4,) for me in ALL}, "regular")


def _random(i):
    from helpers import random_system
    m = SIZES[i]
    s, rhs = random_system(np.random.default_rng(700 + m), max(2, m // 3 + 2), m)
    # the eight sizes walk through eight of the nine (cfm, omega) pairs
    return Case(s, rhs, CFMS[i % 3], OMEGAS[(i + i // 3) % 3], {me: (4,) for me in ALL}, "regular")


def _grouped():
    from helpers import grouped_system, random_system
    rng = np.random.default_rng(712)
    base, _ = random_system(rng, 30, 40, world_frac=0.1)
    s, rhs = grouped_system(rng, base, None, 4)
    return Case(s, rhs, 0.05, 1.5, {me: (4,) for me in ALL}, "regular")


def _start():
    from helpers import random_system
    rng = np.random.default_rng(713)
    s, rhs = random_system(rng, 23, 65)
    return Case(s, rhs, 0.05, 1.5, {me: (4,) for me in ALL}, "regular", x0=rng.uniform(-1, 1, 3 * s.m))


def _oversize():
    s, rhs = oversize_island(np.random.default_rng(714))
    return Case(s, rhs, 0.05, 1.5, {me: (4,) for me in ALL}, "regular")


def _stack(nx, ny, nz, cfm, runs, cls):
    from eggshell_amd import scenes
    return _scene_case(scenes.box_stack(nx, ny, nz), cfm, runs, cls)


def _chain8():
    from eggshell_amd import scenes
    return _scene_case(scenes.chain(8), 0.0, {GAUSS_SEIDEL: (300,), SOR: (300,)}, "regular")


_BUILDERS = {"random-m%d" % m: functools.partial(_random, i) for i, m in enumerate(SIZES)}
_BUILDERS.update({
    "iso-plain": functools.partial(_isotropic, "plain"),
    "iso-linsym": functools.partial(_isotropic, "linsym"),
    "grouped4": _grouped,
    "start": _start,
    "chain8": _chain8,
    "joint-contact": lambda: _scene_case(joint_contact_scene(), 0.01, {GAUSS_SEIDEL: (100,), SOR: (100,)}, "pile"),
    "pile222": lambda: _stack(2, 2, 2, 0.01, {GAUSS_SEIDEL: (100, 500), SOR: (100,)}, "pile"),
    "pile223": lambda: _stack(2, 2, 3, 0.01, {GAUSS_SEIDEL: (100, 500), SOR: (100,)}, "pile"),
    "pile444": lambda: _stack(4, 4, 4, 0.01, {me: (8,) for me in ALL}, "pile"),
    "singular222": lambda: _stack(2, 2, 2, 0.0, {GAUSS_SEIDEL: (500,)}, "singular"),
    "oversize": _oversize,
})
CASE_IDS = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(cid):
    """The seeded case, built once per process and shared; callers must leave it unchanged."""
    return _BUILDERS[cid]()


@functools.lru_cache(maxsize=None)
def case_system(cid, f32=False):
    c = case(cid)
    return system(c.s, c.cfm, f32)


@functools.lru_cache(maxsize=None)
def case_iterates(cid, method, f32=False):
    """{K: x^K} of the case's sweep counts for this method, from one run of the reference."""
    c = case(cid)
    ks = c.runs[method]
    hist = sweeps(case_system(cid, f32), c.rhs, c.s.is_eq, c.s.lo, c.s.hi, method, c.omega, max(ks), c.x0, history=True)
    return {K: hist[K] for K in ks}


# method, tol, sweep limit: the 2 x 2 x 2 pile at cfm = 0 (at cfm = 0.01 it takes 4 301 sweeps to 1e-9) and Chain(8)
STOP_RUNS = {"singular222": (GAUSS_SEIDEL, 1e-9, 200), "chain8": (SOR, 1e-9, 100)}


@functools.lru_cache(maxsize=None)
def stop_reference(cid):
    """(K, clear, residuals) of the reference on a STOP_RUNS case: the sweep at which its residual first passes tol, and
    whether every residual up to there keeps clear of tol by a factor 1.01 (gap_condition)."""
    method, tol, limit = STOP_RUNS[cid]
    c = case(cid)
    A = case_system(cid)
    res = []
    for x in sweeps(A, c.rhs, c.s.is_eq, c.s.lo, c.s.hi, method, c.omega, limit, c.x0, history=True):
        res.append(residual(A, c.rhs, x, c.s.is_eq, c.s.lo, c.s.hi)[0])
        if res[-1] <= tol:
            break
    return gap_condition(res, tol) + (res,)
