"""The Coulomb friction pyramid on the dense direct solvers as mathematics (DESIGN.md sections 4g and 7e): the reference
of egs_mixed_friction_solve_batch and of the dense steps under egs_problem_set_dense_friction.

A pyramid problem is a mixed box LCP (A, b, C, lo, hi) plus, per row r, normal_row[r] (-1: a plain row) and mu[r] >= 0.
A row with normal_row[r] = f >= 0 is a PYRAMID row: an inequality row whatever C[r] says, f a plain inequality row.  The
solve is the fixed-point (Tresca) iteration on the bounds beta:

  start    beta^0 = 0
  solve k  the box LCP P(beta^k): plain rows as stored; a pyramid row with beta^k_r > 0 bounded by [-beta^k_r, beta^k_r];
           one with beta^k_r = 0 PINNED (x_r = 0 exactly, no condition on w_r)
  update   beta^{k+1}_r = x_f > 0 ? fl(mu_r x_f) : 0, from x^k (one fp64 rounding)
  change   delta_k = max_r |beta^{k+1}_r - beta^k_r| / max(1, max_r beta^{k+1}_r)
  stop     at the first k with delta_k <= tol, else after max_outer solves
  result   x = x^k, w = A x^k - b (0 on equality rows), beta = beta^k, outer = k + 1, change = delta_k

reference()  every P(beta^k), with its pinned rows removed, solved by lcp_reference.find_set + certify: with A positive
             definite each has exactly one solution and the certificate is strict, so the iterate is the iteration's,
             whoever proposed the sets.  beta comes from the certified x rounded to fp64.
port()       the same loop in plain numpy fp64: np.linalg.solve on the certified sets, beta from its own x.  It stands
             for "an fp64 implementation" when the bounds are made; it takes no part in a reference value.

Bounds (made as in section 7d; u = 2^-53, kappa = kappa_2 of the FINAL certified set):

  |x - x_ref|_inf <= C kappa u max(1, |x_ref|_inf)

C = 8 x the port's worst measured ratio over the class's cases, rounded up to a power of two.  Measured ratios of the
port (this file's cases, the worst of each class; test_dense_friction_reference_cpu prints every case's):

  random   rnd-n3 0.0623, n6 0.765, n30 0.982, n33 0.794, n63 1.73, n66 1.84, n111 1.69, n114 1.41
           worst 1.84  -> 8 x 1.84 = 14.7  -> C = 16
  scene    cube-mu0.2 0.164, cube-mu0.8 0.0598, pile222-mu0.2 0.126, pile222-mu0.5 0.0264, pile223-mu0.22 0.114,
           joint-contact-mu0.5 0.158
           worst 0.164 -> 8 x 0.164 = 1.31 -> C = 2

Device figures never set a constant.

The seeded cases at the end are shared by the CPU test and the GPU tests, so both see identical inputs."""
import functools

import numpy as np

import lcp_reference as lcp

U = lcp.U
TOL, MAX_OUTER = 1e-10, 32
GAP = 4.0            # delta keeps this factor away from tol at the stopping solve and before it
C_RANDOM, C_SCENE = 16.0, 2.0
BOUNDS = {"random": C_RANDOM, "scene": C_SCENE}


class Result:
    """x, w, beta [n]; outer, change, converged; deltas: delta_0 .. delta_{outer-1}; pinned [n] (bool) at the returned
    solve; refs: lcp_reference.Reference of every solve (the reference only); keep: the rows of the last solve."""


def _sub_problem(A, b, Ceq, lo, hi, nrow, beta):
    pyr = nrow >= 0
    keep = np.flatnonzero(~pyr | (beta > 0))
    C2 = np.where(pyr, 0, Ceq)[keep].astype(np.uint8)
    lo2 = np.where(pyr, -beta, lo)[keep]
    hi2 = np.where(pyr, beta, hi)[keep]
    return keep, A[np.ix_(keep, keep)], b[keep], C2, lo2, hi2


def _next_beta(x, nrow, mu):
    pyr = nrow >= 0
    xf = x[np.where(pyr, nrow, 0)]
    return np.where(pyr & (xf > 0), np.float64(mu) * xf, 0.0)


def _change(new, old):
    return float(np.abs(new - old).max(initial=0.0) / max(1.0, new.max(initial=0.0)))


def _iterate(A, b, Ceq, lo, hi, nrow, mu, tol, max_outer, inner):
    A, b, lo, hi, mu = (np.asarray(v, dtype=np.float64) for v in (A, b, lo, hi, mu))
    nrow = np.asarray(nrow, dtype=np.int64)
    Ceq = np.asarray(Ceq).astype(np.uint8)
    n = b.shape[0]
    beta = np.zeros(n)
    res = Result()
    res.deltas, res.refs = [], []
    for k in range(max_outer):
        keep, A2, b2, C2, lo2, hi2 = _sub_problem(A, b, Ceq, lo, hi, nrow, beta)
        x2, ref = inner(k, A2, b2, C2, lo2, hi2)
        res.refs.append(ref)
        x = np.zeros(n)
        x[keep] = x2
        new = _next_beta(x, nrow, mu)
        res.deltas.append(_change(new, beta))
        if res.deltas[-1] <= tol:
            break
        if k + 1 < max_outer:
            beta = new
    w = A @ x - b
    w[(Ceq != 0) & (nrow < 0)] = 0.0
    res.x, res.w, res.beta, res.keep = x, w, beta, keep
    res.outer, res.change = len(res.deltas), res.deltas[-1]
    res.converged = res.change <= tol
    res.pinned = (nrow >= 0) & (beta == 0)
    return res


def reference(A, b, Ceq, lo, hi, nrow, mu, tol=TOL, max_outer=MAX_OUTER):
    """The certified iteration.  Raises lcp_reference.NotCertified if a solve's certificate is not strict."""
    def inner(k, A2, b2, C2, lo2, hi2):
        ref = lcp.certify(A2, b2, C2, lo2, hi2, lcp.find_set(A2, b2, C2, lo2, hi2))
        return ref.x, ref
    return _iterate(A, b, Ceq, lo, hi, nrow, mu, tol, max_outer, inner)


def port(A, b, Ceq, lo, hi, nrow, mu, ref, tol=TOL, max_outer=MAX_OUTER):
    """Plain numpy fp64 on the certified sets of `ref` (a reference() result; solves beyond its last reuse find_set)."""
    def inner(k, A2, b2, C2, lo2, hi2):
        state = ref.refs[k].state if k < len(ref.refs) and ref.refs[k].state.shape[0] == b2.shape[0] else lcp.find_set(A2, b2, C2, lo2, hi2)
        x, _ = lcp._solve_state(A2, b2, lo2, hi2, np.asarray(state))
        return x, None
    return _iterate(A, b, Ceq, lo, hi, nrow, mu, tol, max_outer, inner)


def x_ratio(ref, x):
    """|x - x_ref|_inf / (kappa u max(1, |x_ref|_inf)) with kappa of the final certified set; the rows outside the last
    solve (pinned) count with x_ref = 0."""
    last = ref.refs[-1]
    full = [np.zeros(ref.x.shape[0]) for _ in last.parts]
    for f, p in zip(full, last.parts):
        f[ref.keep] = p
    err = np.abs(lcp.error_units(x, full)).max(initial=0.0)
    return float(err / (last.kappa * U * max(1.0, np.abs(ref.x).max(initial=0.0))))


def complementarity(A, b, Ceq, nrow, mu, lo, hi, res, tol):
    """What fails of the pyramid's conditions at res.beta, as a list: w = 0 strictly inside, its sign at +-beta,
    |beta_r - mu_r x_f| <= 2 tol max(1, max beta).  The scale of "w = 0" is u mag_r times the final set's kappa."""
    A, b, mu = (np.asarray(v, dtype=np.float64) for v in (A, b, mu))
    nrow = np.asarray(nrow)
    x, w, beta = res.x, res.w, res.beta
    mag = np.abs(A) @ np.abs(x) + np.abs(b)
    kappa = res.refs[-1].kappa if res.refs[-1] is not None else 1.0
    bad = []
    for r in np.flatnonzero(nrow >= 0):
        if beta[r] == 0:
            if x[r] != 0:
                bad.append(("pinned", int(r)))
            continue
        if abs(x[r]) < beta[r]:
            if not abs(w[r]) <= 64 * kappa * U * mag[r]:
                bad.append(("inside", int(r), float(w[r])))
        elif x[r] == beta[r]:
            if not w[r] <= 0:
                bad.append(("at +beta", int(r), float(w[r])))
        elif x[r] == -beta[r]:
            if not w[r] >= 0:
                bad.append(("at -beta", int(r), float(w[r])))
        else:
            bad.append(("outside", int(r)))
        xf = max(x[nrow[r]], 0.0)
        if not abs(beta[r] - mu[r] * xf) <= 2 * tol * max(1.0, beta.max()):
            bad.append(("beta", int(r)))
    return bad


def gap_ok(deltas, tol=TOL, factor=GAP):
    """sweep_reference.gap_condition on the changes: (stopping solve, clear of tol by `factor` on both sides)."""
    from sweep_reference import gap_condition
    return gap_condition(deltas, tol, factor)


# ---- seeded cases --------------------------------------------------------------------------------------------------------
class Case:
    """A, b, Ceq, lo, hi, nrow (int32), mu: the problem as handed to the code under test; cls: the class of BOUNDS."""

    def __init__(self, cid, cls, A, b, Ceq, lo, hi, nrow, mu, extra=None):
        self.id, self.cls, self.A, self.b, self.Ceq, self.lo, self.hi, self.nrow, self.mu = cid, cls, A, b, Ceq, lo, hi, nrow, mu
        self.n = b.shape[0]
        self.extra = extra or {}


RANDOM_SIZES = (3, 6, 30, 33, 63, 66, 111, 114)
MU_DRAW = (0.1, 0.3, 0.7)
# the replacement offset of a seed that missed the conditions when the list was written (the gap to tol on both sides of
# the stopping solve, more than one solve, and from n = 30 on rows pinned, at +beta, at -beta and strictly inside)
SEED_SHIFT = {"rnd-n3": 4, "rnd-n6": 1, "rnd-n30": 15, "rnd-n33": 7, "rnd-n63": 7, "rnd-n66": 1, "rnd-n111": 120, "rnd-n114": 33}


def _random(n, seed):
    """SPD with kappa_2 <= 1e4 (lcp_reference._box's recipe: M^T M / n + I / 2), rows in triples (t, t, n): n // 12
    equality triples in front, then contact triples of which about a quarter are plain boxes."""
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    A = M.T @ M / n + 0.5 * np.eye(n)
    b = rng.uniform(-3, 3, n)
    t = n // 3
    neq = t // 4
    Ceq = np.zeros(n, np.uint8)
    lo, hi = np.zeros(n), np.full(n, lcp.INF)
    nrow = np.full(n, -1, np.int32)
    mu = np.zeros(n)
    for c in range(t):
        r = 3 * c
        if c < neq:
            Ceq[r:r + 3] = 1
        elif c > neq and rng.uniform() < 0.25:                     # (the first contact triple is always a pyramid)
            lo[r:r + 2], hi[r:r + 2] = -0.2, 0.3
        else:
            nrow[r:r + 2] = r + 2
            mu[r:r + 2] = MU_DRAW[rng.integers(0, 3)]
    return Case("rnd-n%d" % n, "random", A, b, Ceq, lo, hi, nrow, mu)


PILE_PUSH = (0.3, 0.1, 0.0)
SCENE_CFM = 0.01


def _scene(cid, sc, mu_c, dt, erp, f_ext=None, Minv=None):
    """A = J M^-1 J^T + 0.01 I from helpers.dense_numpy with its true ode_rhs; the upper triangle mirrored from the
    lower (the factorisations read one triangle, the certificate wants one matrix).  mu_c: per constraint, < 0 = plain."""
    from helpers import dense_numpy, system_from_scene
    from oracle import oracle as orc
    s, err = system_from_scene(sc)
    if Minv is not None:
        s = orc.Sys(Minv, s.body0, s.body1, s.J0, s.J1, s.is_eq, s.lo, s.hi)
    if f_ext is None:
        f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    rhs = orc.ode_rhs(sc["v"], sc["w"], s.Minv, f_ext, s.body0, s.body1, s.J0, s.J1, err, dt, erp)
    A = dense_numpy(s, SCENE_CFM)[0]
    A = np.tril(A) + np.tril(A, -1).T
    m = s.m
    mu_c = np.broadcast_to(np.asarray(mu_c, dtype=np.float64), (m,)).copy()
    mu_c[np.asarray(sc["kind"]) != 1] = -1.0                       # joints stay as stored
    nrow = np.full(3 * m, -1, np.int32)
    mu = np.zeros(3 * m)
    for c in np.flatnonzero(mu_c >= 0):
        nrow[3 * c:3 * c + 2] = 3 * c + 2
        mu[3 * c:3 * c + 2] = mu_c[c]
    extra = dict(scene=sc, sys=s, mu_c=mu_c, dt=dt, erp=erp, f_ext=f_ext)
    return Case(cid, "scene", A, np.asarray(rhs, dtype=np.float64), s.is_eq.astype(np.uint8), s.lo.copy(), s.hi.copy(), nrow, mu, extra)


def _cube(mu):
    import friction_reference as fr
    c = fr.cube_case()
    sc = dict(c)
    return _scene("cube-mu%g" % mu, sc, mu, c["dt"], c["erp"], f_ext=c["f_ext"], Minv=c["Minv"])


def _pile(dims, mu):
    from eggshell_amd import scenes
    sc = scenes.box_stack(*dims)
    sc["v"] = sc["v"] + np.asarray(PILE_PUSH)
    return _scene("pile%d%d%d-mu%g" % (dims + (mu,)), sc, mu, lcp.PILE_DT, lcp.PILE_ERP)


def _joint_contact(mu):
    from sweep_reference import joint_contact_scene
    return _scene("joint-contact-mu%g" % mu, joint_contact_scene(), mu, lcp.PILE_DT, lcp.PILE_ERP)


_BUILDERS = {}
for _n in RANDOM_SIZES:
    _BUILDERS["rnd-n%d" % _n] = (lambda n=_n: _random(n, 12000 + n + 100000 * SEED_SHIFT.get("rnd-n%d" % n, 0)))
RANDOM = list(_BUILDERS)
_BUILDERS["cube-mu0.2"] = lambda: _cube(0.2)
_BUILDERS["cube-mu0.8"] = lambda: _cube(0.8)
_BUILDERS["pile222-mu0.2"] = lambda: _pile((2, 2, 2), 0.2)
_BUILDERS["pile222-mu0.5"] = lambda: _pile((2, 2, 2), 0.5)
# (mu nudged from 0.2: there delta_5 = 2.1e-10 stands within the factor 4 of tol)
_BUILDERS["pile223-mu0.22"] = lambda: _pile((2, 2, 3), 0.22)
_BUILDERS["joint-contact-mu0.5"] = lambda: _joint_contact(0.5)
SCENES = [c for c in _BUILDERS if c not in RANDOM]
CASES = RANDOM + SCENES
NOT_CONVERGED = "pile222-mu0.5"      # with max_outer = 2: converged = 0, outer = 2


@functools.lru_cache(maxsize=None)
def case(cid):
    """The seeded case, built once per process and shared; callers must leave it unchanged."""
    c = _BUILDERS[cid]()
    for v in (c.A, c.b, c.Ceq, c.lo, c.hi, c.nrow, c.mu):
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def solved(cid, max_outer=MAX_OUTER):
    """The certified iteration of a case, computed once per process."""
    c = case(cid)
    return reference(c.A, c.b, c.Ceq, c.lo, c.hi, c.nrow, c.mu, TOL, max_outer)


def bound(c, ref):
    """The bound on |x - x_ref|_inf for a result on case c."""
    return BOUNDS[c.cls] * ref.refs[-1].kappa * U * max(1.0, float(np.abs(ref.x).max(initial=0.0)))


def velocity(c, lam):
    """The velocities [n][6] after the step of a scene case with the multipliers lam (oracle.velocity_update)."""
    from oracle import oracle as orc
    e = c.extra
    sc, s = e["scene"], e["sys"]
    return orc.velocity_update(sc["v"], sc["w"], s.Minv, e["f_ext"], s.body0, s.body1, s.J0, s.J1, lam, e["dt"])


# |v - cube_velocity(mu)|_inf of the cube after the step with the REFERENCE's lambda: not zero, cfm = 0.01 softens the
# contact (recorded from test_dense_friction_reference_cpu.test_cube_velocity_distance)
CUBE_DISTANCE = {0.2: 2.9126288251772134e-05, 0.8: 7.259986766375477e-05}
