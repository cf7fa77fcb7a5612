"""GPU (-m gpu): restitution through the world (egs_world_set_restitution).  A world's step is compared, bit for bit,
with an egs_problem fed the state that step read, its contact list and the per-constraint coefficients the world must
have filled in -- a problem whose rhs tests/test_gpu_restitution.py holds against the twin -- and the impact speed with
the 50-digit reference's value, -e v_z (tests/test_restitution_reference_cpu.py)."""
import numpy as np
import pytest

import restitution_reference as rr
from eggshell_amd import capi
from oracle import oracle as orc
from test_gpu_world_spheres import ball, make_world
from test_gpu_world_step_each import batch_world, bodies, ensemble, ensemble_view, same_bits, single_world
from test_gpu_world_warm import expected_start

pytestmark = pytest.mark.gpu

DT, ERP, U = 5e-3, 0.2, 2.0 ** -53


def problem_step(ctx, e, state, contacts, rest, vth, prm, mu=None, x0=None, dense=None):
    """egs_problem_step (or _step_dense) on that state and contact list with one coefficient per contact; lambda,
    velocities, rhs and the twin's decisions."""
    b0, b1, data = contacts
    m = len(b0)
    pr = capi.Problem(ctx, e["p"].shape[0], b0, b1)
    pr.set_state(*state, e["Minv"], e["f_ext"])
    kind = np.ones(m, np.int32)
    pr.set_constraints(kind, data)
    if rest is not None:
        pr.set_restitution(np.full(m, rest), vth)
    if mu is not None:
        pr.set_friction(np.full(m, mu))
    if x0 is not None:
        pr.set_start(capi.START_GIVEN, x0)
    if dense is not None:
        pr.step_dense(DT, ERP, dense, use_bounds=1)
    else:
        pr.step(DT, ERP, prm)
    lam, v6, rhs = pr.lambda_(), pr.velocity(), pr.blocks()[5]
    pr.close()
    J0, J1, _, _, _, err = orc.assemble(state[0], state[1], kind, b0, b1, data)
    case = dict(p=state[0], R=state[1], v=state[2], w=state[3], Minv=e["Minv"], f_ext=e["f_ext"], kind=kind, body0=b0,
                body1=b1, data=data, dt=DT, erp=ERP)
    want, what, _ = rr.twin_rhs(case, J0, J1, err, None if rest is None else np.full(m, rest), vth)
    assert same_bits(rhs.reshape(-1), want)
    return lam, v6, what


@pytest.mark.parametrize("mu", [None, 0.5], ids=["box", "pyramid"])
@pytest.mark.parametrize("e", [0.8, 0.0])
def test_sphere_dropped_centrally(ctx, e, mu):
    """A ball 1 mm into the plate falling at 2 m/s, one contact whose normal row stands alone (cfm 0: one sweep solves
    it).  v_z' is the reference's -e v_z (e = 0: the Baumgarte floor erp depth / dt) within dt times the reference's
    rhs tolerance plus the velocity update's few roundings, and the step is the problem's with the same coefficient."""
    depth, vz = 1e-3, -2.0
    b = ball(z=0.15 - depth)
    b["v"][0, 2] = vz
    mass = 1.0 / b["Minv"][0, 0]
    w, _ = make_world(ctx, [b])
    w.set_restitution(e, 0.0)
    if mu is not None:
        w.set_friction(mu)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=4, tol=0.0, cfm=0.0)
    state = w.bodies()
    w.step(DT, ERP, prm)
    contacts, lam = w.contacts(), w.lambda_()
    _, _, v, wv = w.bodies()
    w.close()
    assert len(contacts[0]) == 1
    plam, pv6, what = problem_step(ctx, b, state, contacts, e, 0.0, prm, mu=mu)
    assert what == ["bounce" if e > 0 else "floor"]
    assert same_bits(lam, plam) and same_bits(np.concatenate([v[0], wv[0]]), pv6.reshape(-1))
    ref_v, _, ref_tol, ref_what, ref_lam = rr.impact_reference(mass, vz, float(contacts[2][0, 6]), e, 0.0, DT, ERP)
    assert ref_what == what[0]
    bound = DT * float(ref_tol) + 16 * U * (abs(vz) + DT * (9.8 + float(ref_lam) / mass))
    print("e=%g: v_z' = %.17g, reference %.17g, bound %.3g" % (e, v[0, 2], float(ref_v), bound))
    assert abs(v[0, 2] - float(ref_v)) <= bound
    if e > 0:
        assert abs(float(ref_v) - (-e * vz)) < 1e-30


@pytest.mark.parametrize("mu", [None, 0.5], ids=["box", "pyramid"])
def test_flat_cube_dropped(ctx, mu):
    """A cube flat on the plate, four contacts, SOR to its sweep bound.  By symmetry the four normal multipliers are
    equal, (A + cfm I) lambda - rhs = w, and J v' = -e vn - dt (cfm lambda - w): the bound is dt (cfm max lambda +
    the reported residual) plus rounding."""
    e, vz, cfm = 0.7, -1.5, 0.01
    sc = bodies([[0.0, 0.0, 0.149]])
    sc["v"][0, 2] = vz
    b = ensemble(sc)
    w = single_world(ctx, b, capi.F64)
    w.set_restitution(e, 0.0)
    if mu is not None:
        w.set_friction(mu)
    prm = capi.params(method=capi.SOR, max_iters=60, tol=0.0, cfm=cfm)
    state = w.bodies()
    st = w.step(DT, ERP, prm, want_stats=True)
    contacts, lam = w.contacts(), w.lambda_()
    _, _, v, wv = w.bodies()
    w.close()
    assert len(contacts[0]) == 4
    plam, pv6, what = problem_step(ctx, b, state, contacts, e, 0.0, prm, mu=mu)
    assert what == ["bounce"] * 4
    assert same_bits(lam, plam) and same_bits(np.concatenate([v[0], wv[0]]), pv6.reshape(-1))
    bound = DT * (cfm * np.abs(lam).max() + st.residual) + 1e-12
    print("cube: v_z' = %.17g, -e v_z = %.17g, bound %.3g (residual %.3g)" % (v[0, 2], -e * vz, bound, st.residual))
    assert abs(v[0, 2] - (-e * vz)) <= bound


def falling(z, vz, n=1):
    sc = bodies([[0.0, 0.0, z + 0.299 * k] for k in range(n)])
    sc["v"][:, 2] = vz
    return ensemble(sc)


REST3 = [-1.0, 0.0, 0.8]


def three():
    return [falling(0.149, -1.0), falling(0.149, -1.5, n=2), falling(0.1485, -2.0)]


@pytest.mark.parametrize("entry", ["step", "step_each", "step_dense"])
def test_batched_world_ensembles_are_their_own_worlds(ctx, entry):
    """rest = [-1, 0, 0.8]: after every step each ensemble has the bits of a world holding only it with its own
    coefficient, and the -1 ensemble those of a world that never heard of restitution."""
    ens = three()
    vth = 0.1
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=15, tol=0.0, cfm=0.01)
    bw, off = batch_world(ctx, ens, capi.F64)
    bw.set_restitution(REST3, vth)
    singles = [single_world(ctx, e, capi.F64) for e in ens]
    for s, r in zip(singles[1:], REST3[1:]):
        s.set_restitution(r, vth)
    rates = [([DT, 0.0, 2e-3], [0.2, 0.2, 0.3]), ([DT, 2.5e-3, 2e-3], [0.2, 0.1, 0.3])]
    bounced = False
    for k in range(2):
        dt, erp = rates[k] if entry == "step_each" else ([DT] * 3, [ERP] * 3)
        if entry == "step":
            bw.step(DT, ERP, prm)
        elif entry == "step_each":
            bw.step_each(np.array(dt), np.array(erp), prm)
        else:
            bw.step_dense(DT, ERP, 0.01, use_bounds=1)
        info = bw.batch_info()
        for i, s in enumerate(singles):
            if dt[i] != 0.0:
                if entry == "step_dense":
                    s.step_dense(dt[i], erp[i], 0.01, use_bounds=1)
                else:
                    s.step(dt[i], erp[i], prm)
                body, con, lam = ensemble_view(bw, info, off, i)
                for a, b in zip(body, s.bodies()):
                    assert same_bits(a, b), (entry, k, i)
                assert same_bits(lam, s.lambda_()), (entry, k, i)
                if i == 2 and k == 0:
                    bounced = body[2][0, 2] > 1.0      # 0.8 x 2 m/s upwards
    assert bounced
    bw.close()
    for s in singles:
        s.close()


def test_replan_across_the_impact(ctx):
    """A cube that reaches the plate in its second step: the list grows from nothing to four contacts (a re-plan), and
    the new contacts carry the ensemble's coefficient."""
    e, vth = 0.6, 0.2
    b = falling(0.154, -2.0)
    w = single_world(ctx, b, capi.F64)
    w.set_restitution(e, vth)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20, tol=0.0, cfm=0.01)
    w.step(DT, ERP, prm)
    assert len(w.contacts()[0]) == 0
    replans = w.info()["replans"]
    state = w.bodies()
    w.step(DT, ERP, prm)
    contacts, lam = w.contacts(), w.lambda_()
    _, _, v, wv = w.bodies()
    assert len(contacts[0]) == 4 and w.info()["replans"] > replans
    w.close()
    plam, pv6, what = problem_step(ctx, b, state, contacts, e, vth, prm)
    assert what == ["bounce"] * 4
    assert same_bits(lam, plam) and same_bits(np.concatenate([v[0], wv[0]]), pv6.reshape(-1))
    assert v[0, 2] > 0.5 * e * abs(state[2][0, 2])


def test_warm_start_takes_its_history_after_the_restituted_solve(ctx):
    """Warm start on: the impact step runs from the default start and solves the restituted rows; the next step's x0
    is the matcher on that step's lambda."""
    e, vth = 0.1, 0.0
    b = falling(0.149, -2.0)
    w = single_world(ctx, b, capi.F64)
    w.set_warm_start(True, 0.01)
    w.set_restitution(e, vth)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20, tol=0.0, cfm=0.01)
    state = w.bodies()
    w.step(DT, ERP, prm)
    contacts, lam = w.contacts(), w.lambda_()
    x0, src = w.start()
    assert (src == -2).all() and len(contacts[0]) == 4
    plam, _, what = problem_step(ctx, b, state, contacts, e, vth, prm, x0=x0)
    assert what == ["bounce"] * 4 and same_bits(lam, plam)
    prev = (*contacts, lam)
    state = w.bodies()
    w.step(DT, ERP, prm)
    x0, src = w.start()
    want, wsrc = expected_start(prev, w)
    assert (src >= 0).all() and np.array_equal(src, wsrc) and same_bits(x0, want)
    plam, _, _ = problem_step(ctx, b, state, w.contacts(), e, vth, prm, x0=x0)
    assert same_bits(w.lambda_(), plam)
    w.close()
