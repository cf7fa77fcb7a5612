"""GPU (-m gpu): the friction pyramid through the C ABI's problem entries (egs_problem_set_friction): schedules that
run the same method give the same bits; friction set and cleared leaves no trace; a friction step takes the assembly
kernel and equals the unfused step bit for bit; the tilted-gravity cube slides and sticks as Coulomb says; a batch
problem's ensembles are bit-identical alone, in the batch and in the reversed batch; the dense step and a NaN
coefficient are refused; the same cube through the C++ adapter (Ensemble::SetFriction, friction_demo)."""
import json
import os
import subprocess

import numpy as np
import pytest

import friction_reference as fr
import model_reference as mref
import sweep_reference as ref
from eggshell_amd import capi
from test_gpu_solve_start import ENV, SCHEDULES, set_schedule

pytestmark = pytest.mark.gpu


def solve(ctx, c, mu, prm, precision=capi.F64):
    s = c.s
    pr = capi.Problem(ctx, s.n, s.body0, s.body1, precision)
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, c.rhs)
    if mu is not None:
        pr.set_friction(mu)
    st = pr.solve(prm)
    out = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), it=st.iterations, res=st.residual, sched=st.schedule)
    pr.close()
    assert st.status == capi.OK
    return out


def same_bits(p, q):
    return all(p[k].tobytes() == q[k].tobytes() for k in ("x", "a", "w")) and p["it"] == q["it"] and \
        np.float64(p["res"]).tobytes() == np.float64(q["res"]).tobytes()


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", ["random-m65", "random-m513", "grouped4", "oversize"])
def test_schedules_of_one_method_give_the_same_bits_with_friction(ctx, cid, precision, monkeypatch):
    """As without friction (test_gpu_solve_start.py): the kernels differ in how they order the list, not in what an
    update computes -- fixed sweeps and a tolerance-terminated run."""
    c = ref.case(cid)
    mu = fr.case_mu(cid)
    for method in (capi.GAUSS_SEIDEL, capi.SOR, capi.JACOBI):
        names = [n for n, (_, m) in SCHEDULES.items() if (m == capi.JACOBI) == (method == capi.JACOBI)]
        for prm in (capi.params(method=method, max_iters=4, tol=0.0, cfm=0.05, omega=c.omega),
                    capi.params(method=method, max_iters=40, tol=1e-4, cfm=0.5, omega=c.omega)):
            first = None
            for name in names:
                set_schedule(monkeypatch, name)
                got = solve(ctx, c, mu, prm, precision)
                assert got["sched"] & capi.SCHED_FRICTION
                first = first or got
                assert same_bits(first, got), (name, method, prm.tol)
            box = solve(ctx, c, None, prm, precision)
            assert box["x"].tobytes() != first["x"].tobytes()      # the pyramid is not the box


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_friction_set_and_cleared_is_a_problem_that_never_had_it(ctx, name, monkeypatch):
    method = set_schedule(monkeypatch, name)
    cid = "oversize" if name in ("quad_patches", "lane_patches", "all_global") else "random-m257"
    c, mu = ref.case(cid), fr.case_mu(cid)
    prm = capi.params(method=method, max_iters=4, tol=0.0, cfm=0.05, omega=c.omega)
    never = solve(ctx, c, None, prm)
    s = c.s
    pr = capi.Problem(ctx, s.n, s.body0, s.body1)
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, c.rhs)
    pr.set_friction(mu)
    on = pr.solve(prm)
    assert on.schedule == never["sched"] | capi.SCHED_FRICTION
    for off in (None, np.full(s.m, -1.0)):      # NULL and all negative both turn it off
        pr.set_friction(mu)
        pr.set_friction(off)
        st = pr.solve(prm)
        got = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), it=st.iterations, res=st.residual)
        assert st.schedule == never["sched"] and same_bits(never, got), name
    pr.close()


def _step(ctx, case, mu, prm, clear=False):
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"])
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    if mu is not None:
        pr.set_friction(mu)
    if clear:
        pr.set_friction(None)
    st = pr.step(case["dt"], case["erp"], prm, want_stats=True)
    out = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), v=pr.velocity(), it=st.iterations, res=st.residual,
               sched=st.schedule)
    pr.close()
    assert st.status == capi.OK
    return out


def _force_linsym(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EGS_QUAD", "0")
    monkeypatch.setenv("EGS_STEP", "1")
    monkeypatch.setenv("EGS_ISO", "2")
    monkeypatch.delenv("EGS_FUSED_ASSEMBLY", raising=False)
    monkeypatch.delenv("EGS_ISO_LINSYM", raising=False)


@pytest.mark.parametrize("method", [capi.GAUSS_SEIDEL, capi.SOR], ids=["gs", "sor"])
def test_friction_step_on_the_linsym_route_equals_the_unfused_step(ctx, method, monkeypatch):
    """The 2 x 2 x 2 stack forced onto the LINSYM timetable form: without friction the step fuses the assembly; with
    friction it does not, and equals EGS_FUSED_ASSEMBLY=0 bit for bit; friction set and cleared
    fuses again and gives the bits of a step that never had it."""
    _force_linsym(monkeypatch)
    case = mref.step_scene_b()
    prm = capi.params(method=method, max_iters=10, tol=0.0, cfm=0.01)
    mu = np.full(case["kind"].shape[0], 0.5)
    never = _step(ctx, case, None, prm)
    assert never["sched"] & capi.SCHED_FUSED_ASSEMBLY and never["sched"] & capi.SCHED_LINSYM
    assert not never["sched"] & capi.SCHED_FRICTION
    on = _step(ctx, case, mu, prm)
    assert on["sched"] & capi.SCHED_FRICTION and on["sched"] & capi.SCHED_LINSYM
    assert not on["sched"] & capi.SCHED_FUSED_ASSEMBLY
    cleared = _step(ctx, case, mu, prm, clear=True)
    assert cleared["sched"] == never["sched"] and same_bits(never, cleared) and cleared["v"].tobytes() == never["v"].tobytes()
    monkeypatch.setenv("EGS_FUSED_ASSEMBLY", "0")
    unfused = _step(ctx, case, mu, prm)
    assert unfused["sched"] == on["sched"]
    assert same_bits(on, unfused) and on["v"].tobytes() == unfused["v"].tobytes()
    assert on["x"].tobytes() != never["x"].tobytes()


@pytest.mark.parametrize("method", [capi.GAUSS_SEIDEL, capi.SOR], ids=["gs", "sor"])
@pytest.mark.parametrize("mu", [0.2, 0.8])
def test_tilted_gravity_cube_through_problem_step(ctx, mu, method):
    """One cube on the ground under gravity tilted by atan 0.5: it slides with v_x = dt g (sin - mu cos) at mu = 0.2
    (2.632299e-3) and sticks at mu = 0.8.  The device's velocity against the 50-digit reference's (500 sweeps of
    sweeps_pyramid on the blocks the step assembled) within the accumulator bound, and the reference's against the
    analytic value within CUBE_REF_DISTANCE.  The friction box gives neither."""
    case = fr.cube_case()
    cfm = 0.0
    prm = capi.params(method=method, max_iters=fr.CUBE_SWEEPS, tol=0.0, cfm=cfm, omega=1.5)
    mus = np.full(4, mu)
    pr = capi.Problem(ctx, 1, case["body0"], case["body1"])
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    pr.set_friction(mus)
    st = pr.step(case["dt"], case["erp"], prm, want_stats=True)
    lam, v6 = pr.lambda_(), pr.velocity()
    J0, J1, is_eq, lo, hi, rhs, _ = pr.blocks()
    pr.close()
    assert st.status == capi.OK and st.schedule & capi.SCHED_FRICTION
    import types
    blocks = types.SimpleNamespace(n=1, m=4, Minv=case["Minv"], body0=case["body0"], body1=case["body1"], J0=J0, J1=J1)
    A = ref.system(blocks, cfm)
    x_ref = fr.sweeps_pyramid(A, rhs, is_eq, lo, hi, mus, method, 1.5, fr.CUBE_SWEEPS)
    v_ref = ref.velocity_after(case, J0, J1, np.array([float(t) for t in x_ref]))
    want = fr.cube_velocity(mu)
    ref_dist = np.abs(v_ref.array() - want).max()
    ratio = ref.err_vector(v6, v_ref.val)
    bound = fr.BOUNDS[("singular", False)]["a"]      # four redundant contacts at cfm = 0: the singular class
    print("cube mu %.1f method %d: v = %s, |reference - analytic| = %.3g, device error %.3g u / %g" %
          (mu, method, v6, ref_dist, ratio, bound))
    assert ref_dist <= fr.CUBE_REF_DISTANCE, ref_dist
    assert ratio <= bound
    # the reference's box saturates at 1 per contact: 4 < m g sin(theta) = 4.387, so it neither holds nor is Coulomb's
    box = _step(ctx, case, None, prm)
    assert np.abs(box["v"] - want).max() > 1e-4


DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "friction_demo")


def demo(*args):
    if not os.path.exists(DEMO):
        pytest.fail("friction_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO, *args], check=True, capture_output=True, text=True, timeout=120)
    return [json.loads(line) for line in p.stdout.strip().splitlines()]


@pytest.mark.parametrize("method", [1, 2], ids=["gs", "sor"])
def test_tilted_gravity_cube_through_the_adapter(method):
    """Ensemble::SetFriction(COULOMB_PYRAMID, mu) and one Step of the adapter's device world (friction_demo): the cube
    slides at mu = 0.2 and sticks at mu = 0.8 with Coulomb's velocity for the normal force of that step (the corners
    start 1e-6 below the ground, which the step also pushes out); 1e-12 m/s is eight orders below v_x and far above the
    fp64 rounding of a converged 4-contact solve.  The default model, the reference's box, gives another velocity."""
    for mu in (0.2, 0.8):
        out = demo(str(mu), str(method))[-1]
        print(out)
        assert out["contacts"] == 4
        want = np.array([out["coulomb_vx"], 0.0, out["coulomb_vz"], 0.0, 0.0, 0.0])
        assert np.abs(np.array(out["v"] + out["w"]) - want).max() <= 1e-12
        assert (out["coulomb_vx"] > 2e-3) == (mu == 0.2)
    box = demo("--box", "0.2", str(method))[-1]
    assert box["contacts"] == 4 and abs(box["v"][0] - box["coulomb_vx"]) > 1e-4


def test_the_adapter_refuses_the_models_it_does_not_build():
    out = demo("--refuse")
    assert [o["case"] for o in out] == ["no_friction", "infinite", "negative_mu", "dense"]
    assert [o["refused"] for o in out] == [capi.ERR_UNSUPPORTED, capi.ERR_UNSUPPORTED, capi.ERR_INVALID, capi.ERR_UNSUPPORTED]


def test_batch_problem_ensembles_are_bit_identical_alone_and_in_any_order(ctx):
    """Three ensembles (a random system each, its own mu) in one batch problem, in the reversed batch and alone: the
    same lambda, accumulators and w, bit for bit -- fixed sweeps, and each ensemble alone stopping on its own tol run."""
    cids = ["random-m63", "random-m65", "grouped4"]
    cs = [ref.case(cid) for cid in cids]
    mus = [fr.case_mu(cid) for cid in cids]
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=6, tol=0.0, cfm=0.05)

    def run(order):
        pr, boff, coff = capi.Problem.batch(ctx, [cs[k].s.n for k in order], [cs[k].s.m for k in order],
                                            np.concatenate([cs[k].s.body0 for k in order]),
                                            np.concatenate([cs[k].s.body1 for k in order]))
        cat = lambda f: np.concatenate([np.asarray(f(cs[k])).reshape(-1) for k in order])
        pr.set_blocks(cat(lambda c: c.s.Minv), cat(lambda c: c.s.J0), cat(lambda c: c.s.J1), cat(lambda c: c.s.is_eq),
                      cat(lambda c: c.s.lo), cat(lambda c: c.s.hi), cat(lambda c: c.rhs))
        pr.set_friction(np.concatenate([mus[k] for k in order]))
        st = pr.solve(prm)
        assert st.status == capi.OK and st.schedule & capi.SCHED_FRICTION
        x, a, w = pr.lambda_(), pr.accumulators().reshape(-1), pr.wres()
        pr.close()
        return {k: (x[3 * coff[i]:3 * coff[i + 1]], a[6 * boff[i]:6 * boff[i + 1]], w[3 * coff[i]:3 * coff[i + 1]])
                for i, k in enumerate(order)}

    fwd, rev = run([0, 1, 2]), run([2, 1, 0])
    for k in range(3):
        alone = solve(ctx, cs[k], mus[k], prm)
        for got in (fwd[k], rev[k]):
            assert got[0].tobytes() == alone["x"].tobytes(), k
            assert got[1].tobytes() == alone["a"].reshape(-1).tobytes(), k
            assert got[2].tobytes() == alone["w"].tobytes(), k


def test_dense_step_and_nan_are_refused(ctx):
    case = mref.step_scene_b()
    m = case["kind"].shape[0]
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"])
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    mu = np.full(m, -1.0); mu[3] = 0.0
    pr.set_friction(mu)
    with pytest.raises(capi.EgsError) as e:
        pr.step_dense(case["dt"], case["erp"], 0.01)
    assert e.value.status == capi.ERR_UNSUPPORTED
    bad = mu.copy(); bad[0] = np.nan
    with pytest.raises(capi.EgsError) as e:
        pr.set_friction(bad)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.EgsError) as e:      # the NaN changed nothing: friction is still on
        pr.step_dense(case["dt"], case["erp"], 0.01)
    assert e.value.status == capi.ERR_UNSUPPORTED
    pr.set_friction(None)
    pr.step_dense(case["dt"], case["erp"], 0.01)      # off: the dense step runs again
    pr.close()
