"""GPU (-m gpu): the device's projected sweeps -- every kernel a sweep can run on (test_gpu_solve_start.SCHEDULES), fp64
and fp32 -- against the 50-digit reference of tests/sweep_reference.py, on the seeded cases and within the bounds that
test_sweep_reference_cpu.py applies to the oracle: lambda against the reference's sweeps; accumulators(), wres() and the
reported residual against the mathematics at the device's own lambda; the sweep count of the tolerance-terminated
runs; one whole step of the 2 x 2 x 2 stack through the fused LINSYM launch.  Every test prints error / bound per
schedule (pytest -s).  Measured on MI355X: DESIGN.md section 6c."""
import types

import pytest

import model_reference as mref
import sweep_reference as ref
from eggshell_amd import capi
from test_gpu_solve_start import ENV, SCHEDULES, set_schedule

pytestmark = pytest.mark.gpu

PRECISION = {False: capi.F64, True: capi.F32}
ISO_CASES = ("iso-plain", "iso-linsym")
OVERSIZE_FLAGS = {"quad_patches": capi.SCHED_QUAD_PATCHES, "lane_patches": capi.SCHED_LANE_PATCHES,
                  "all_global": capi.SCHED_ALL_GLOBAL}
_measured = {}


def solve(ctx, c, method, K, f32, tol=0.0):
    s = c.s
    pr = capi.Problem(ctx, s.n, s.body0, s.body1, PRECISION[f32])
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, c.rhs)
    if c.x0 is not None:
        pr.set_start(capi.START_GIVEN, c.x0)
    st = pr.solve(capi.params(method=method, max_iters=K, tol=tol, cfm=c.cfm, omega=c.omega))
    out = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), res=st.residual, st=st)
    pr.close()
    assert st.status == capi.OK
    return out


def ratios(cid, method, K, f32, got):
    """The four error ratios of one device result; a result whose bits were measured already (the schedules are held
    bit-equal by the other tests, so most are) is not measured again."""
    key = (cid, method, K, f32, got["x"].tobytes(), got["a"].tobytes(), got["w"].tobytes(), got["res"])
    if key not in _measured:
        c = ref.case(cid)
        _measured[key] = ref.measure(ref.case_system(cid, f32), c.rhs, c.s.is_eq, c.s.lo, c.s.hi,
                                     ref.case_iterates(cid, method, f32)[K], got["x"], got["a"], got["w"], got["res"])
    return _measured[key]


def schedules_of(cid, monkeypatch):
    """(name, method) of every schedule whose method the case runs, with the schedule's switches set; the isotropic
    cases force the isotropic kernels on the two schedules that have them."""
    c = ref.case(cid)
    for name in SCHEDULES:
        method = set_schedule(monkeypatch, name)
        if method not in c.runs:
            continue
        if cid in ISO_CASES and name in ("tile", "timetable"):
            monkeypatch.setenv("EGS_ISO", "2")
        yield name, method


def check_case(ctx, cid, f32, monkeypatch):
    c = ref.case(cid)
    bound = ref.BOUNDS[(c.cls, f32)]
    bad, worst = [], dict(x=0.0, a=0.0, w=0.0, r=0.0)
    for name, method in schedules_of(cid, monkeypatch):
        for K in c.runs[method]:
            got = solve(ctx, c, method, K, f32)
            st = got["st"]
            assert st.iterations == K
            if cid in ISO_CASES and name in ("tile", "timetable"):
                assert st.schedule & capi.SCHED_ISO, name
                if name == "timetable" and not f32:      # the LINSYM form is fp64 only
                    assert bool(st.schedule & capi.SCHED_LINSYM) == (cid == "iso-linsym")
            if cid == "oversize" and name in OVERSIZE_FLAGS:
                assert st.n_global > 0 and st.schedule & OVERSIZE_FLAGS[name], (name, st.n_global, st.schedule)
            r = ratios(cid, method, K, f32, got)
            print("%s %s %-19s K %3d sched %#6x: " % (cid, "f32" if f32 else "f64", name, K, st.schedule) +
                  " ".join("%s=%.3g/%g" % (q, v, bound[q]) for q, v in sorted(r.items())))
            bad += [(name, K, q, v) for q, v in r.items() if not v <= bound[q]]
            worst = {q: max(worst[q], v) for q, v in r.items()}
    print("%s %s (%s) worst: " % (cid, "f32" if f32 else "f64", c.cls) + " ".join("%s=%.3g" % kv for kv in sorted(worst.items())))
    assert not bad, bad


REGULAR = ["random-m%d" % m for m in ref.SIZES] + ["iso-plain", "iso-linsym", "grouped4", "start", "chain8", "oversize"]
PILES = ["joint-contact", "pile222", "pile223", "pile444", "singular222"]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", REGULAR)
def test_regular_cases_on_every_schedule(ctx, cid, f32, monkeypatch):
    """K = 4 sweeps at m = 1, 63, 64, 65, 255, 256, 257, 513 (every method, omega 1.0 / 1.5 / 1.9, cfm 0 / 0.01 / 0.3, mixed
    row types, +-inf bounds, world sides), the plain isotropic and the LINSYM form, runs of four, a start other than
    rhs, 300 sweeps of Chain(8) at cfm 0, and one oversize island (n_global > 0; the patch and all-global flags are
    asserted)."""
    check_case(ctx, cid, f32, monkeypatch)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", PILES)
def test_contact_piles_on_every_schedule(ctx, cid, f32, monkeypatch):
    """Contact scenes with their true right-hand side: a joint + contact island and the 2 x 2 x 2 and 2 x 2 x 3 piles at
    100 and 500 sweeps, the 4 x 4 x 4 pile at 8 sweeps (more than 100 rows on a bound), and the singular pile (2 x 2 x 2,
    cfm = 0, 500 sweeps), which has constants of its own."""
    check_case(ctx, cid, f32, monkeypatch)


@pytest.mark.parametrize("cid", list(ref.STOP_RUNS))
def test_a_tolerance_terminated_run_stops_where_the_reference_stops(ctx, cid, monkeypatch):
    method, tol, limit = ref.STOP_RUNS[cid]
    K, clear, _ = ref.stop_reference(cid)
    assert K is not None and clear
    c = ref.case(cid)
    for name in SCHEDULES:
        if set_schedule(monkeypatch, name) != method:
            continue
        got = solve(ctx, c, method, limit, False, tol=tol)
        print("%s %-19s stops after %d sweeps (reference %d), residual %.3g" % (cid, name, got["st"].iterations, K, got["res"]))
        assert got["st"].iterations == K and got["res"] <= tol, name


def test_whole_step_through_the_fused_linsym_launch(ctx, monkeypatch):
    """One egs_problem_step of the 2 x 2 x 2 stack, forced onto the 1-lane timetable's isotropic LINSYM form with the
    fused assembly as test_gpu_model_reference.py forces it: lambda against the reference's sweeps on the blocks the
    step left, velocity() against v + dt (M^-1 f + M^-1 J^T lambda) for the device's own lambda, in the form and with
    the constant of the accumulators it is made of."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EGS_QUAD", "0")
    monkeypatch.setenv("EGS_STEP", "1")
    monkeypatch.setenv("EGS_ISO", "2")
    monkeypatch.delenv("EGS_FUSED_ASSEMBLY", raising=False)
    monkeypatch.delenv("EGS_ISO_LINSYM", raising=False)
    case = mref.step_scene_b()
    K, cfm = 10, 0.01
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"])
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    st = pr.step(case["dt"], case["erp"], capi.params(method=capi.GAUSS_SEIDEL, max_iters=K, tol=0.0, cfm=cfm), want_stats=True)
    lam, v6, acc, w = pr.lambda_(), pr.velocity(), pr.accumulators(), pr.wres()
    J0, J1, is_eq, lo, hi, rhs, _ = pr.blocks()
    pr.close()
    assert st.status == capi.OK and st.iterations == K
    assert st.schedule & capi.SCHED_FUSED_ASSEMBLY and st.schedule & capi.SCHED_LINSYM

    blocks = types.SimpleNamespace(n=case["p"].shape[0], m=case["kind"].shape[0], Minv=case["Minv"], body0=case["body0"],
                                   body1=case["body1"], J0=J0, J1=J1)
    A = ref.system(blocks, cfm)
    x_ref = ref.sweeps(A, rhs, is_eq, lo, hi, ref.GAUSS_SEIDEL, 1.5, K)
    r = ref.measure(A, rhs, is_eq, lo, hi, x_ref, lam, acc, w, st.residual)
    bound = ref.BOUNDS[("pile", False)]
    print("fused step: " + " ".join("%s=%.3g/%g" % (q, v, bound[q]) for q, v in sorted(r.items())))
    assert all(v <= bound[q] for q, v in r.items()), r
    vr = ref.velocity_after(case, J0, J1, lam)
    ratio = ref.err_vector(v6, vr.val)
    print("fused step: velocity error %.3g u max(1, |v'|), bound %g" % (ratio, bound["a"]))
    assert ratio <= bound["a"]      # v' is v + dt (M^-1 f + the accumulators): the accumulators' bound
