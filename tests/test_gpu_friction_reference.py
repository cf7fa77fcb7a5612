"""GPU (-m gpu): the device's friction pyramid (egs_problem_set_friction) on every kernel a sweep can run on
(test_gpu_solve_start.SCHEDULES), fp64 and fp32, against the 50-digit reference of tests/friction_reference.py on the
seeded cases: lambda against sweeps_pyramid; accumulators(), wres() and the reported residual against the mathematics at
the device's own lambda (residual_pyramid with the rounded bound); EGS_SCHED_FRICTION and the schedule's own flags; the
sweep count of the two tolerance-terminated runs.  Bounds: friction_reference.BOUNDS.  Every test
prints error / bound per schedule (pytest -s)."""
import pytest

import friction_reference as fr
import sweep_reference as ref
from eggshell_amd import capi
from test_gpu_solve_start import SCHEDULES, set_schedule

pytestmark = pytest.mark.gpu

PRECISION = {False: capi.F64, True: capi.F32}
ISO_CASES = ("iso-plain", "iso-linsym")
OVERSIZE_FLAGS = {"quad_patches": capi.SCHED_QUAD_PATCHES, "lane_patches": capi.SCHED_LANE_PATCHES,
                  "all_global": capi.SCHED_ALL_GLOBAL}
_measured = {}


def solve(ctx, c, mu, method, K, f32, tol=0.0):
    s = c.s
    pr = capi.Problem(ctx, s.n, s.body0, s.body1, PRECISION[f32])
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, c.rhs)
    pr.set_friction(mu)
    if c.x0 is not None:
        pr.set_start(capi.START_GIVEN, c.x0)
    st = pr.solve(capi.params(method=method, max_iters=K, tol=tol, cfm=c.cfm, omega=c.omega))
    out = dict(x=pr.lambda_(), a=pr.accumulators(), w=pr.wres(), res=st.residual, st=st)
    pr.close()
    assert st.status == capi.OK
    return out


def ratios(cid, method, K, f32, got):
    """The four error ratios of one device result; equal bits are measured once."""
    key = (cid, method, K, f32, got["x"].tobytes(), got["a"].tobytes(), got["w"].tobytes(), got["res"])
    if key not in _measured:
        c = ref.case(cid)
        _measured[key] = fr.measure(ref.case_system(cid, f32), c.rhs, c.s.is_eq, c.s.lo, c.s.hi, fr.case_mu(cid),
                                    fr.case_iterates(cid, method, f32)[K], got["x"], got["a"], got["w"], got["res"])
    return _measured[key]


def schedules_of(cid, monkeypatch):
    c = ref.case(cid)
    for name in SCHEDULES:
        method = set_schedule(monkeypatch, name)
        if method not in c.runs:
            continue
        if cid in ISO_CASES and name in ("tile", "timetable"):
            monkeypatch.setenv("EGS_ISO", "2")
        yield name, method


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", fr.CASES)
def test_friction_cases_on_every_schedule(ctx, cid, f32, monkeypatch):
    """K = 4 sweeps at m = 1, 63, 64, 65, 255, 256, 257, 513 with a seeded mu from {-1, 0, 0.3, 1.0, 2.5} (about half the
    constraints flagged; mixed row types under the pyramid), the plain isotropic and the LINSYM form, runs of four, a
    start whose normals are partly negative, one oversize island, and the contact scenes at their sweep counts with
    mu = 0.5 on every contact and -1 on the joints."""
    c = ref.case(cid)
    mu = fr.case_mu(cid)
    assert (mu >= 0).any()
    if cid == "start":
        assert (c.x0[2::3][mu >= 0] < 0).any()
    bound = fr.BOUNDS[(c.cls, f32)]
    bad, worst = [], dict(x=0.0, a=0.0, w=0.0, r=0.0)
    for name, method in schedules_of(cid, monkeypatch):
        for K in c.runs[method]:
            got = solve(ctx, c, mu, method, K, f32)
            st = got["st"]
            assert st.iterations == K
            assert st.schedule & capi.SCHED_FRICTION, (name, st.schedule)
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


@pytest.mark.parametrize("method", fr.STOP_METHODS, ids=["gs", "sor"])
def test_a_tolerance_terminated_friction_run_stops_where_the_reference_stops(ctx, method, monkeypatch):
    """singular222 with mu = 0.5, tol 1e-9: every schedule of the method stops at the reference's sweep."""
    K, clear, _ = fr.stop_reference(method)
    assert K is not None and clear
    c = ref.case(fr.STOP_CASE)
    mu = fr.case_mu(fr.STOP_CASE)
    ran = 0
    for name in SCHEDULES:
        if set_schedule(monkeypatch, name) != method:
            continue
        got = solve(ctx, c, mu, method, fr.STOP_LIMIT, False, tol=fr.STOP_TOL)
        print("%-19s stops after %d sweeps (reference %d), residual %.3g" % (name, got["st"].iterations, K, got["res"]))
        assert got["st"].iterations == K and got["res"] <= fr.STOP_TOL, name
        assert got["st"].schedule & capi.SCHED_FRICTION
        ran += 1
    assert ran > 0
