"""GPU (-m gpu): restitution on a problem (egs_problem_set_restitution).  The assembly's rhs against the fp64 twin of
tests/restitution_reference.py, bit for bit; off is the untouched problem; the fused step launch (ASSEMBLE, PAIR and
CHAIN forms, storing and store-free) against assemble + solve; the refusals; the dense step on a dropped cube."""
import ctypes as C

import numpy as np
import pytest

import bench
import restitution_reference as rr
import step_chain_cases as scc
import step_contact_bounds_cases as sbc
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP, CFM = 5e-3, 0.2, 0.01
BASE_ENV = {"EGS_QUAD": "0", "EGS_ISO": "2", "EGS_STEP": "1"}      # the 1-lane isotropic timetable kernel for small piles


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_problem(ctx, case, precision=capi.F64):
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"], precision)
    pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    return pr


# ---- 1. the assembly against the twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", rr.IDS)
def test_assemble_is_the_twin(ctx, cid, precision):
    case, rest, vth, J0, J1, err, want, what = rr.generated(cid)
    pr = make_problem(ctx, case, precision)
    pr.assemble(case["dt"], case["erp"])
    off = pr.blocks()
    pr.set_restitution(rest, vth)
    pr.assemble(case["dt"], case["erp"])
    on = pr.blocks()
    pr.close()
    cast = (lambda a: a) if precision == capi.F64 else (lambda a: np.asarray(a).astype(np.float32).astype(np.float64))
    if precision == capi.F64:
        assert bits(on[0].reshape(-1), np.asarray(J0).reshape(-1)) and bits(on[1].reshape(-1), np.asarray(J1).reshape(-1))
    assert bits(on[6].reshape(-1), np.asarray(err).reshape(-1))
    assert bits(on[5].reshape(-1), cast(want))
    # everything but rhs[2] of the bouncing contacts is what the same call gives with restitution off
    for k in (0, 1, 2, 3, 4, 6):
        assert bits(on[k], off[k]), k
    same = np.ones(on[5].size, bool)
    same[[3 * i + 2 for i, w in enumerate(what) if w == "bounce"]] = False
    assert bits(on[5].reshape(-1)[same], off[5].reshape(-1)[same])
    if "bounce" in what:
        assert not bits(on[5], off[5])


def each_world(ctx, precision, rest, vth):
    """Three one-body ensembles, each a cube resting on the plate and moving down at its own speed; warm start on, so
    that start() reports the first step's x0: its rhs rows."""
    from test_gpu_world_step_each import batch_world, bodies, ensemble
    ens = []
    for vz in (-1.0, -2.0, -0.5):
        sc = bodies([[0.0, 0.0, 0.149]])
        sc["v"][0] = [0.1, 0.0, vz]
        ens.append(ensemble(sc))
    w, off = batch_world(ctx, ens, precision)
    w.set_warm_start(True, 0.01)
    if rest is not None:
        w.set_restitution(rest, vth)
    return w, ens


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_each_form_is_the_twin_and_a_sitter_is_zero(ctx, precision):
    """assemble_kernel's per-ensemble form, read through the warm start's first x0 (no history: the rhs rows): every
    ensemble on its own dt and erp, ensemble 1 sitting out."""
    rest, vth = np.array([0.5, 0.9, -1.0]), 0.3
    dt, erp = np.array([5e-3, 0.0, 2e-3]), np.array([0.2, 0.2, 0.4])
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=2, tol=0.0, cfm=CFM)
    rows = {}
    for on in (False, True):
        w, ens = each_world(ctx, precision, rest if on else None, vth)
        w.step_each(dt, erp, prm)
        rows[on] = w.start()[0]
        b0, b1, data = w.contacts()
        w.close()
    m = len(b0)
    assert m == 12 and (b0 < 0).all()
    case = dict(p=np.concatenate([e["p"] for e in ens]), R=np.concatenate([e["R"] for e in ens]),
                v=np.concatenate([e["v"] for e in ens]), w=np.concatenate([e["w"] for e in ens]),
                Minv=np.concatenate([e["Minv"] for e in ens]), f_ext=np.concatenate([e["f_ext"] for e in ens]),
                kind=np.ones(m, np.int32), body0=b0, body1=b1, data=data, dt=0.0, erp=0.0)
    J0, J1, _, _, _, err = orc.assemble(case["p"], case["R"], case["kind"], b0, b1, data)
    cast = (lambda a: a) if precision == capi.F64 else (lambda a: a.astype(np.float32).astype(np.float64))
    for on in (False, True):
        want, what, margin = rr.twin_rhs(case, J0, J1, err, rest[b1] if on else None, vth, dt[b1], erp[b1])
        assert min(min(x) for x in margin) > rr.TIE
        assert bits(rows[on], cast(want)), on
        assert np.all(rows[on][3 * 4:3 * 8] == 0.0) and not np.signbit(rows[on][3 * 4:3 * 8]).any()
        if on:
            assert what[:4] == ["bounce"] * 4 and what[4:8] == ["sits"] * 4 and what[8:] == ["off"] * 4
    assert not bits(rows[True][:12], rows[False][:12]) and bits(rows[True][12:], rows[False][12:])


# ---- 2. off is the parent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["null", "negative", "idle"])
def test_off_is_the_untouched_problem(ctx, table):
    case, rest, vth, *_ = rr.generated("m257")
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=7, tol=0.0, cfm=CFM)
    out = []
    for touched in (False, True):
        pr = make_problem(ctx, case)
        if touched:
            if table == "null":
                pr.set_restitution(rest, vth)
                pr.set_restitution(None, vth)
            elif table == "negative":
                pr.set_restitution(np.full(rest.shape, -0.5), 0.0)
            else:      # coefficients >= 0 behind a threshold no contact reaches
                pr.set_restitution(np.abs(rest), 1e6)
        pr.step(case["dt"], case["erp"], prm)
        out.append((pr.blocks()[5], pr.lambda_(), pr.velocity(), pr.schedule()))
        pr.close()
    for a, b in zip(*out):
        assert bits(np.asarray(a), np.asarray(b))


# ---- 3. the fused launch against assemble + solve ------------------------------------------------------------------------
FORMS = {"lane": ("s4", 0), "pair": ("odd3", capi.SCHED_PAIR), "chain": ("g32", capi.SCHED_PAIR | capi.SCHED_CHAIN)}
_scene = {}
# switches that would take these piles off the fused forms (tests/tools/env_matrix.sh sets some): cleared here
FORM_SWITCHES = ("EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY", "EGS_STEP_CHAIN", "EGS_STEP_PAIR", "EGS_STEP_STEADY",
                 "EGS_TILE", "EGS_LANE_ORDER")


def falling(form):
    if form not in _scene:
        name = FORMS[form][0]
        sc = dict(sbc.scene(name) if form == "lane" else scc.scene(name))
        rng = np.random.default_rng(11)
        sc["v"] = sc["v"].copy()
        sc["v"][:, 2] -= rng.uniform(0.05, 2.0, sc["v"].shape[0])      # every body approaches the one below it
        m = sc["body0"].shape[0]
        _scene[form] = (sc, np.array([rr.COEFFICIENTS[i % 5] for i in range(m)]))
    return _scene[form]


@pytest.mark.parametrize("store", [False, True], ids=["deferred", "storing"])
@pytest.mark.parametrize("method", ["gs", "sor", "jacobi"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_fused_step_is_assemble_plus_solve(ctx, monkeypatch, form, method, store):
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    for k in FORM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if store:
        monkeypatch.setenv("EGS_STEP_DEFER_SYSTEM", "0")
    else:
        monkeypatch.delenv("EGS_STEP_DEFER_SYSTEM", raising=False)
    sc, rest = falling(form)
    vth = 0.5
    prm = (capi.params(method=capi.JACOBI, max_iters=5, tol=0.0, cfm=CFM) if method == "jacobi" else sbc.params(method, 5))
    res = {}
    for path in ("step", "unfused", "step_off"):
        if path == "unfused":
            monkeypatch.setenv("EGS_FUSED_ASSEMBLY", "0")      # assemble_kernel, then the sweep launch
        else:
            monkeypatch.delenv("EGS_FUSED_ASSEMBLY", raising=False)
        pr, _ = bench.build_problem(ctx, sc, capi.F64)
        if path != "step_off":
            pr.set_restitution(rest, vth)
        pr.step(DT, ERP, prm)
        st = pr.stats()
        sched = pr.schedule()
        lam, v6 = pr.lambda_(), pr.velocity()
        rhs = pr.blocks()[5]                                     # a deferred system is materialised here, after the step
        res[path] = dict(lam=lam, rhs=rhs, v6=v6, sched=sched, deferred=bool(st.schedule & capi.SCHED_DEFERRED_SYSTEM))
        pr.close()
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    pr.set_restitution(rest, vth)
    pr.assemble(DT, ERP)
    pr.solve(prm)
    split = dict(lam=pr.lambda_(), rhs=pr.blocks()[5])
    pr.close()
    on, unfused, off = res["step"], res["unfused"], res["step_off"]
    assert not unfused["sched"] & capi.SCHED_FUSED_ASSEMBLY
    assert bits(on["lam"], unfused["lam"]) and bits(on["rhs"], unfused["rhs"]) and bits(on["v6"], unfused["v6"])
    assert bits(on["lam"], split["lam"]) and bits(on["rhs"], split["rhs"])
    # the velocities: v + dt M^-1 (f + J^T lambda) from the oracle, as the other step tests compare them
    Minv, f_ext = bench.host_mass_and_force(sc)
    J0, J1, _, _, _, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
    v6o = orc.velocity_update(sc["v"], sc["w"], Minv, f_ext, sc["body0"], sc["body1"], J0, J1, on["lam"], DT)
    assert np.abs(on["v6"] - v6o).max() <= 1e-12 * max(1.0, np.abs(v6o).max())
    # restitution changes something here, and the rhs is the twin's
    case = dict(sc, Minv=Minv, f_ext=f_ext, dt=DT, erp=ERP)
    want, what, _ = rr.twin_rhs(case, J0, J1, err, rest, vth)
    assert "bounce" in what and bits(on["rhs"].reshape(-1), want) and not bits(on["lam"], off["lam"])
    # the schedule is the one of the same step without restitution: fused where that is (GS, SOR), with its form
    assert on["sched"] == off["sched"] and on["deferred"] == off["deferred"] == (method != "jacobi" and not store)
    fused = capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_PAIR | capi.SCHED_CHAIN
    assert on["sched"] & fused == (0 if method == "jacobi" else capi.SCHED_FUSED_ASSEMBLY | FORMS[form][1])


def test_deferred_system_keeps_the_table_of_its_step(ctx, monkeypatch):
    """The setter materialises a deferred system before it changes the table: the rhs read afterwards is the step's."""
    for k, v in BASE_ENV.items():
        monkeypatch.setenv(k, v)
    for k in FORM_SWITCHES + ("EGS_STEP_DEFER_SYSTEM",):
        monkeypatch.delenv(k, raising=False)
    sc, rest = falling("chain")
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    pr.set_restitution(rest, 0.5)
    pr.step(DT, ERP, sbc.params("gs", 3))
    assert pr.stats().schedule & capi.SCHED_DEFERRED_SYSTEM
    pr.set_restitution(None, 0.0)
    rhs = pr.blocks()[5]
    pr.close()
    Minv, f_ext = bench.host_mass_and_force(sc)
    J0, J1, _, _, _, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
    want = rr.twin_rhs(dict(sc, Minv=Minv, f_ext=f_ext, dt=DT, erp=ERP), J0, J1, err, rest, 0.5)[0]
    assert bits(rhs.reshape(-1), want)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_table(ctx):
    case, rest, vth, J0, J1, err, want, what = rr.generated("m40")
    pr = make_problem(ctx, case)
    pr.set_restitution(rest, vth)
    bad = rest.copy()
    for value, thr in ((np.nan, vth), (np.inf, vth), (-np.inf, vth), (None, -1.0), (None, np.nan), (None, np.inf)):
        table = rest
        if value is not None:
            table = bad.copy(); table[3] = value
        with pytest.raises(capi.EgsError) as ei:
            pr.set_restitution(table, thr)
        assert ei.value.status == capi.ERR_INVALID
    pr.assemble(case["dt"], case["erp"])
    assert bits(pr.blocks()[5].reshape(-1), want)
    pr.close()
    from test_gpu_world_step_each import bodies, ensemble, single_world
    w = single_world(ctx, ensemble(bodies([[0.0, 0.0, 0.149]])), capi.F64)
    w.set_restitution(0.5, 0.1)
    lib = capi.load()
    one = np.array([0.5])
    for n, table, thr in ((2, one, 0.1), (1, None, 0.1), (1, np.array([np.nan]), 0.1), (1, np.array([np.inf]), 0.1),
                          (1, one, -0.5), (1, one, np.nan), (1, one, np.inf)):
        ptr = None if table is None else table.ctypes.data_as(C.c_void_p)
        assert lib.egs_world_set_restitution(w.h, C.c_int32(n), ptr, C.c_double(thr)) == capi.ERR_INVALID
    w.close()


# ---- 5. the dense step on a dropped cube -------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0.0, 0.6, 1.0])
def test_dense_step_on_a_dropped_cube(ctx, e):
    """One 0.3 cube flat on the plate, 1 mm deep, falling at 2 m/s: four contacts.  egs_problem_step_dense with bounds:
    every contact's normal speed after the step is at least -e vn (and the Baumgarte floor), and the velocities are the
    oracle's mixed solve of the twin's rhs within the dense path's bound (tests/test_gpu_dense_path.py: 1e-9)."""
    sc = scenes.box_stack(1, 1, 1)
    sc = dict(sc, p=sc["p"].copy(), v=sc["v"].copy())
    sc["p"][0, 2] -= 1e-3
    sc["v"][0, 2] = -2.0
    b0, b1, data = ctx.update_contacts(sc["p"], sc["R"])
    m = len(b0)
    assert m == 4
    Minv, f_ext = bench.host_mass_and_force(sc)
    pr = capi.Problem(ctx, 1, b0, b1)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
    kind = np.ones(m, np.int32)
    pr.set_constraints(kind, data)
    rest = np.full(m, e)
    pr.set_restitution(rest, 0.0)
    ok, _ = pr.step_dense(DT, ERP, CFM, use_bounds=1)
    assert ok
    v6, lam = pr.velocity().reshape(-1), pr.lambda_()
    pr.close()
    J0, J1, is_eq, lo, hi, err = orc.assemble(sc["p"], sc["R"], kind, b0, b1, data)
    case = dict(sc, Minv=Minv, f_ext=f_ext, kind=kind, body0=b0, body1=b1, data=data, dt=DT, erp=ERP)
    rhs, what, _ = rr.twin_rhs(case, J0, J1, err, rest, 0.0)
    assert what == (["bounce"] * 4 if e > 0 else ["floor"] * 4)
    Jn = np.asarray(J1).reshape(m, 3, 6)[:, 2, :]
    vn_old = Jn @ np.concatenate([sc["v"][0], sc["w"][0]])
    vn_new = Jn @ v6
    target = np.maximum(-e * vn_old, ERP * data[:, 6] / DT)
    # (A + cfm I) lambda - rhs >= 0 is J v' >= target - dt cfm lambda: the regularisation's share, plus rounding
    tol = DT * CFM * np.abs(lam).max() + 1e-9 * max(1.0, np.abs(target).max())
    print("e=%g: normal speeds %s, targets %s, tol %.3g" % (e, vn_new, target, tol))
    assert np.all(vn_new >= target - tol)
    # the reference's step: the oracle's MixedConstraintsSolver on the same matrix and the twin's rhs
    Jf = np.asarray(J1).reshape(3 * m, 6)
    A = Jf @ np.asarray(Minv).reshape(6, 6) @ Jf.T + CFM * np.eye(3 * m)
    oko, xo, _, _ = orc.mixed_constraints(A, rhs, np.asarray(is_eq).reshape(-1), np.asarray(lo).reshape(-1),
                                          np.asarray(hi).reshape(-1), 1)
    assert oko and np.abs(lam - xo).max() <= 1e-8 * max(1.0, np.abs(xo).max())
    v6o = orc.velocity_update(sc["v"], sc["w"], Minv, f_ext, b0, b1, J0, J1, lam, DT).reshape(-1)
    assert np.abs(v6 - v6o).max() <= 1e-9 * max(1.0, np.abs(v6o).max())
