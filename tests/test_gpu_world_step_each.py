"""GPU (-m gpu): a time step and an erp per ensemble (egs_world_step_each, egs_world_step_dense_each).  A batched
world stepped with dt[e] / erp[e] must leave each ensemble, after every step, with exactly the bits of a world that
holds only that ensemble and takes step(dt[e], erp[e]): bodies, contact list (order included), lambda, sweep count
and residual.  An ensemble with dt[e] = 0 sits the step out: its single world is not stepped.

The contact list of an ensemble that sits out: the world's detection runs on the poses of NOW, while the single
world's stored list is the one its last step detected BEFORE that step moved the bodies.  What the batched list must
equal is therefore the detection at the single's current poses: the stateless egs_update_contacts_joints on the
single's bodies, and the list the single's own next step detects (the same poses: it has not moved in between)."""
import ctypes as C

import numpy as np
import pytest

from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


# ---- the helpers of tests/test_gpu_world_batch.py ------------------------------------------------------------------
def ensemble(sc, joints=False):
    n = sc["p"].shape[0]
    e = dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy(),
             Minv=orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36),
             f_ext=orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6))
    e["joints"] = (sc["body0"], sc["body1"], sc["data"]) if joints else None
    return e


def bodies(p):
    p = np.asarray(p, float).reshape(-1, 3)
    n = p.shape[0]
    return dict(p=p, R=np.tile(np.eye(3).reshape(9), (n, 1)), v=np.zeros((n, 3)), w=np.zeros((n, 3)),
                mass=np.ones(n), I_body=np.tile((np.eye(3) * 0.1).reshape(9), (n, 1)))


def three_boxes():
    return bodies([[0.0, 0.0, 0.2 + 0.35 * k] for k in range(3)])


def spaced_chain(n, z=2.0):
    sc = bodies([[0.6 * i, 0.0, z] for i in range(n)])
    b0 = np.arange(n, dtype=np.int32)
    b1 = np.append(np.arange(1, n, dtype=np.int32), -1).astype(np.int32)
    data = np.zeros((n, 7))
    data[:n - 1, 0:3] = [0.3, 0.0, 0.0]
    data[:n - 1, 3:6] = [-0.3, 0.0, 0.0]
    data[n - 1, 0:3] = [-0.3, 0.0, 0.0]
    data[n - 1, 3:6] = [-0.3, 0.0, z]
    b0[n - 1] = 0
    sc.update(body0=b0, body1=b1, data=data)
    return sc


def single_world(ctx, e, precision):
    w = capi.World(ctx, e["p"].shape[0], precision)
    w.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"])
    if e["joints"] is not None:
        w.set_joints(*e["joints"])
    return w


def batch_world(ctx, ens, precision, bodies_set=True):
    w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens], precision)
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens]) if off[-1] else np.zeros((0, d))
    if bodies_set:
        w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6))
    b0, b1, data = [], [], []
    for e, o in zip(ens, off):
        if e["joints"] is not None:
            j0, j1, jd = e["joints"]
            b0.append(np.where(j0 >= 0, j0 + o, -1)); b1.append(np.where(j1 >= 0, j1 + o, -1)); data.append(jd)
    if b0 and bodies_set:
        w.set_joints(np.concatenate(b0), np.concatenate(b1), np.concatenate(data))
    return w, off


def ensemble_view(w, info, off, e):
    """Ensemble e's part of the batched world, in its own (local) numbering."""
    pos, R, v, wv = w.bodies()
    s = slice(off[e], off[e + 1])
    b0, b1, data = w.contacts()
    co, jo = info["contact_offset"], info["joint_offset"]
    c = slice(co[e], co[e + 1])
    lb0 = np.where(b0[c] >= 0, b0[c] - off[e], -1).astype(np.int32)
    lb1 = np.where(b1[c] >= 0, b1[c] - off[e], -1).astype(np.int32)
    lam = w.lambda_()
    mj = jo[-1]
    lam_e = np.concatenate([lam[3 * jo[e]:3 * jo[e + 1]], lam[3 * (mj + co[e]):3 * (mj + co[e + 1])]])
    return (pos[s], R[s], v[s], wv[s]), (lb0, lb1, data[c]), lam_e


# ---- the ensembles: the smallest that reach every path ---------------------------------------------------------------
def small_batch():
    """2 joints and no contacts; 8 contacts; a contact set that changes while it settles; one free body; no body."""
    return [ensemble(spaced_chain(2), joints=True), ensemble(scenes.box_stack(1, 1, 2)), ensemble(three_boxes()),
            ensemble(bodies([[0.0, 0.0, 5.0]])), ensemble(bodies(np.zeros((0, 3))))]


DT5 = [1e-3, 5e-3, 2.5e-3, 4e-3, 1e-3]
ERP5 = [0.2, 0.2, 0.1, 0.3, 0.2]
SOLVES = {
    "gs_tol": dict(method=capi.GAUSS_SEIDEL, max_iters=500, tol=1e-9, cfm=0.01),
    "sor_fixed": dict(method=capi.SOR, max_iters=20, tol=0.0, cfm=0.01),
    "jacobi_fixed": dict(method=capi.JACOBI, max_iters=10, tol=0.0, cfm=0.01),
}


def same_bits(a, b):
    """np.array_equal on the values' bits (so a NaN equals the same NaN, and -0 differs from +0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_each_against_singles(ctx, ens, prm, rates, precision=capi.F64):
    """Steps the batch with step_each(dt, erp) of every entry of `rates` and one world per non-empty ensemble with
    step(dt[e], erp[e]) -- not at all where dt[e] = 0 -- side by side; bit-for-bit checks after every step.
    Returns the world's re-plan count after every step."""
    bw, off = batch_world(ctx, ens, precision)
    singles = [single_world(ctx, e, precision) if e["p"].shape[0] else None for e in ens]
    awaited = {}      # ensemble -> the list the batch detected while it sat out: its single's next step must detect it
    replans = []
    try:
        for step, (dt, erp) in enumerate(rates):
            bst = bw.step_each(dt, erp, prm, want_stats=True)
            info = bw.batch_info()
            replans.append(bw.info()["replans"])
            for e, s in enumerate(singles):
                body, con, lam = ensemble_view(bw, info, off, e)
                if s is None:   # an empty ensemble: nothing of its own, nothing solved
                    assert all(a.size == 0 for a in body + con) and lam.size == 0
                    assert info["iterations"][e] == 0 and info["residual"][e] == 0.0
                    continue
                if dt[e] == 0:   # sits out: the single is not stepped
                    pos, R = s.bodies()[:2]
                    now = ctx.update_contacts(pos, R, joints=ens[e]["joints"])
                    for a, b in zip(con, now):
                        assert np.array_equal(a, b), (step, e, "contacts of an ensemble sitting out")
                    awaited[e] = con
                    assert lam.shape[0] == 3 * (len(con[0]) + (len(ens[e]["joints"][0]) if ens[e]["joints"] else 0))
                    assert np.all(lam == 0.0), (step, e, "lambda of an ensemble sitting out")
                    assert info["residual"][e] == 0.0, (step, e, info["residual"][e])
                    want = 0 if prm.tol > 0 or lam.size == 0 else prm.max_iters
                    assert info["iterations"][e] == want, (step, e, info["iterations"][e], want)
                else:
                    sst = s.step(dt[e], np.broadcast_to(erp, (len(ens),))[e], prm, want_stats=True)
                    for a, b in zip(con, s.contacts()):
                        assert np.array_equal(a, b), (step, e, "contacts")
                    if e in awaited:
                        for a, b in zip(awaited.pop(e), s.contacts()):
                            assert np.array_equal(a, b), (step, e, "contacts after sitting out")
                    assert np.array_equal(lam, s.lambda_()), (step, e, "lambda")
                    assert info["iterations"][e] == sst.iterations, (step, e, info["iterations"][e], sst.iterations)
                    assert np.array_equal(info["residual"][e], sst.residual), (step, e, info["residual"][e], sst.residual)
                for a, b in zip(body, s.bodies()):
                    assert np.array_equal(a, b), (step, e, "bodies")
            assert bst.iterations == info["iterations"].max()
            assert bst.residual == info["residual"].max()
    finally:
        bw.close()
        for s in singles:
            if s is not None:
                s.close()
    return replans


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solve", list(SOLVES))
def test_mixed_rates_match_separate_worlds(ctx, solve, precision):
    prm = capi.params(**SOLVES[solve])
    replans = run_each_against_singles(ctx, small_batch(), prm, [(DT5, ERP5)] * 6, precision)
    print("re-plans after each step:", replans)


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solve", list(SOLVES))
def test_sit_out(ctx, solve, precision):
    """Steps 2, 3 and 5 (of 0..5) let the pile, the chain and the three boxes sit out, one each."""
    prm = capi.params(**SOLVES[solve])
    rates = []
    for step in range(6):
        dt = list(DT5)
        if step in (2, 3, 5):
            dt[{2: 1, 3: 0, 5: 2}[step]] = 0.0
        rates.append((dt, ERP5))
    run_each_against_singles(ctx, small_batch(), prm, rates, precision)


def state_of(w):
    info = w.batch_info()
    return list(w.bodies()) + list(w.contacts()) + [w.lambda_(), info["joint_offset"], info["contact_offset"],
                                                    info["iterations"], info["residual"]]


@pytest.mark.parametrize("solve", list(SOLVES))
def test_every_dt_zero_moves_nothing(ctx, solve):
    prm = capi.params(**SOLVES[solve])
    ens = small_batch()
    bw, off = batch_world(ctx, ens, capi.F64)
    try:
        bw.step_each(DT5, ERP5, prm)
        bw.step_each(DT5, ERP5, prm)
        before = bw.bodies()
        st = capi.load().egs_world_step_each(bw.h, C.c_int32(5), capi._p(np.zeros(5)), capi._p(np.array(ERP5)),
                                             C.byref(prm), C.c_int32(1), None)
        assert st == capi.OK
        for a, b in zip(before, bw.bodies()):
            assert same_bits(a, b)
        assert np.all(bw.lambda_() == 0.0)
        info = bw.batch_info()
        assert np.all(info["residual"] == 0.0)
        for e in range(5):
            rows = (info["joint_offset"][e + 1] - info["joint_offset"][e]) + (info["contact_offset"][e + 1] - info["contact_offset"][e])
            assert info["iterations"][e] == (0 if prm.tol > 0 or rows == 0 else prm.max_iters)
    finally:
        bw.close()


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solve", list(SOLVES))
def test_equal_rates_equal_the_scalar_entry(ctx, solve, precision):
    prm = capi.params(**SOLVES[solve])
    wa, _ = batch_world(ctx, small_batch(), precision)
    wb, _ = batch_world(ctx, small_batch(), precision)
    try:
        for step in range(4):
            sa = wa.step(5e-3, 0.2, prm, want_stats=True)
            sb = wb.step_each([5e-3] * 5, [0.2] * 5, prm, want_stats=True)
            for a, b in zip(state_of(wa), state_of(wb)):
                assert same_bits(a, b), step
            assert sa.schedule == sb.schedule
            assert (sa.iterations, sa.status, sa.n_islands, sa.n_tiles, sa.n_global, sa.tile_constraints) == \
                   (sb.iterations, sb.status, sb.n_islands, sb.n_tiles, sb.n_global, sb.tile_constraints)
            assert same_bits(np.float64(sa.residual), np.float64(sb.residual))
        assert wa.info() == wb.info()
    finally:
        wa.close(); wb.close()


def test_plain_world_takes_one_rate(ctx):
    """A plain world is one ensemble: step_each([dt], [erp]) is step(dt, erp); dt 0 leaves it alone."""
    prm = capi.params(**SOLVES["gs_tol"])
    e = ensemble(scenes.box_stack(1, 1, 2))
    wa, wb = single_world(ctx, e, capi.F64), single_world(ctx, e, capi.F64)
    try:
        for step in range(3):
            wa.step(4e-3, 0.3, prm)
            wb.step_each([4e-3], 0.3, prm)
            for a, b in zip(state_of(wa), state_of(wb)):
                assert same_bits(a, b), step
        before = wb.bodies()
        wb.step_each([0.0], 0.3, prm)
        for a, b in zip(before, wb.bodies()):
            assert same_bits(a, b)
        info = wb.batch_info()
        assert np.all(wb.lambda_() == 0.0) and info["iterations"][0] == 0 and info["residual"][0] == 0.0
        wa.step(4e-3, 0.3, prm)
        wb.step_each([4e-3], [0.3], prm)
        for a, b in zip(state_of(wa), state_of(wb)):
            assert same_bits(a, b)
    finally:
        wa.close(); wb.close()


# ---- the dense path ----------------------------------------------------------------------------------------------------
def dense_batch():
    """6, 24, 96 (the <= 112 class) and 144 rows (above the fused cap: the multi-launch route)."""
    return [ensemble(spaced_chain(2), joints=True), ensemble(scenes.box_stack(1, 1, 2)),
            ensemble(scenes.box_stack(2, 2, 2)), ensemble(scenes.box_stack(2, 2, 3))]


def dense_chains():
    """The same four size classes with equality rows only -- 6, 24, 96 and 144 rows of ball joints -- which the
    reference's solver takes with use_bounds = 0 too (it gives up on the piles' contact rows there, see below)."""
    return [ensemble(spaced_chain(n), joints=True) for n in (2, 8, 32, 48)]


def run_dense_each(ctx, ens, use_bounds, must_solve):
    """step_dense_each with ensemble 2 sitting out, an iterative step_each, step_dense_each with every ensemble,
    against one world per ensemble.  A dense step in which an ensemble's solve fails (use_bounds = 0 on contact piles:
    egs_world_step_dense's own behaviour, the reference Panics there) advances no body of the batch, while the
    singles that do solve advance: then the failing set, the figures of dense_info and the untouched bodies are
    compared and the run ends.  must_solve: such a failure is itself a failure of the test."""
    bw, off = batch_world(ctx, ens, capi.F64)
    singles = [single_world(ctx, e, capi.F64) for e in ens]
    prm = capi.params(**SOLVES["gs_tol"])
    erp = [0.2, 0.1, 0.2, 0.3]

    def compare(step, dt, dense):
        info = bw.batch_info()
        dinfo = bw.dense_info() if dense else None
        for e, s in enumerate(singles):
            body, con, lam = ensemble_view(bw, info, off, e)
            for a, b in zip(body, s.bodies()):
                assert np.array_equal(a, b), (step, e, "bodies")
            if dt[e] == 0:   # sits out: the detection at its (untouched) poses, lambda rows of 0, not solved
                pos, R = s.bodies()[:2]
                for a, b in zip(con, ctx.update_contacts(pos, R, joints=ens[e]["joints"])):
                    assert np.array_equal(a, b), (step, e, "contacts of an ensemble sitting out")
                assert np.all(lam == 0.0) and lam.size == 96, (step, e, lam.size)
                assert dinfo["ok"][e] and dinfo["pivots"][e] == 0 and dinfo["cfm"][e] == 0.0
                continue
            for a, b in zip(con, s.contacts()):
                assert np.array_equal(a, b), (step, e, "contacts")
            assert np.array_equal(lam, s.lambda_()), (step, e, "lambda")
            if dense:
                assert dinfo["ok"][e]
                assert info["iterations"][e] == dinfo["pivots"][e]

    def dense_step(step, dt):
        """True if every ensemble solved (then everything is compared); False after a failing step's checks."""
        before = bw.bodies()
        nf = bw.step_dense_each(dt, erp, cfm=0.01, use_bounds=use_bounds)
        failed = [s.step_dense(dt[e], erp[e], cfm=0.01, use_bounds=use_bounds) if dt[e] > 0 else 0
                  for e, s in enumerate(singles)]
        assert nf == sum(failed), (step, nf, failed)
        dinfo = bw.dense_info()
        for e, s in enumerate(singles):
            if dt[e] == 0:
                assert dinfo["ok"][e] and dinfo["pivots"][e] == 0 and dinfo["cfm"][e] == 0.0, (step, e)
                continue
            si = s.dense_info()
            for k in ("pivots", "cfm", "ok", "condition"):
                assert np.array_equal(dinfo[k][e], si[k][0]), (step, e, k, dinfo[k][e], si[k][0])
            assert bool(dinfo["ok"][e]) == (failed[e] == 0), (step, e)
        if nf == 0:
            compare(step, dt, True)
            return True
        assert not must_solve, (step, "ensembles failed to solve", failed)
        for a, b in zip(before, bw.bodies()):   # a failure of one ensemble advances no body, sitting out or not
            assert same_bits(a, b), (step, "a body moved in a failed step")
        return False

    def topology():
        b0, b1, _ = bw.contacts()
        return b0.tobytes(), b1.tobytes()

    try:
        if not dense_step(0, [1e-3, 5e-3, 0.0, 2e-3]):
            return False
        topo, replans = topology(), bw.info()["replans"]
        dt = [2e-3, 1e-3, 3e-3, 1e-3]   # an iterative step in between: the two paths share one plan
        bw.step_each(dt, erp, prm)
        for e, s in enumerate(singles):
            s.step(dt[e], erp[e], prm)
        compare(1, dt, False)
        same_list = [topology() == topo]
        moved = [bw.info()["replans"] - replans]
        topo, replans = topology(), bw.info()["replans"]
        if not dense_step(2, [1e-3, 5e-3, 2.5e-3, 2e-3]):
            return False
        same_list.append(topology() == topo)
        moved.append(bw.info()["replans"] - replans)
        # a re-plan happens only where the contact topology changed, never because the entry or the solver did
        print("contact list unchanged:", same_list, "re-plans:", moved)
        for same, d in zip(same_list, moved):
            assert d == (0 if same else 1), (same_list, moved)
        assert any(same_list), "the contact lists changed on every step: the check above saw no switch"
        return True
    finally:
        bw.close()
        for s in singles:
            s.close()


@pytest.mark.parametrize("use_bounds", [0, 1])
def test_dense_each_matches_separate_worlds(ctx, use_bounds):
    """The piles' contact rows are solved with use_bounds = 1 only: with 0 (the reference, quirk Q3)
    egs_world_step_dense itself reports them failed, and so must the per-ensemble entry, ensemble by ensemble."""
    solved = run_dense_each(ctx, dense_batch(), use_bounds, must_solve=use_bounds == 1)
    print("use_bounds", use_bounds, "every ensemble solved:", solved)


@pytest.mark.parametrize("use_bounds", [0, 1])
def test_dense_each_on_equality_rows(ctx, use_bounds):
    """The whole run -- sit-out, the switch to the sweeps and back, both dense routes -- where use_bounds = 0 solves."""
    assert run_dense_each(ctx, dense_chains(), use_bounds, must_solve=True)


@pytest.mark.parametrize("use_bounds", [0, 1])
def test_dense_equal_rates_equal_the_scalar_entry(ctx, use_bounds):
    wa, _ = batch_world(ctx, dense_batch(), capi.F64)
    wb, _ = batch_world(ctx, dense_batch(), capi.F64)
    try:
        for step in range(2):
            na = wa.step_dense(5e-3, 0.2, cfm=0.01, use_bounds=use_bounds)
            nb = wb.step_dense_each([5e-3] * 4, 0.2, cfm=0.01, use_bounds=use_bounds)
            assert na == nb and (na == 0 or use_bounds == 0), (step, na, nb)
            for k, (a, b) in enumerate(zip(state_of(wa), state_of(wb))):
                if na > 0 and k == 7:   # lambda: the rows of an ensemble whose solve failed are not written
                    continue
                assert same_bits(a, b), (step, k)
            ia, ib = wa.dense_info(), wb.dense_info()
            for k in ia:
                assert same_bits(ia[k], ib[k]), (step, k)
    finally:
        wa.close(); wb.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_move_nothing(ctx):
    prm = capi.params(**SOLVES["gs_tol"])
    ens = small_batch()
    lib = capi.load()
    good_dt, good_erp = np.array(DT5), np.array(ERP5)

    def sweeps(w, E, dt, erp):
        return lib.egs_world_step_each(w.h, C.c_int32(E), capi._p(dt), capi._p(erp), C.byref(prm), C.c_int32(1), None)

    def dense(w, E, dt, erp):
        return lib.egs_world_step_dense_each(w.h, C.c_int32(E), capi._p(dt), capi._p(erp), C.c_double(0.01), C.c_int32(0),
                                             C.c_int32(1), None)

    # before set_bodies
    w0, _ = batch_world(ctx, ens, capi.F64, bodies_set=False)
    try:
        assert sweeps(w0, 5, good_dt, good_erp) == capi.ERR_INVALID
        assert dense(w0, 5, good_dt, good_erp) == capi.ERR_INVALID
    finally:
        w0.close()

    bad = {"negative": good_dt.copy(), "nan": good_dt.copy()}
    bad["negative"][2] = -1e-3
    bad["nan"][1] = np.nan
    for entry in (sweeps, dense):
        bw, off = batch_world(ctx, ens, capi.F64)
        singles = [single_world(ctx, e, capi.F64) if e["p"].shape[0] else None for e in ens]
        try:
            bw.step_each(DT5, ERP5, prm)
            before = bw.bodies()
            assert entry(bw, 4, good_dt, good_erp) == capi.ERR_INVALID      # wrong n_ensembles
            assert entry(bw, 6, np.append(good_dt, 1e-3), np.append(good_erp, 0.2)) == capi.ERR_INVALID
            assert entry(bw, 5, bad["negative"], good_erp) == capi.ERR_INVALID
            assert entry(bw, 5, bad["nan"], good_erp) == capi.ERR_INVALID
            assert entry(bw, 5, None, good_erp) == capi.ERR_INVALID         # a NULL array
            assert entry(bw, 5, good_dt, None) == capi.ERR_INVALID
            for a, b in zip(before, bw.bodies()):
                assert same_bits(a, b)
            # a valid step afterwards still matches the singles
            bw.step_each(DT5, ERP5, prm)
            info = bw.batch_info()
            for e, s in enumerate(singles):
                if s is None:
                    continue
                s.step(DT5[e], ERP5[e], prm)
                s.step(DT5[e], ERP5[e], prm)
                body, con, lam = ensemble_view(bw, info, off, e)
                for a, b in zip(body, s.bodies()):
                    assert np.array_equal(a, b), (e, "bodies")
                for a, b in zip(con, s.contacts()):
                    assert np.array_equal(a, b), (e, "contacts")
                assert np.array_equal(lam, s.lambda_()), (e, "lambda")
        finally:
            bw.close()
            for s in singles:
                if s is not None:
                    s.close()


def test_wrapper_refuses_a_wrong_length(ctx):
    prm = capi.params(**SOLVES["gs_tol"])
    bw, _ = batch_world(ctx, small_batch(), capi.F64)
    try:
        before = bw.bodies()
        with pytest.raises(ValueError):
            bw.step_each(DT5[:4], 0.2, prm)
        with pytest.raises(ValueError):
            bw.step_dense_each(DT5, ERP5[:3])
        with pytest.raises(capi.EgsError) as ei:
            bw.step_each([1e-3, -1.0, 1e-3, 1e-3, 1e-3], 0.2, prm)
        assert ei.value.status == capi.ERR_INVALID
        for a, b in zip(before, bw.bodies()):
            assert same_bits(a, b)
    finally:
        bw.close()


def test_dense_each_is_fp64_only(ctx):
    bw, _ = batch_world(ctx, small_batch(), capi.F32)
    try:
        st = capi.load().egs_world_step_dense_each(bw.h, C.c_int32(5), capi._p(np.array(DT5)), capi._p(np.array(ERP5)),
                                                   C.c_double(0.01), C.c_int32(0), C.c_int32(1), None)
        assert st == capi.ERR_UNSUPPORTED
    finally:
        bw.close()
