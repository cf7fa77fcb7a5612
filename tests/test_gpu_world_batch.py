"""GPU (-m gpu): the batched world (egs_world_create_batch).  E independent
ensembles stepped by one device pipeline -- SimulationStep() calling Step() on
every Ensemble in turn (model.cc:37-70) -- must leave each ensemble, after every
step, with exactly the bits of a world that holds only that ensemble: bodies,
contact list (order included), lambda, sweep count and residual."""
import numpy as np
import pytest

from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT, ERP = 0.005, 0.2


def ensemble(sc, joints=False, zero_force=False):
    """Bodies (and, if asked, the scene's joints, ensemble-local indices) of one ensemble."""
    n = sc["p"].shape[0]
    e = dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy(),
             Minv=orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36),
             f_ext=orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6))
    if zero_force:
        e["f_ext"] = np.zeros((n, 6))
    e["joints"] = (sc["body0"], sc["body1"], sc["data"]) if joints else None
    return e


def bodies(p):
    p = np.asarray(p, float).reshape(-1, 3)
    n = p.shape[0]
    return dict(p=p, R=np.tile(np.eye(3).reshape(9), (n, 1)), v=np.zeros((n, 3)), w=np.zeros((n, 3)),
                mass=np.ones(n), I_body=np.tile((np.eye(3) * 0.1).reshape(9), (n, 1)))


def three_boxes(origin=(0.0, 0.0)):
    return bodies([[origin[0], origin[1], 0.2 + 0.35 * k] for k in range(3)])


def spaced_chain(n, z=2.0):
    """n boxes 0.6 apart along x, ball joints halfway between neighbours, the first held at its left: links
    that never touch, so there are no contacts (scenes.chain's links meet at their corners)."""
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


def mixed_batch():
    """Case 1: chain(9) with joints, two piles and three dropped boxes, all at one origin."""
    return [ensemble(scenes.chain(9, anchor=(0.0, 0.0, 0.6)), joints=True),
            ensemble(scenes.box_stack(2, 2, 3)), ensemble(scenes.box_stack(4, 4, 3)),
            ensemble(three_boxes())]


def single_world(ctx, e, precision):
    n = e["p"].shape[0]
    w = capi.World(ctx, n, precision)
    w.set_bodies(e["p"], e["R"], e["v"], e["w"], e["Minv"], e["f_ext"], side=e.get("side"))
    if e["joints"] is not None:
        w.set_joints(*e["joints"])
    return w


def batch_world(ctx, ens, precision):
    w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens], precision)
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens]) if off[-1] else np.zeros((0, d))
    side = None
    if any(e.get("side") is not None for e in ens):   # an ensemble without side lengths of its own: cubes of 0.3
        side = np.concatenate([np.full((e["p"].shape[0], 3), 0.3) if e.get("side") is None else e["side"] for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6), side=side)
    b0, b1, data = [], [], []
    for e, o in zip(ens, off):
        if e["joints"] is not None:
            j0, j1, jd = e["joints"]
            b0.append(np.where(j0 >= 0, j0 + o, -1)); b1.append(np.where(j1 >= 0, j1 + o, -1)); data.append(jd)
    if b0:
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


def check_no_cross_contacts(w, info, off):
    b0, b1, _ = w.contacts()
    co = info["contact_offset"]
    assert co[0] == 0 and co[-1] == len(b0) and (np.diff(co) >= 0).all()
    for e in range(len(off) - 1):
        for b in (b0[co[e]:co[e + 1]], b1[co[e]:co[e + 1]]):
            b = b[b >= 0]
            assert ((b >= off[e]) & (b < off[e + 1])).all(), e


def run_against_singles(ctx, ens, prm, steps, precision=capi.F64, after_step=None):
    """Steps the batch and one world per (non-empty) ensemble side by side; bit-for-bit checks after
    every step.  Returns the per-step arrays of per-ensemble sweep counts."""
    bw, off = batch_world(ctx, ens, precision)
    singles = [single_world(ctx, e, precision) if e["p"].shape[0] else None for e in ens]
    counts = []
    try:
        for step in range(steps):
            bst = bw.step(DT, ERP, prm, want_stats=True)
            sst = [s.step(DT, ERP, prm, want_stats=True) if s is not None else None for s in singles]
            info = bw.batch_info()
            check_no_cross_contacts(bw, info, off)
            counts.append(info["iterations"].copy())
            for e, s in enumerate(singles):
                body, con, lam = ensemble_view(bw, info, off, e)
                if s is None:   # an empty ensemble: nothing of its own, nothing solved
                    assert all(a.size == 0 for a in body + con) and lam.size == 0
                    assert info["iterations"][e] == 0 and info["residual"][e] == 0.0
                    continue
                for a, b in zip(body, s.bodies()):
                    assert np.array_equal(a, b), (step, e, "bodies")
                for a, b in zip(con, s.contacts()):
                    assert np.array_equal(a, b), (step, e, "contacts")
                assert np.array_equal(lam, s.lambda_()), (step, e, "lambda")
                assert info["iterations"][e] == sst[e].iterations, (step, e, info["iterations"][e], sst[e].iterations)
                assert np.array_equal(info["residual"][e], sst[e].residual), (step, e, info["residual"][e], sst[e].residual)
            assert bst.iterations == info["iterations"].max()
            assert bst.residual == info["residual"].max()
            if after_step is not None:
                after_step(step, bw, off, info, bst)
    finally:
        bw.close()
        for s in singles:
            if s is not None:
                s.close()
    return np.array(counts)


def test_mixed_batch_co_located_matches_separate_worlds(ctx):
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    counts = run_against_singles(ctx, mixed_batch(), prm, 40)
    # the stopping rule is per ensemble: the sweep counts differ between ensembles
    assert any(len(set(c.tolist())) > 1 for c in counts), counts
    assert (counts < 500).any()


@pytest.mark.parametrize("case", ["gauss_seidel", "jacobi", "jacobi_global", "f32", "check_every", "cap1", "no_defer"])
def test_mixed_batch_other_solves(ctx, case, monkeypatch):
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    precision = capi.F64
    if case == "gauss_seidel":
        prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=500, tol=1e-9, cfm=0.01)
    elif case == "jacobi":
        # projected Jacobi diverges on stacked boxes (the oracle's fast_iterate as well): chains, which it
        # solves to the tolerance in a few dozen sweeps, and single-layer piles, on which it stays bounded
        prm = capi.params(method=capi.JACOBI, max_iters=500, tol=1e-9, cfm=0.01)
        ens = [ensemble(scenes.chain(9), joints=True), ensemble(scenes.chain(5), joints=True),
               ensemble(scenes.box_stack(1, 1, 1)), ensemble(scenes.chain(12), joints=True),
               ensemble(scenes.box_stack(2, 2, 1))]
        run_against_singles(ctx, ens, prm, 15)
        return
    elif case == "jacobi_global":
        # a 600-joint chain is one island larger than a workgroup takes: Jacobi runs it on the cross-workgroup
        # kernels, a launch per sweep, so the stopping test runs after every sweep instead of on recorded chunks
        prm = capi.params(method=capi.JACOBI, max_iters=500, tol=1e-9, cfm=0.1)
        ens = [ensemble(spaced_chain(600), joints=True), ensemble(spaced_chain(7), joints=True),
               ensemble(scenes.box_stack(1, 1, 1))]

        def oversize(step, bw, off, info, bst):
            assert bst.n_global > 0

        run_against_singles(ctx, ens, prm, 4, after_step=oversize)
        return
    elif case == "f32":
        precision = capi.F32
        prm = capi.params(method=capi.SOR, max_iters=300, tol=1e-4, cfm=0.01)
    elif case == "check_every":   # only every 4th sweep (and the cap) is tested
        prm = capi.params(method=capi.SOR, max_iters=301, tol=1e-9, cfm=0.01, check_every=4)
    elif case == "cap1":          # max_iters 1: the loop without recorded chunks
        prm = capi.params(method=capi.SOR, max_iters=1, tol=1e-9, cfm=0.01)
    elif case == "no_defer":      # the residual of x0 read on its own
        monkeypatch.setenv("EGS_DEFER_RESIDUAL", "0")
    run_against_singles(ctx, mixed_batch(), prm, 15, precision)


def test_large_co_located_batch_on_the_grid(ctx):
    """256 co-located 4x4x4 piles (16 384 bodies: the hashed-grid broad phase), 50 fixed sweeps."""
    from test_gpu_collide import reference_contacts
    E = 256
    ens = [ensemble(scenes.box_stack(4, 4, 4, jitter=0.004, seed=e)) for e in range(E)]
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=50, tol=0.0, cfm=0.01)
    bw, off = batch_world(ctx, ens, capi.F64)
    sample = [0, 1, 77, 128, E - 1]
    singles = {e: single_world(ctx, ens[e], capi.F64) for e in sample}
    try:
        for step in range(3):
            pos0, R0, _, _ = bw.bodies()
            bst = bw.step(DT, ERP, prm, want_stats=True)
            info = bw.batch_info()
            check_no_cross_contacts(bw, info, off)
            assert (info["iterations"] == 50).all() and bst.iterations == 50
            for e, s in singles.items():
                st = s.step(DT, ERP, prm, want_stats=True)
                body, con, lam = ensemble_view(bw, info, off, e)
                for a, b in zip(body, s.bodies()):
                    assert np.array_equal(a, b), (step, e)
                for a, b in zip(con, s.contacts()):
                    assert np.array_equal(a, b), (step, e)
                assert np.array_equal(lam, s.lambda_()), (step, e)
                assert info["iterations"][e] == st.iterations and info["residual"][e] == st.residual, (step, e)
            e = E - 1
            r0, r1, rd = reference_contacts(pos0[off[e]:off[e + 1]], R0[off[e]:off[e + 1]])
            _, (c0, c1, cd), _ = ensemble_view(bw, info, off, e)
            assert np.array_equal(c0, r0) and np.array_equal(c1, r1) and np.array_equal(cd, rd), step
    finally:
        bw.close()
        for s in singles.values():
            s.close()


def test_edge_ensembles(ctx):
    """An empty ensemble, a free body, and an ensemble whose x0 already passes (a body held at its
    own centre by a ball joint to the world, no force on it: rhs = 0), next to a pile."""
    held = bodies([[3.0, 3.0, 5.0]])
    held.update(body0=np.array([0], np.int32), body1=np.array([-1], np.int32),
                data=np.array([[0.0, 0.0, 0.0, 3.0, 3.0, 5.0, 0.0]]))
    ens = [ensemble(scenes.box_stack(2, 2, 2)), ensemble(bodies(np.zeros((0, 3)))),
           ensemble(bodies([[0.0, 0.0, 5.0]])), ensemble(held, joints=True, zero_force=True), ensemble(three_boxes())]
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    counts = run_against_singles(ctx, ens, prm, 10)
    assert (counts[:, 1] == 0).all() and (counts[:, 2] == 0).all()
    assert (counts[:, 3] == 0).all()      # stopped at x0
    assert (counts[:, 0] > 0).all()


def test_batch_of_one_is_the_plain_world(ctx):
    sc = three_boxes()
    e = ensemble(sc)
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    bw, off = batch_world(ctx, [e], capi.F64)
    pw = single_world(ctx, e, capi.F64)
    assert off.tolist() == [0, 3]
    try:
        for step in range(20):
            bst = bw.step(DT, ERP, prm, want_stats=True)
            pst = pw.step(DT, ERP, prm, want_stats=True)
            assert (bst.iterations, bst.residual) == (pst.iterations, pst.residual)
            for a, b in zip(bw.bodies(), pw.bodies()):
                assert np.array_equal(a, b), step
            for a, b in zip(bw.contacts(), pw.contacts()):
                assert np.array_equal(a, b), step
            assert np.array_equal(bw.lambda_(), pw.lambda_())
            assert bw.info() == pw.info()
            info = bw.batch_info()
            assert info["iterations"][0] == pst.iterations and info["residual"][0] == pst.residual
            assert info["contact_offset"].tolist() == [0, pw.info()["n_contacts"]]
            assert info["joint_offset"].tolist() == [0, 0]
    finally:
        bw.close()
        pw.close()


def test_three_boxes_in_a_batch_match_the_oracle(ctx):
    from test_gpu_fullstep import oracle_step_loop
    drop = three_boxes()
    ens = [ensemble(scenes.chain(9, anchor=(0.0, 0.0, 0.6)), joints=True), ensemble(drop),
           ensemble(scenes.box_stack(2, 2, 2))]
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    bw, off = batch_world(ctx, ens, capi.F64)
    seen = 0
    try:
        for _ in range(120):
            bw.step(DT, ERP, prm)
            co = bw.batch_info()["contact_offset"]
            seen += int(co[2] - co[1])
        pos, R, v, w = bw.bodies()
    finally:
        bw.close()
    s = slice(off[1], off[2])
    po, v6o, seen_o = oracle_step_loop(drop["p"], drop["R"], 120, DT)
    assert seen == seen_o
    assert np.abs(pos[s] - po).max() < 1e-7
    assert np.abs(np.concatenate([v[s], w[s]], axis=1) - v6o).max() < 1e-5


def test_refusals(ctx):
    with pytest.raises(capi.EgsError) as e:
        capi.World.batch(ctx, [3, -1, 2])
    assert e.value.status == capi.ERR_INVALID
    w, off = capi.World.batch(ctx, [2, 2, 2])
    try:
        jd = np.zeros((1, 7))
        with pytest.raises(capi.EgsError) as e:     # bodies 1 (ensemble 0) and 2 (ensemble 1)
            w.set_joints([1], [2], jd)
        assert e.value.status == capi.ERR_INVALID
        with pytest.raises(capi.EgsError) as e:     # ensemble 1 before ensemble 0
            w.set_joints([2, 0], [3, -1], np.zeros((2, 7)))
        assert e.value.status == capi.ERR_INVALID
        w.set_joints([0, 2, 3, 4], [1, -1, -1, 5], np.zeros((4, 7)))   # grouped, world allowed
        assert w.batch_info()["joint_offset"].tolist() == [0, 1, 3, 4]
    finally:
        w.close()
