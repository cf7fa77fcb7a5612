"""GPU (-m gpu): Ensemble::InitStabilize / PostStabilize for every ensemble of a world (egs_world_stabilize).
A plain world against the same loops built from oracle pieces (numpy's least squares for (J J^T) y = err, as
test_gpu_stabilize.py does for the adapter); every ensemble of a mixed batch bit for bit against a world that holds
it alone; a cairn relaxed with contact detection; the steps that follow; the refusals."""
import numpy as np
import pytest

from eggshell_amd import capi, scenes
from test_gpu_stabilize import explicit_euler, relaxation
from test_gpu_world_dense import ensemble, make_world

pytestmark = pytest.mark.gpu

INIT, POST = capi.STABILIZE_INIT, capi.STABILIZE_POST


def bent_chain(scale):
    sc = scenes.chain(4)
    for i in range(1, 4):
        sc["p"][i] += scale * np.array([0.01 * i, -0.02 * i, 0.015 * i])
    return sc


def loose_ensemble(sc):
    """Bodies only: contacts come from the world's detection."""
    n = sc["p"].shape[0]
    sc = dict(sc, kind=np.zeros(0, np.int32), body0=np.zeros(0, np.int32), body1=np.zeros(0, np.int32),
              data=np.zeros((0, 7)))
    e = ensemble(sc, joints=False)
    assert e["p"].shape[0] == n
    return e


def lone_box():
    """One box high above the ground: no joints, no contacts."""
    sc = dict(p=np.array([[3.0, 3.0, 5.0]]), R=np.eye(3).reshape(1, 9), v=np.array([[0.1, 0.0, 0.0]]),
              w=np.zeros((1, 3)), mass=np.ones(1), I_body=(np.eye(3) * 0.1).reshape(1, 9))
    return loose_ensemble(sc)


def mixed():
    return [ensemble(bent_chain(1.0)), ensemble(bent_chain(-0.7)), ensemble(bent_chain(1.6)),
            ensemble(scenes.chain(4)), loose_ensemble(scenes.cairn(5, seed=11)), lone_box()]


def state(w, off, e):
    pos, R, v, wv = w.bodies()
    s = slice(off[e], off[e + 1])
    return pos[s], R[s], v[s], wv[s]


def contacts(w, off, e):
    info = w.batch_info()
    b0, b1, data = w.contacts()
    co = info["contact_offset"]
    c = slice(co[e], co[e + 1])
    loc = lambda b: np.where(b >= 0, b - off[e], -1)
    return loc(b0[c]), loc(b1[c]), data[c]


def test_plain_chain_init_then_post_against_the_oracle(ctx):
    sc = bent_chain(1.0)
    e = ensemble(sc)
    w, off = make_world(ctx, [e])
    try:
        assert w.stabilize(INIT, detect_contacts=False) == 0
        info = w.stabilize_info()
        steps = 0
        corr, err = relaxation(sc)
        while err @ err > 1e-9 and steps < 100:            # InitStabilize, ensembles.cc:602-622
            explicit_euler(sc, corr, 0.001 * 500)
            corr, err = relaxation(sc)
            steps += 1
        assert info["steps"][0] == steps and 0 < steps < 100
        assert info["err_sq"][0] <= 1e-9
        pos, R, v, wv = w.bodies()
        assert np.abs(pos - sc["p"]).max() < 1e-8
        assert np.abs(R - sc["R"]).max() < 1e-8
        assert np.array_equal(v, e["v"]) and np.array_equal(wv, e["w"])
        # PostStabilize from the perturbation of test_gpu_stabilize.py, applied to both
        for i in range(1, 4):
            sc["p"][i] += np.array([-0.02, 0.01 * i, 0.0])
            sc["v"][i] = [0.1, 0.0, -0.2]
            pos[i] += np.array([-0.02, 0.01 * i, 0.0])
            v[i] = [0.1, 0.0, -0.2]
        w.set_bodies(pos, R, v, wv, None, None)
        assert w.stabilize(POST, detect_contacts=False) == 0
        steps = 0
        corr, err = relaxation(sc)
        while err @ err > 1e-9 and steps < 500:            # PostStabilize, ensembles.cc:624-646
            explicit_euler(sc, corr, 0.001 * 100)
            sc["v"] = sc["v"] + corr[:, :3]
            sc["w"] = sc["w"] + corr[:, 3:]
            corr, err = relaxation(sc)
            steps += 1
        assert w.stabilize_info()["steps"][0] == steps and steps > 0
        pos, R, v, wv = w.bodies()
        assert np.abs(pos - sc["p"]).max() < 1e-7
        assert np.abs(np.concatenate([v, wv], 1) - np.concatenate([sc["v"], sc["w"]], 1)).max() < 1e-6
    finally:
        w.close()


@pytest.mark.parametrize("mode", [POST, INIT])
def test_mixed_batch_matches_worlds_of_one(ctx, mode):
    ens = mixed()
    bw, boff = make_world(ctx, ens)
    singles = [make_world(ctx, [e]) for e in ens]
    try:
        bw.stabilize(mode)
        binfo = bw.stabilize_info()
        for e, (sw, soff) in enumerate(singles):
            sw.stabilize(mode)
            sinfo = sw.stabilize_info()
            assert binfo["steps"][e] == sinfo["steps"][0], e
            assert binfo["err_sq"][e].tobytes() == sinfo["err_sq"][0].tobytes(), e
            for a, b in zip(state(bw, boff, e), state(sw, soff, 0)):
                assert a.tobytes() == b.tobytes(), e
            for a, b in zip(contacts(bw, boff, e), contacts(sw, soff, 0)):
                assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), e
        assert binfo["steps"][:3].min() > 0
        for e in (3, 5):   # the settled chain and the empty ensemble: no step, their bits kept
            assert binfo["steps"][e] == 0
            pos, R, v, wv = state(bw, boff, e)
            assert np.array_equal(pos, ens[e]["p"]) and np.array_equal(R, ens[e]["R"])
            assert np.array_equal(v, ens[e]["v"]) and np.array_equal(wv, ens[e]["w"])
        assert binfo["err_sq"][5] == 0.0
    finally:
        bw.close()
        for sw, _ in singles:
            sw.close()


def test_cairn_init_with_contact_detection(ctx):
    e = loose_ensemble(scenes.cairn(6, seed=5))
    before = ctx.update_contacts(e["p"], e["R"])[2][:, 6].max()
    assert before > 0.01
    w, _ = make_world(ctx, [e])
    try:
        unsettled = w.stabilize(INIT)
        info = w.stabilize_info()
        assert (unsettled == 0 and info["err_sq"][0] <= 1e-9) or info["steps"][0] == 100
        assert info["steps"][0] > 0
        pos, R, v, wv = w.bodies()
        after = ctx.update_contacts(pos, R)[2][:, 6].max()
        assert after < before
        assert np.array_equal(v, e["v"]) and np.array_equal(wv, e["w"])
        assert w.info()["n_contacts"] == ctx.update_contacts(pos, R)[0].shape[0]
    finally:
        w.close()


@pytest.mark.parametrize("dense", [False, True])
def test_step_after_stabilize_is_a_fresh_worlds_step(ctx, dense):
    ens = [loose_ensemble(scenes.cairn(4, seed=7)), ensemble(bent_chain(1.0)), lone_box()]
    w, off = make_world(ctx, ens)
    try:
        w.stabilize(INIT)
        with pytest.raises(capi.EgsError) as err:
            w.lambda_()
        assert err.value.status == capi.ERR_INVALID
        pos, R, v, wv = w.bodies()
        fresh_ens = []
        for e in range(len(ens)):
            s = slice(off[e], off[e + 1])
            fresh_ens.append(dict(ens[e], p=pos[s], R=R[s], v=v[s], w=wv[s]))
        fw, foff = make_world(ctx, fresh_ens)
        try:
            for world in (w, fw):
                if dense:
                    assert world.step_dense(1e-3) == 0
                else:
                    world.step(1e-3, 0.2, capi.params(method=capi.SOR, max_iters=200, tol=1e-9))
            for a, b in zip(w.bodies(), fw.bodies()):
                assert a.tobytes() == b.tobytes()
            for a, b in zip(w.contacts(), fw.contacts()):
                assert a.tobytes() == b.tobytes()
            assert w.lambda_().tobytes() == fw.lambda_().tobytes()
        finally:
            fw.close()
    finally:
        w.close()


def test_step_cap_and_unsettled_count(ctx):
    """max_steps > 0 caps each ensemble's loop; n_unsettled counts those left with err_sq > 1e-9."""
    sc = bent_chain(1.0)
    ens = [ensemble(sc), ensemble(scenes.chain(4))]
    w, off = make_world(ctx, ens)
    try:
        assert w.stabilize(POST, max_steps=3, detect_contacts=False) == 1
        info = w.stabilize_info()
        assert info["steps"].tolist() == [3, 0]
        assert info["err_sq"][0] > 1e-9 and info["err_sq"][1] <= 1e-9
        for _ in range(3):                                  # three passes of PostStabilize
            corr, _ = relaxation(sc)
            explicit_euler(sc, corr, 0.001 * 100)
            sc["v"] = sc["v"] + corr[:, :3]
            sc["w"] = sc["w"] + corr[:, 3:]
        pos, R, v, wv = state(w, off, 0)
        assert np.abs(pos - sc["p"]).max() < 1e-7
        assert np.abs(np.concatenate([v, wv], 1) - np.concatenate([sc["v"], sc["w"]], 1)).max() < 1e-6
        _, err = relaxation(sc)
        assert abs(info["err_sq"][0] - err @ err) <= 1e-6 * err @ err
    finally:
        w.close()


def test_caller_params(ctx):
    """A caller's relaxation solve (Gauss-Seidel here) instead of the adapter's SOR: the same loop, to the oracle."""
    sc = bent_chain(-0.8)
    w, _ = make_world(ctx, [ensemble(sc)])
    try:
        prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=20000, tol=1e-12, check_every=10)
        assert w.stabilize(INIT, detect_contacts=False, params=prm) == 0
        info = w.stabilize_info()
        steps = 0
        corr, err = relaxation(sc)
        while err @ err > 1e-9 and steps < 100:
            explicit_euler(sc, corr, 0.001 * 500)
            corr, err = relaxation(sc)
            steps += 1
        assert info["steps"][0] == steps > 0
        assert np.abs(w.bodies()[0] - sc["p"]).max() < 1e-8
        bad = capi.params(method=capi.SOR, max_iters=-1, tol=1e-11)
        start = w.bodies()
        with pytest.raises(capi.EgsError) as e:
            w.stabilize(POST, params=bad)
        assert e.value.status == capi.ERR_INVALID
        for a, b in zip(w.bodies(), start):
            assert a.tobytes() == b.tobytes()
    finally:
        w.close()


def test_refusals(ctx):
    e = ensemble(bent_chain(1.0))
    w32, _ = make_world(ctx, [e], capi.F32)
    try:
        with pytest.raises(capi.EgsError) as err:
            w32.stabilize(INIT)
        assert err.value.status == capi.ERR_UNSUPPORTED
        assert np.array_equal(w32.bodies()[0], e["p"])
    finally:
        w32.close()
    empty = capi.World(ctx, 4)
    try:
        with pytest.raises(capi.EgsError) as err:
            empty.stabilize(INIT)
        assert err.value.status == capi.ERR_INVALID
    finally:
        empty.close()
    w, off = make_world(ctx, [e, ensemble(bent_chain(-1.0))])
    try:
        w.step(1e-3, 0.2, capi.params(method=capi.SOR, max_iters=50, tol=0.0))
        start = w.bodies()
        with pytest.raises(capi.EgsError) as err:   # before any stabilise call
            w.stabilize_info()
        assert err.value.status == capi.ERR_INVALID
        for mode, max_steps in ((2, 0), (-1, 0), (INIT, -1), (POST, -5)):
            with pytest.raises(capi.EgsError) as err:
                w.stabilize(mode, max_steps=max_steps)
            assert err.value.status == capi.ERR_INVALID
        for a, b in zip(w.bodies(), start):
            assert a.tobytes() == b.tobytes()
        w.lambda_()   # still the step's
        w.stabilize(POST)
        with pytest.raises(capi.EgsError) as err:
            w.lambda_()
        assert err.value.status == capi.ERR_INVALID
        w.n_ensembles = 1
        with pytest.raises(capi.EgsError) as err:   # wrong E
            w.stabilize_info()
        assert err.value.status == capi.ERR_INVALID
        w.n_ensembles = 2
        assert w.stabilize_info()["steps"].shape == (2,)
        w.step(1e-3, 0.2, capi.params(method=capi.SOR, max_iters=50, tol=0.0))
        assert w.lambda_().shape[0] == 3 * w.info()["n_constraints"]
    finally:
        w.close()
