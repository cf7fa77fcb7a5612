"""GPU (-m gpu): live inertia in a batched world (egs_world_create_batch + egs_world_set_live_inertia, global body
indices).  The state is per body, so every ensemble of the batch must hold, after every step, exactly the bits of a
live world created for it alone -- through egs_world_step and egs_world_step_each; an ensemble sitting a step out
(dt[e] = 0) keeps its bodies and its get_mass rows; an ensemble of cubes is the live-off world bit for bit."""
import numpy as np
import pytest

import live_inertia_cases as lic
from eggshell_amd import capi, scenes
from oracle import oracle as orc
from test_gpu_world_step_each import batch_world, ensemble_view, same_bits, single_world

pytestmark = pytest.mark.gpu

ERP = 0.2


def with_mass(sc, joints):
    n = sc["p"].shape[0]
    e = dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy(), mass=sc["mass"], I_body=sc["I_body"],
             Minv=orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36),
             f_ext=orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6))
    e["joints"] = (sc["body0"], sc["body1"], sc["data"]) if joints else None
    return e


def free_bricks():
    a, b = lic.free_brick_bodies("random", z=6.0), lic.free_brick_bodies("intermediate", z=8.0)
    sc = {k: np.concatenate([a[k], b[k]]) for k in ("p", "R", "v", "w", "mass", "I_body")}
    sc["p"][1, 0] = 3.0
    return sc


def three_ensembles():
    """bricks on a chain; free bricks; a 2 x 2 x 2 stack of cubes, every body isotropic"""
    return [with_mass(lic.brick_chain(4), True), with_mass(free_bricks(), False),
            with_mass(scenes.box_stack(2, 2, 2, origin=(10.0, 10.0)), False)]


def live_batch(ctx, ens):
    bw, off = batch_world(ctx, ens, capi.F64)
    bw.set_live_inertia(np.concatenate([e["I_body"] for e in ens]))
    return bw, off


def live_single(ctx, e, live=True):
    w = single_world(ctx, e, capi.F64)
    if live:
        w.set_live_inertia(e["I_body"])
    return w


def assert_ensemble_is_single(bw, off, e, single, what):
    body, con, lam = ensemble_view(bw, bw.batch_info(), off, e)
    for a, b, name in zip(body, single.bodies(), ("pos", "R", "v", "w")):
        assert same_bits(a, b), (what, e, name)
    for a, b in zip(con, single.contacts()):
        assert same_bits(a, b), (what, e, "contacts")
    assert same_bits(lam, single.lambda_()), (what, e, "lambda")
    Mb, fb = bw.mass()
    Ms, fs = single.mass()
    s = slice(off[e], off[e + 1])
    assert same_bits(Mb[s], Ms) and same_bits(fb[s], fs), (what, e, "get_mass")


@pytest.mark.parametrize("entry", ["step", "step_each"])
def test_every_ensemble_is_its_own_live_world(ctx, entry):
    ens = three_ensembles()
    prm = capi.params(method=capi.SOR, max_iters=40, tol=1e-9, cfm=0.01)
    dts = [1e-3, 2e-3, 5e-3] if entry == "step_each" else [2e-3] * 3
    bw, off = live_batch(ctx, ens)
    singles = [live_single(ctx, e) for e in ens]
    cubes_off = live_single(ctx, ens[2], live=False)
    for k in range(10):
        if entry == "step":
            bw.step(dts[0], ERP, prm)
        else:
            bw.step_each(dts, ERP, prm)
        for e, s in enumerate(singles):
            s.step(dts[e], ERP, prm)
            assert_ensemble_is_single(bw, off, e, s, k)
        cubes_off.step(dts[2], ERP, prm)
        assert_ensemble_is_single(bw, off, 2, cubes_off, (k, "cubes, live off"))
    # the live ensembles did turn, and their blocks followed
    assert np.abs(singles[1].bodies()[1] - ens[1]["R"]).max() > 1e-3
    assert not same_bits(bw.mass()[0][off[1]:off[2]], ens[1]["Minv"])
    assert same_bits(bw.mass()[0][off[2]:off[3]], ens[2]["Minv"])
    bw.close(); cubes_off.close()
    for s in singles:
        s.close()


def test_an_ensemble_sitting_out_keeps_bodies_and_mass(ctx):
    ens = three_ensembles()
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=30, tol=0.0, cfm=0.01)
    bw, off = live_batch(ctx, ens)
    for _ in range(3):
        bw.step_each([1e-3, 1e-3, 1e-3], ERP, prm)
    for out in (0, 1):
        before_bodies, before_mass = bw.bodies(), bw.mass()
        dt = [1e-3, 1e-3, 1e-3]
        dt[out] = 0.0
        for _ in range(2):
            bw.step_each(dt, ERP, prm)
        s = slice(off[out], off[out + 1])
        for a, b in zip(before_bodies, bw.bodies()):
            assert same_bits(a[s], b[s]), out
        after_mass = bw.mass()
        assert same_bits(before_mass[0][s], after_mass[0][s]) and same_bits(before_mass[1][s], after_mass[1][s]), out
        other = slice(off[1 - out], off[2 - out])
        assert not same_bits(before_bodies[1][other], bw.bodies()[1][other])      # the others went on
    bw.close()
