"""GPU (-m gpu): step_solve_kernel's LINSYM form (one linear block for both sides of a constraint) at the bench
configuration.  It must give the bits of the plain isotropic timetable kernel (EGS_ISO_LINSYM=0) -- lambda, w and the
accumulators, byte for byte -- and of the sequential oracle; a scene with unequal masses must stay on the plain kernel."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import bench
from eggshell_amd import capi, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@contextmanager
def linsym_env(value):
    old = os.environ.get("EGS_ISO_LINSYM")
    if value is None:
        os.environ.pop("EGS_ISO_LINSYM", None)
    else:
        os.environ["EGS_ISO_LINSYM"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("EGS_ISO_LINSYM", None)
        else:
            os.environ["EGS_ISO_LINSYM"] = old


def c3_piles(batch, heavy=False):
    nx, ny, nz, _, _, _ = bench.WORKLOADS["c3"]
    piles = [scenes.box_stack(nx, ny, nz, jitter=1e-3, seed=k + 1, origin=(0.0, 100.0 * k)) for k in range(batch)]
    sc = scenes.concat(piles)
    if heavy:   # one box of the last pile twice as heavy: unequal linear weights on its contacts
        sc["mass"] = sc["mass"].copy()
        sc["mass"][-1] *= 2.0
    return sc, piles


def run(ctx, sc, prm, env):
    """One step of the scene (assemble, solve, velocity) with EGS_ISO_LINSYM = env; the arrays as bytes-comparable copies."""
    _, _, _, _, _, dt = bench.WORKLOADS["c3"]
    with linsym_env(env):
        pr, _ = bench.build_problem(ctx, sc, capi.F64)
        st = pr.step(dt, 0.2, prm, want_stats=True)
    out = dict(lam=pr.lambda_(), wres=pr.wres(), acc=pr.accumulators(), v6=pr.velocity(), blocks=pr.blocks())
    pr.close()
    return st, out


def assert_same_bytes(a, b):
    for k in ("lam", "wres", "acc", "v6"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def oracle_check(sc, piles, out, method, sweeps, omega, which):
    J0, J1, is_eq, lo, hi, rhs, _ = out["blocks"]
    Minv, _ = bench.host_mass_and_force(sc)
    m1, n1 = piles[0]["kind"].shape[0], piles[0]["p"].shape[0]
    for k in which:
        cons, rows, bod = slice(k * m1, (k + 1) * m1), slice(3 * k * m1, 3 * (k + 1) * m1), slice(k * n1, (k + 1) * n1)
        s = orc.Sys(Minv[bod], np.where(sc["body0"][cons] >= 0, sc["body0"][cons] - k * n1, -1), sc["body1"][cons] - k * n1,
                    J0[cons], J1[cons], is_eq[rows], lo[rows], hi[rows])
        xf, af, _, _ = orc.fast_iterate(s, rhs[rows], 0.01, method, max_iters=sweeps, tol=0.0, omega=omega)
        assert np.array_equal(out["lam"][rows], xf), "pile %d" % k
        assert np.array_equal(out["acc"][bod], af), "pile %d" % k
        assert np.array_equal(out["wres"][rows], orc.fast_wres(s, rhs[rows], 0.01, xf, af)), "pile %d" % k


@pytest.mark.parametrize("method", ["gs", "sor"])
def test_linsym_bits_c3x24(ctx, method):
    sweeps = bench.WORKLOADS["c3"][3]
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    prm = capi.params(method=meth, max_iters=sweeps, tol=0.0, cfm=0.01, omega=omega)
    sc, piles = c3_piles(24)
    st_new, new = run(ctx, sc, prm, None)
    st_old, old = run(ctx, sc, prm, "0")
    assert st_new.status == capi.OK and st_old.status == capi.OK
    assert st_new.schedule & capi.SCHED_STATIC and st_new.schedule & capi.SCHED_ISO
    assert st_new.schedule & capi.SCHED_LINSYM
    assert not st_old.schedule & capi.SCHED_LINSYM
    assert_same_bytes(new, old)
    oracle_check(sc, piles, new, meth, sweeps, omega, which=(0, 23))


def test_linsym_bits_tol_loop(ctx):
    """A tolerance-terminated solve: its first launch (sweep 0) runs the LINSYM form, the snapshot-recording resumed
    launches the plain kernel on the accumulators it left."""
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=300, tol=1e-7, cfm=0.01)
    sc, _ = c3_piles(24)
    st_new, new = run(ctx, sc, prm, None)
    st_old, old = run(ctx, sc, prm, "0")
    assert st_new.status == capi.OK and st_old.status == capi.OK
    assert st_new.iterations == st_old.iterations and st_new.residual == st_old.residual
    assert_same_bytes(new, old)


def test_linsym_mixed_mass_falls_back(ctx):
    sweeps = bench.WORKLOADS["c3"][3]
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=sweeps, tol=0.0, cfm=0.01)
    sc, piles = c3_piles(24, heavy=True)
    st_new, new = run(ctx, sc, prm, None)
    st_old, old = run(ctx, sc, prm, "0")
    assert st_new.status == capi.OK
    assert st_new.schedule & capi.SCHED_STATIC and st_new.schedule & capi.SCHED_ISO
    assert not st_new.schedule & capi.SCHED_LINSYM
    assert_same_bytes(new, old)
    oracle_check(sc, piles, new, capi.GAUSS_SEIDEL, sweeps, 1.0, which=(23,))
