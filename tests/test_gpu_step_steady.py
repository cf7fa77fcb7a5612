"""GPU (-m gpu): step_solve_kernel's steady-state loop (EGS_STEP_STEADY).  It changes no operand and no rounding, so
lambda, w, the accumulators and the velocities must keep every bit of

  * the same build with the switch off (the single general loop),
  * the sequential CPU oracle (the velocity update as the other step tests compare it: its sums are ordered otherwise),

on shapes at which the window between fill and drain is empty, a few steps long, or most of the launch (cases and
sweep counts: step_steady_cases.py): one partly filled tile, one full 256-lane tile, tiles that mix islands of different
depth and keep inactive lanes; GS and backward SOR; the fused store-free launch (step), the plain LINSYM launch
(assemble + solve), the regular kernel, the plain isotropic kernel and fp32 at one tile per workgroup (these two keep
the single loop: no registers for a second one), and the stopping loop, whose snapshot-recording launches keep it too.  Every environment runs in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import step_steady_cases as ssc
from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OFF = {"EGS_STEP_STEADY": "0"}
SWITCHES = ("EGS_STEP_STEADY", "EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY",
            "EGS_STEP_DEFER_SYSTEM")

_results = {}


def results(tmp_path_factory, group, **switches):
    """Every output of every case of `group` from one fresh process with `switches` set (cached per environment)."""
    ident = (group,) + tuple(sorted(switches.items()))
    if ident not in _results:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(ssc.BASE_ENV)
        env.update(switches)
        path = str(tmp_path_factory.mktemp("steady") / "out.npz")
        r = subprocess.run([sys.executable, os.path.abspath(ssc.__file__), group, path], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(path) as z:
            _results[ident] = {k: z[k] for k in z.files}
    return _results[ident]


def assert_same(new, old):
    assert new.keys() == old.keys() and len(new) > 0
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k


def schedules(res, path):
    return [int(res[k][2]) for k in res if k.endswith(".st") and ".%s." % path in k]


def statuses_ok(res):
    return all(int(res[k][0]) == capi.OK for k in res if k.endswith(".st"))


def test_default_runs_the_intended_kernels(tmp_path_factory):
    on = results(tmp_path_factory, "main")
    assert statuses_ok(on)
    fused = capi.SCHED_STATIC | capi.SCHED_ISO | capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_DEFERRED_SYSTEM
    assert all(s & fused == fused for s in schedules(on, "step"))
    plain = capi.SCHED_STATIC | capi.SCHED_ISO | capi.SCHED_LINSYM
    assert all(s & plain == plain and not s & capi.SCHED_FUSED_ASSEMBLY for s in schedules(on, "solve"))
    assert all(s & capi.SCHED_STATIC and not s & capi.SCHED_FUSED_ASSEMBLY for s in schedules(on, "tol"))


def test_switch_off(tmp_path_factory):
    """GS and SOR, step and assemble + solve, all scenes and sweep counts, and the stopping loop."""
    on, off = results(tmp_path_factory, "main"), results(tmp_path_factory, "main", **OFF)
    assert statuses_ok(off)
    assert_same(on, off)
    tol = on[ssc.key(("s4", "tol", "gs", 64)) + ".st"]
    assert 1 <= int(tol[1]) <= 64


@pytest.mark.parametrize("kernel", ["iso", "regular"])
def test_plain_isotropic_and_regular_kernel(tmp_path_factory, kernel):
    sw = {"EGS_ISO_LINSYM": "0"} if kernel == "iso" else {"EGS_ISO": "0"}
    on, off = results(tmp_path_factory, "solve", **sw), results(tmp_path_factory, "solve", **sw, **OFF)
    assert statuses_ok(on) and statuses_ok(off)
    for s in schedules(on, "solve"):
        assert s & capi.SCHED_STATIC and not s & capi.SCHED_LINSYM
        assert bool(s & capi.SCHED_ISO) == (kernel == "iso")
    assert_same(on, off)
    if kernel == "iso":   # the LINSYM launch keeps the plain isotropic kernel's bits (test_gpu_step_linsym.py)
        main = results(tmp_path_factory, "main")
        for k in on:
            if not k.endswith(".st"):
                assert on[k].tobytes() == main[k].tobytes(), k


def test_fp32_one_tile_per_workgroup(tmp_path_factory):
    on = results(tmp_path_factory, "f32", EGS_STEP_GROUP="1")
    off = results(tmp_path_factory, "f32", EGS_STEP_GROUP="1", **OFF)
    assert statuses_ok(on) and statuses_ok(off)
    assert all(s & capi.SCHED_STATIC and s & capi.SCHED_ISO and not s & capi.SCHED_LINSYM for s in schedules(on, "step"))
    assert_same(on, off)


_oracle = {}


def oracle(sc_name, method, sweeps):
    """lambda, accumulators, w and v6 of one step of the scene from the sequential oracle (computed once per case)."""
    ident = (sc_name, method, sweeps)
    if ident not in _oracle:
        sc = ssc.scene(sc_name)
        meth, omega = (orc.GAUSS_SEIDEL, 1.0) if method == "gs" else (orc.SOR, 1.5)
        Minv, f_ext = bench.host_mass_and_force(sc)
        J0, J1, is_eq, lo, hi, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
        s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
        rhs = orc.ode_rhs(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, err, ssc.DT, ssc.ERP)
        xf, af, _, _ = orc.fast_iterate(s, rhs, ssc.CFM, meth, max_iters=sweeps, tol=0.0, omega=omega)
        v6 = orc.velocity_update(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, xf, ssc.DT)
        _oracle[ident] = dict(lam=xf, acc=af, wres=orc.fast_wres(s, rhs, ssc.CFM, xf, af), v6=v6)
    return _oracle[ident]


@pytest.mark.parametrize("sc_name", ["s4", "s16", "uneven"])
@pytest.mark.parametrize("method", ["gs", "sor"])
def test_oracle_bits(tmp_path_factory, sc_name, method):
    on = results(tmp_path_factory, "main")
    for sweeps in ssc.SWEEPS[sc_name]:
        ref = oracle(sc_name, method, sweeps)
        for path in ("step", "solve"):
            k = ssc.key((sc_name, path, method, sweeps))
            for name in ("lam", "acc", "wres"):
                assert np.array_equal(on[k + "." + name].reshape(ref[name].shape), ref[name]), (k, name)
            if path == "step":
                assert np.abs(on[k + ".v6"] - ref["v6"]).max() <= 1e-12 * max(1.0, np.abs(ref["v6"]).max()), k
