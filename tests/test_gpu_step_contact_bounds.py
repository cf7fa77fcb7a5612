"""GPU (-m gpu): the fused step's sweep projects with a contact's bounds as literals (rows 0 and 1 to [-1, 1], row 2
to [0, +inf)) and holds side 0's angular products of B in registers.  Neither changes an operand or a rounding, so
lambda, w and the accumulators must keep every bit of

  * the sequential CPU oracle, which projects with the assembled lo / hi (the velocity update within 1e-12 relative,
    as test_gpu_step_steady.py compares it: its sums are ordered otherwise),
  * assemble + solve of the same build: the plain LINSYM launch, which still reads its bounds from memory,

on one partly filled tile with side-1-only ground lanes and on one full 256-lane tile, at rest and with random body
velocities, GS and backward SOR at 1, 3 and 10 sweeps (step_contact_bounds_cases.py).  The oracle's lambda must itself
sit on every branch of the projection -- friction at +1, at -1 and inside, normal at 0 and above -- or the comparison
would not exercise the clamps.  A list that holds any joint keeps the launch it had: no fused assembly, oracle bits.
Every environment runs in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import step_contact_bounds_cases as cbc
from eggshell_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SWITCHES = ("EGS_STEP_STEADY", "EGS_ISO_LINSYM", "EGS_STEP_GROUP", "EGS_FUSED_ASSEMBLY", "EGS_STEP_DEFER_SYSTEM")

_results = {}


def results(tmp_path_factory, group):
    """Every output of every case of `group` from one fresh process (cached)."""
    if group not in _results:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(cbc.BASE_ENV)
        path = str(tmp_path_factory.mktemp("bounds") / "out.npz")
        r = subprocess.run([sys.executable, os.path.abspath(cbc.__file__), group, path], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(path) as z:
            _results[group] = {k: z[k] for k in z.files}
    return _results[group]


_oracle = {}


def oracle(sc_name, method, sweeps):
    """lambda, accumulators, w and v6 of one step of the scene from the sequential oracle (computed once per case)."""
    ident = (sc_name, method, sweeps)
    if ident not in _oracle:
        sc = cbc.scene(sc_name)
        meth, omega = (orc.GAUSS_SEIDEL, 1.0) if method == "gs" else (orc.SOR, 1.5)
        Minv, f_ext = bench.host_mass_and_force(sc)
        J0, J1, is_eq, lo, hi, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
        s = orc.Sys(Minv, sc["body0"], sc["body1"], J0, J1, is_eq, lo, hi)
        rhs = orc.ode_rhs(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, err, cbc.DT, cbc.ERP)
        xf, af, _, _ = orc.fast_iterate(s, rhs, cbc.CFM, meth, max_iters=sweeps, tol=0.0, omega=omega)
        v6 = orc.velocity_update(sc["v"], sc["w"], Minv, f_ext, s.body0, s.body1, J0, J1, xf, cbc.DT)
        _oracle[ident] = dict(lam=xf, acc=af, wres=orc.fast_wres(s, rhs, cbc.CFM, xf, af), v6=v6)
    return _oracle[ident]


def outcomes(lam):
    """How many rows of lambda sit on each branch of a contact's projection."""
    lam = np.asarray(lam).reshape(-1, 3)
    f, n = lam[:, :2], lam[:, 2]
    return dict(plus=int((f == 1.0).sum()), minus=int((f == -1.0).sum()), inside=int((np.abs(f) < 1.0).sum()),
                zero=int((n == 0.0).sum()), positive=int((n > 0.0).sum()))


def test_reference_takes_every_branch():
    total = dict(plus=0, minus=0, inside=0, zero=0, positive=0)
    for sc_name in cbc.CONTACT_SCENES:
        for method in ("gs", "sor"):
            for sweeps in cbc.SWEEPS:
                for k, v in outcomes(oracle(sc_name, method, sweeps)["lam"]).items():
                    total[k] += v
    print(total)
    assert all(v >= 10 for v in total.values()), total


def test_fused_launch_runs(tmp_path_factory):
    res = results(tmp_path_factory, "contacts")
    fused = capi.SCHED_STATIC | capi.SCHED_ISO | capi.SCHED_LINSYM | capi.SCHED_FUSED_ASSEMBLY | capi.SCHED_DEFERRED_SYSTEM
    plain = capi.SCHED_STATIC | capi.SCHED_ISO | capi.SCHED_LINSYM
    for case in cbc.cases("contacts"):
        st = res[cbc.key(case) + ".st"]
        assert int(st[0]) == capi.OK, case
        if case[1] == "step":
            assert int(st[2]) & fused == fused, case
        else:
            assert int(st[2]) & plain == plain and not int(st[2]) & capi.SCHED_FUSED_ASSEMBLY, case


@pytest.mark.parametrize("sc_name", cbc.CONTACT_SCENES)
@pytest.mark.parametrize("method", ["gs", "sor"])
def test_oracle_bits(tmp_path_factory, sc_name, method):
    res = results(tmp_path_factory, "contacts")
    for sweeps in cbc.SWEEPS:
        ref = oracle(sc_name, method, sweeps)
        k = cbc.key((sc_name, "step", method, sweeps))
        for name in ("lam", "acc", "wres"):
            assert np.array_equal(res[k + "." + name].reshape(ref[name].shape), ref[name]), (k, name)
        assert np.abs(res[k + ".v6"] - ref["v6"]).max() <= 1e-12 * max(1.0, np.abs(ref["v6"]).max()), k


@pytest.mark.parametrize("sc_name", cbc.CONTACT_SCENES)
@pytest.mark.parametrize("method", ["gs", "sor"])
def test_bounds_from_memory(tmp_path_factory, sc_name, method):
    """The fused launch against assemble + solve of the same build."""
    res = results(tmp_path_factory, "contacts")
    for sweeps in cbc.SWEEPS:
        a, b = cbc.key((sc_name, "step", method, sweeps)), cbc.key((sc_name, "solve", method, sweeps))
        for name in ("lam", "acc", "wres"):
            x, y = res[a + "." + name], res[b + "." + name]
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (a, name)


@pytest.mark.parametrize("sc_name", cbc.JOINT_SCENES)
def test_joints_keep_their_launch(tmp_path_factory, sc_name):
    res = results(tmp_path_factory, "joints")
    for method in ("gs", "sor"):
        for sweeps in cbc.SWEEPS:
            k = cbc.key((sc_name, "step", method, sweeps))
            st = res[k + ".st"]
            assert int(st[0]) == capi.OK, k
            assert not int(st[2]) & capi.SCHED_FUSED_ASSEMBLY, k
            ref = oracle(sc_name, method, sweeps)
            for name in ("lam", "acc", "wres"):
                assert np.array_equal(res[k + "." + name].reshape(ref[name].shape), ref[name]), (k, name)
