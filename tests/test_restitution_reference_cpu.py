"""CPU: the restitution model's 50-digit reference and its fp64 twin (tests/restitution_reference.py), and the symbols
the feature adds to the library."""
import collections
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import model_reference as mr
import restitution_reference as rr
from eggshell_amd import capi
from oracle import oracle as orc


def test_generated_cases_cover_every_decision():
    count = collections.Counter()
    for cid in rr.IDS:
        case, rest, vth, J0, J1, err, rhs, what = rr.generated(cid)
        count.update(what)
        assert len(what) == case["kind"].shape[0]
    print(dict(count))
    assert len(rr.IDS) == 6 and sum(count.values()) == 1 + 1 + 1 + 40 + 257 + 513
    for k in ("joint", "off", "slow", "floor", "bounce"):
        assert count[k] > 0, k
    # both world sides and two-body contacts bounce; every coefficient is drawn
    case, rest, _, _, _, _, _, what = rr.generated("m513")
    sides = {(case["body0"][i] < 0, case["body1"][i] < 0) for i, w in enumerate(what) if w == "bounce"}
    assert sides == {(True, False), (False, True), (False, False)}
    assert set(rest) == set(rr.COEFFICIENTS)


@pytest.mark.parametrize("cid", rr.IDS)
def test_twin_off_is_the_oracle_and_on_is_within_the_reference_bound(cid):
    case, rest, vth, J0, J1, err, rhs, what = rr.generated(cid)
    off = rr.twin_rhs(case, J0, J1, err, None, vth)[0]
    want = orc.ode_rhs(case["v"], case["w"], case["Minv"], case["f_ext"], case["body0"], case["body1"], J0, J1, err, case["dt"], case["erp"])
    assert off.tobytes() == np.asarray(want).reshape(-1).tobytes()
    changed = np.nonzero(off != rhs)[0]
    assert set(changed) <= {3 * i + 2 for i, w in enumerate(what) if w == "bounce"}
    asm = mr.assemble_reference(case)
    ref, rwhat = rr.rhs_reference(case, asm, rest, vth)
    assert rwhat == what
    worst, where = ref.worst(rhs)
    print("%s: twin max error / tolerance %.3g at row %d" % (cid, worst, where))
    assert worst <= 1.0


@pytest.mark.parametrize("e, vz, depth, wins", [(0.8, -2.0, 1e-3, True), (1.0, -1.0, 0.0, True), (1.7, -0.7, 2e-3, True),
                                                 (0.0, -2.0, 1e-3, False), (0.5, -0.01, 5e-3, False), (0.8, -0.2, 1e-3, None)])
def test_central_impact_on_the_reference(e, vz, depth, wins):
    """v_z' = -e v_z to 1e-30 where the bounce wins; otherwise (the floor wins, or below the threshold vth = 0.5: the
    last case) the value without restitution."""
    dt, erp, vth = 5e-3, 0.2, 0.5 if wins is None else 0.0
    got, _, _, what, lam = rr.impact_reference(1.3, vz, depth, e, vth, dt, erp)
    plain = rr.impact_reference(1.3, vz, depth, None, 0.0, dt, erp)[0]
    with mp.workdps(mr.DPS):
        if wins:
            assert what == "bounce" and lam > 0
            want = -mp.mpf(float(e)) * mp.mpf(float(vz))
            assert abs(got - want) <= mp.mpf("1e-30") * max(abs(want), 1)
        else:
            assert what == ("slow" if wins is None else "floor")
            assert got == plain
            assert abs(plain - mp.mpf(float(erp)) * mp.mpf(float(depth)) / mp.mpf(float(dt))) <= mp.mpf("1e-30")


def test_library_exports_and_wrappers():
    lib = capi.load()
    for name in ("egs_problem_set_restitution", "egs_world_set_restitution"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert callable(capi.Problem.set_restitution) and callable(capi.World.set_restitution)
    assert lib.egs_problem_set_restitution(None, None, C.c_double(0.0)) == capi.ERR_INVALID
    assert lib.egs_world_set_restitution(None, 1, None, C.c_double(0.0)) == capi.ERR_INVALID
