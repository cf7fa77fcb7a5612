"""CPU: what the SHARE form of the fused step launch asks beyond a chained plan (plan.h: plan_shares_normals;
egs_debug_plan_share): the two contacts of every thread pair of the lane-pair form carry the same normal as bit
patterns.  The entry against the definition, recomputed here in numpy from the planner's own tables, on the chained
topologies of test_plan_chained.py with one normal per face, with one pair's B normal changed in the sign of a zero and
tilted, with a tilted A that has no B, and on pairable lists whose plan is not chained."""
import numpy as np
import pytest

import step_chain_cases as scc
import step_share_cases as ssc
from eggshell_amd import capi


def share_by_definition(sc):
    """Chained, and data[7 i + 3 .. 5] of A and of B equal as integers wherever a thread pair holds both."""
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    if not capi.debug_plan_chained(n, b0, b1):
        return False
    bits = np.ascontiguousarray(sc["data"], dtype=np.float64).reshape(-1, 7)[:, 3:6].copy().view(np.uint64)
    return all(b is None or (bits[a] == bits[b]).all() for a, b in ssc.pairs(sc))


def entry(sc):
    return capi.debug_plan_share(sc["p"].shape[0], sc["body0"], sc["body1"], sc["data"])


@pytest.mark.parametrize("name", scc.CHAINED)
def test_one_normal_per_face_shares(name):
    for variant in ("", ":tilt"):
        sc = ssc.scene(name + variant)
        assert share_by_definition(sc) and entry(sc), name + variant


@pytest.mark.parametrize("variant", ["zero", "tiltB"])
@pytest.mark.parametrize("name", scc.CHAINED)
def test_one_pair_with_two_normals_does_not(name, variant):
    sc, plain = ssc.scene(name + ":" + variant), ssc.scene(name)
    changed = np.flatnonzero((sc["data"] != plain["data"]).any(axis=1) |
                             (np.signbit(sc["data"]) != np.signbit(plain["data"])).any(axis=1))
    assert changed.shape == (1,)                               # one contact, and it is the B of a pair with an A
    assert any(b == changed[0] for a, b in ssc.pairs(sc))
    if variant == "zero":                                      # equal as doubles, not as integers
        assert np.array_equal(sc["data"], plain["data"])
    assert not share_by_definition(sc) and not entry(sc)


def test_an_a_without_a_b_asks_nothing():
    sc, plain = ssc.scene("g32p:alone"), ssc.scene("g32p")
    changed = np.flatnonzero((sc["data"] != plain["data"]).any(axis=1))
    assert changed.shape == (1,) and (int(changed[0]), None) in ssc.pairs(sc)
    assert share_by_definition(sc) and entry(sc)


@pytest.mark.parametrize("name", scc.PAIRABLE_NOT_CHAINED)
def test_an_unchained_list_is_not_offered_the_form(name):
    sc = scc.scene(name)
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    assert capi.debug_plan_pairable(n, b0, b1) and not capi.debug_plan_chained(n, b0, b1)
    assert len(set(sc["data"][:, 3:6].tobytes()[i:i + 24] for i in range(0, 24 * b0.shape[0], 24))) == 1   # one normal
    assert not share_by_definition(sc) and not entry(sc)


def test_an_empty_list_does_not_share():
    assert not capi.debug_plan_share(1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)))


def test_a_list_without_descriptors_is_refused():
    sc = scc.scene("g32")
    lib = capi.load()
    import ctypes as C
    out = C.c_int32(0)
    b0, b1 = capi._i32(sc["body0"]), capi._i32(sc["body1"])
    st = lib.egs_debug_plan_share(C.c_int32(sc["p"].shape[0]), C.c_int32(b0.shape[0]), capi._p(b0), capi._p(b1), None,
                                  C.byref(out))
    assert st == capi.ERR_INVALID
