"""CPU: the oracle's contact generation (oracle/collision.c) against the 50-digit statement of the geometry in
tests/collision_reference.py, on the five seeded families of rotated boxes with unequal sides: which pairs are
separated, which axis carries the normal, how deep, and the properties of every face contact -- decided independently
of the fp64 operation order.  This pins the oracle the device is held bit-equal to, and shows that the exclusion caps
are attainable by correct code.  Run with -s for the measured errors and counts."""
import ctypes as C

import numpy as np
import pytest

import collision_reference as ref
from oracle import oracle as orc


def collide_boxes_32(c1, R1, s1, c2, R2, s2):
    """orc.collide_boxes_info with room for 32 contacts, so that a pair with more than 16 would show."""
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (c1, R1, s1, c2, R2, s2)]
    out = np.zeros((32, 7)); code = C.c_int(0); info = np.zeros(4)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    n = orc.lib().orc_collide_boxes_info(*[ptr(x) for x in a], ptr(out), C.c_int(32), C.byref(code), ptr(info))
    return out[:n].copy(), code.value


@pytest.mark.parametrize("f", ref.FAMILIES)
def test_oracle_against_the_reference(f):
    p, R, side = ref.family(f)
    pairs, grounds = ref.family_reference(f)
    b0, b1, data = [], [], []
    for b in range(p.shape[0]):
        for c in orc.collide_box_ground(p[b], R[b], side[b]):
            b0.append(-1); b1.append(b); data.append(c)
    for i in range(p.shape[0]):
        for j in range(i + 1, p.shape[0]):     # ALL pairs: the ones outside `pairs` must come back empty
            cs, code = orc.collide_boxes(p[i], R[i], p[j], R[j], side[i], side[j])
            assert (code == 0) == (len(cs) == 0)
            for c in cs:
                b0.append(i); b1.append(j); data.append(c)
    tally = ref.Tally()
    ref.check_scene((pairs, grounds), b0, b1, np.array(data).reshape(-1, 7), tally, "family %d" % f)
    print("\n" + tally.line("oracle, family %d" % f))
    tally.assert_caps(f)


def test_every_code_and_every_aacount_class_occurs():
    """The families reach all fifteen axes as the deciding one, the fallback, and aacount 0, 1, 2 and 3 among the
    pairs whose properties are checked; no pair produces more than the 16 contacts the device's buffer holds."""
    codes, aacounts, most = set(), set(), 0
    for f in ref.FAMILIES:
        p, R, side = ref.family(f)
        for (i, j), r in ref.family_reference(f)[0].items():
            cs, code, axis, depth = orc.collide_boxes_info(p[i], R[i], p[j], R[j], side[i], side[j])
            cs32, code32 = collide_boxes_32(p[i], R[i], side[i], p[j], R[j], side[j])
            assert code32 == code and len(cs32) <= 16 and np.array_equal(cs32, cs)
            most = max(most, len(cs32))
            codes.add(code)
            if code and not r.excluded:
                aacounts.add(r.aacount)
    print("\ncodes %s, aacount classes %s, at most %d contacts per pair" % (sorted(codes), sorted(aacounts), most))
    assert codes == set(range(17))
    assert aacounts == {0, 1, 2, 3}
