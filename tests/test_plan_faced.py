"""CPU: Plan::faced (plan.h) and plan_faces_normals, what the fused step launch asks before a thread pair runs the four
contact points of a box face behind one barrier (step_face.hip).  The flag against its definition,
recomputed here from the planner's own tables (tile, lane, slots, level, period), on the chained scenes of
test_gpu_step_chain.py, on one C3 pile, on a pile with two contact points per face (chained, not faced) and on the lists
that are not chained; the normals' answer beside SHARE's; and which steady windows the cases of test_gpu_step_face.py
can reach.

A group is the plan lanes 128 W + 32 k + l (k = 0 .. 3) of a tile.  In g32p the last twelve boxes lack their fourth
contact: twelve groups of THREE members (in the lane-pair form's terms: twelve pairs of the second wavefront with an A
and no B)."""
import numpy as np
import pytest

import step_chain_cases as scc
import step_face_cases as sfc
import test_plan_chained as tpc
from eggshell_amd import capi, scenes

FACED = scc.CHAINED


def faced_by_definition(sc):
    """(faced, groups of four members, groups of fewer)"""
    tile, lane, slot0, slot1, level, period = tpc.tables(sc)
    ok = tpc.chained_by_definition(sc)[0] and all(int(p) % 4 == 0 for p in period)
    if not ok:
        return False, 0, 0
    groups, owner = {}, {}
    for i, (t, l) in enumerate(zip(tile, lane)):
        g = (int(t), int(l) // 128, int(l) % 32)
        groups.setdefault(g, {})[(int(l) % 128) // 32] = i
        blk = (int(level[i]) // 4) % (int(period[i]) // 4)
        for s in (int(slot0[i]), int(slot1[i])):
            if s != 0:                                            # slot 0 is the world: no accumulator
                owner.setdefault((int(t), blk, s), set()).add(g)
    ok = all(len(gs) == 1 for gs in owner.values())               # one group per block of four steps and slot
    whole = partial = 0
    for members in groups.values():
        ok = ok and sorted(members) == list(range(len(members)))  # member k only with member k - 1
        if not ok:
            break
        a = members[0]
        ok = ok and int(level[a]) % 4 == 0
        for k, i in members.items():
            ok = ok and slot0[i] == slot0[a] and slot1[i] == slot1[a] and level[i] == level[a] + k
            ok = ok and sc["body0"][i] == sc["body0"][a] and sc["body1"][i] == sc["body1"][a]
        whole += len(members) == 4
        partial += len(members) < 4
    return bool(ok), whole, partial


def flag(sc):
    return capi.debug_plan_faced(sc["p"].shape[0], sc["body0"], sc["body1"])


def normals(sc):
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    return capi.debug_plan_share(n, b0, b1, sc["data"]), capi.debug_plan_face_normals(n, b0, b1, sc["data"])


@pytest.mark.parametrize("name", FACED)
def test_flag_is_the_definition(name):
    sc = scc.scene(name)
    want, whole, partial = faced_by_definition(sc)
    assert want and flag(sc)
    if name == "g32p":
        assert (whole, partial) == (20, 12)
        assert sorted(len(m) for m in sfc.groups(sc)) == [3] * 12 + [4] * 20
    else:
        assert partial == 0 and 4 * whole == sc["body0"].shape[0]
    assert normals(sc) == (True, True)


def test_a_c3_pile_is_faced():
    sc = scenes.box_stack(16, 16, 16)
    want, whole, partial = faced_by_definition(sc)
    assert want and (whole, partial) == (4096, 0)
    assert flag(sc) and normals(sc) == (True, True)


def test_two_contact_points_per_face_are_chained_not_faced():
    """8 x 4 x 2 with contacts 0 and 1 of every face: period 4, and a group's member 2 is another face."""
    sc = sfc.scene("h2half")
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    assert capi.debug_plan_pairable(n, b0, b1) and capi.debug_plan_chained(n, b0, b1)
    want, _, _ = faced_by_definition(sc)
    assert not want and not flag(sc)
    assert normals(sc) == (True, False)
    g = next(m for m in sfc.groups(sc) if len(m) > 2)
    assert (b0[g[2]], b1[g[2]]) != (b0[g[0]], b1[g[0]])


@pytest.mark.parametrize("name", scc.NOT_CHAINED)
def test_a_plan_that_is_not_chained_is_not_faced(name):
    sc = scc.scene(name)
    assert not flag(sc) and normals(sc) == (False, False)
    if name in scc.PAIRABLE_NOT_CHAINED:
        assert not faced_by_definition(sc)[0]


@pytest.mark.parametrize("name", ["g32:zeroCD", "h2:zeroCD", "two:tiltCD", "g32p:tiltC"])
def test_a_second_normal_in_the_upper_pair_keeps_share(name):
    """A group's C and D (a group of three: its C) carry another normal than A and B, in value or in the sign of a zero
    only: every lane pair still carries one normal, the group does not."""
    sc = sfc.scene(name)
    assert flag(sc) and normals(sc) == (True, False)


@pytest.mark.parametrize("name", ["g32:zeroB", "h2:zeroD"])
def test_a_second_normal_inside_a_pair_takes_both_away(name):
    sc = sfc.scene(name)
    assert flag(sc) and normals(sc) == (False, False)


def test_one_tilted_normal_everywhere_is_one_normal():
    assert normals(sfc.scene("h2:tilt")) == (True, True)


def test_null_data_and_empty_lists():
    import ctypes as C
    sc = scc.scene("g32")
    b0, b1 = capi._i32(sc["body0"]), capi._i32(sc["body1"])
    out = C.c_int32(7)
    st = capi.load().egs_debug_plan_face_normals(C.c_int32(sc["p"].shape[0]), C.c_int32(b0.shape[0]), capi._p(b0), capi._p(b1),
                                                 None, C.byref(out))
    assert st != capi.OK
    none = np.zeros(0, np.int32)
    assert not capi.debug_plan_faced(1, none, none)
    assert not capi.debug_plan_face_normals(1, none, none, np.zeros((0, 7)))


def test_the_cases_cover_the_windows():
    """CPU arithmetic only.  The FACE form trims the steady window [t_s, t_e) of a forward launch to whole blocks of four
    steps from a step = 0 (mod 4).  On a faced plan whose deepest groups are whole the depth and the period are
    multiples of 4, and so are t_s = depth and t_e = min(P (sweeps + 1), depth + P sweeps): remainder 0 is the only one
    these depths and periods produce, which is asserted, and the cases hold an empty window, one block, and many, with and
    without steps left to the general loop before (a window that is not empty) and after (a tile deeper than its period)."""
    seen = set()
    for name in sfc.GPU_SCENES:
        sc = sfc.scene(name)
        tt = capi.debug_plan_timetable(sc["p"].shape[0], sc["body0"], sc["body1"], 256)
        for depth, period in set(zip(tt["depth"].tolist(), tt["period"].tolist())):
            assert depth % 4 == 0 and period % 4 == 0
            for sweeps in sfc.SWEEPS:
                t_s, t_e, t_end = scc.steady_window("gs", depth, period, sweeps)
                assert t_s % 4 == 0 and (t_e - t_s) % 4 == 0 and t_end % 4 == 0
                first = (t_s + 3) // 4 * 4
                length = (t_e - first) - (t_e - first) % 4 if t_e > first else 0
                seen.add(("start", first % 4))
                seen.add(("length", length % 4))
                seen.add("empty" if length == 0 else "one block" if length == 4 else "blocks")
                seen.add("fill" if first > 0 else "no fill")
                seen.add("drain" if t_end > t_e else "no drain")
    assert seen == {("start", 0), ("length", 0), "empty", "one block", "blocks", "fill", "no fill", "drain", "no drain"}, seen
