"""CPU: Plan::chained (plan.h), what the fused step launch asks of a tile plan before a lane pair keeps its two bodies'
accumulators in registers from the first of its two updates to the second.  The flag against its definition, recomputed
here from the planner's own tables (tile, lane, slots, level, period), on the topologies of test_gpu_step_chain.py and
on one C3 pile; and that the cases of the GPU test reach every shape of the steady window they can."""
import numpy as np
import pytest

import step_chain_cases as scc
from eggshell_amd import capi, scenes


def tables(sc):
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    tt = capi.debug_plan_timetable(n, b0, b1, 256)
    assert tt["runs"] is False
    sl = capi.debug_plan_slots(n, b0, b1, 256)
    tile = capi.debug_plan(n, b0, b1, 256)["cons_tile"]
    assert (tile >= 0).all() and (sl["lane"] >= 0).all()      # no oversize island in these scenes
    return tile, sl["lane"], sl["slot0"], sl["slot1"], tt["level"], tt["period"]


def chained_by_definition(sc):
    """(chained, thread pairs with an A and a B, thread pairs with an A alone)"""
    tile, lane, slot0, slot1, level, period = tables(sc)
    halves, at = {}, {}
    for i, (t, l) in enumerate(zip(tile, lane)):
        halves.setdefault((int(t), int(l) // 32), set()).add(int(level[i]) % int(period[i]))
        at[(int(t), int(l))] = i
    ok = all(len(s) == 1 for s in halves.values())            # pairable
    ok = ok and all(int(p) % 2 == 0 for p in period)
    both = alone = 0
    for (t, l), a in at.items():
        if l % 64 >= 32:
            ok = ok and (t, l - 32) in at                       # no B without its A
            continue
        ok = ok and int(level[a]) % 2 == 0
        b = at.get((t, l + 32))
        if b is None:
            alone += 1
            continue
        both += 1
        ok = ok and slot0[a] == slot0[b] and slot1[a] == slot1[b] and level[b] == level[a] + 1
        # the same LDS slots of one tile are the same bodies
        ok = ok and sc["body0"][a] == sc["body0"][b] and sc["body1"][a] == sc["body1"][b]
    return bool(ok), both, alone


@pytest.mark.parametrize("name", scc.CHAINED + scc.NOT_CHAINED)
def test_flag_is_the_definition(name):
    sc = scc.scene(name)
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    got = capi.debug_plan_chained(n, b0, b1)
    if name in scc.spc.NOT_PAIRABLE:
        # `chain` has an oversize-free plan too, but none of the three is pairable, which the definition starts from
        assert not capi.debug_plan_pairable(n, b0, b1) and not got
        return
    want, both, alone = chained_by_definition(sc)
    assert got == want
    assert want == (name in scc.CHAINED)
    assert capi.debug_plan_pairable(n, b0, b1)
    if name == "g32p":
        assert (both, alone) == (52, 12)
    elif want:
        assert alone == 0 and 2 * both == b0.shape[0]


def test_a_c3_pile_is_chained():
    sc = scenes.box_stack(16, 16, 16)
    want, both, alone = chained_by_definition(sc)
    assert want and alone == 0 and both == 8192
    assert capi.debug_plan_chained(sc["p"].shape[0], sc["body0"], sc["body1"])


def test_why_the_other_two_are_not():
    """flat64: period 1, and a pair's A and B are different boxes at one level; odd3: period 3."""
    for name, period in (("flat64", 1), ("odd3", 3)):
        sc = scc.scene(name)
        tile, lane, slot0, slot1, level, per = tables(sc)
        assert set(int(p) for p in per) == {period}
    sc = scc.scene("flat64")
    tile, lane, slot0, slot1, level, per = tables(sc)
    assert sorted(int(l) for l in lane) == list(range(64)) and not level.any()
    assert len(set(int(s) for s in slot1)) == 64


def test_the_cases_cover_the_windows():
    """CPU arithmetic only: among the cases the steady window is empty, starts on an even and on an odd step, and has an
    even and an odd length; once its start is rounded up to an even step the rest is even everywhere
    (test_gpu_step_chain.py says why)."""
    seen = set()
    for name in scc.CHAINED:
        sc = scc.scene(name)
        tt = capi.debug_plan_timetable(sc["p"].shape[0], sc["body0"], sc["body1"], 256)
        for depth, period in set(zip(tt["depth"].tolist(), tt["period"].tolist())):
            assert depth % 2 == 0 and period % 2 == 0
            for method in ("gs", "sor"):
                for sweeps in scc.SWEEPS:
                    t_s, t_e, _ = scc.steady_window(method, depth, period, sweeps)
                    if t_e == t_s:
                        seen.add("empty")
                        continue
                    seen.add("odd entry" if t_s % 2 else "even entry")
                    seen.add("odd length" if (t_e - t_s) % 2 else "even length")
                    first = t_s + t_s % 2
                    assert (t_e - first) % 2 == 0
                    seen.add("iterations" if t_e > first else "trimmed to nothing")
    assert seen >= {"empty", "odd entry", "even entry", "odd length", "even length", "iterations"}, seen


def test_an_empty_list_is_not_chained():
    assert not capi.debug_plan_chained(1, np.zeros(0, np.int32), np.zeros(0, np.int32))
