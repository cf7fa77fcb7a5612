"""CPU: Plan::pairable (plan.h), what the fused step launch asks of a tile plan before it runs an update on a lane pair.
The flag against its definition, recomputed here from the planner's own tables (lane, tile, level, period), on the
topologies of test_gpu_step_pair.py."""
import numpy as np
import pytest

import step_pair_cases as spc
from eggshell_amd import capi


def pairable_by_definition(sc):
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    tt = capi.debug_plan_timetable(n, b0, b1, 256)
    assert tt["runs"] is False
    lane = capi.debug_plan_slots(n, b0, b1, 256)["lane"]
    tile = capi.debug_plan(n, b0, b1, 256)["cons_tile"]
    assert (tile >= 0).all() and (lane >= 0).all()      # no oversize island in these scenes
    phases = {}
    for t, l, lv, p in zip(tile, lane, tt["level"], tt["period"]):
        phases.setdefault((int(t), int(l) // 32), set()).add(int(lv) % int(p))
    return all(len(s) == 1 for s in phases.values()), phases


@pytest.mark.parametrize("name", spc.PAIRABLE + spc.NOT_PAIRABLE)
def test_flag_is_the_definition(name):
    sc = spc.scene(name)
    want, _ = pairable_by_definition(sc)
    assert capi.debug_plan_pairable(sc["p"].shape[0], sc["body0"], sc["body1"]) == want
    assert want == (name in spc.PAIRABLE)


def test_layouts_the_gpu_test_relies_on():
    """g32 fills two wavefronts and leaves two idle; g32p's last pairs have an A and no B; `two` spans two tiles."""
    def lanes_per_half(name):
        sc = spc.scene(name)
        lane = capi.debug_plan_slots(sc["p"].shape[0], sc["body0"], sc["body1"], 256)["lane"]
        tile = capi.debug_plan(sc["p"].shape[0], sc["body0"], sc["body1"], 256)["cons_tile"]
        count = {}
        for t, l in zip(tile, lane):
            count[(int(t), int(l) // 32)] = count.get((int(t), int(l) // 32), 0) + 1
        return count
    assert lanes_per_half("g32") == {(0, h): 32 for h in range(4)}
    assert lanes_per_half("g32p") == {(0, 0): 32, (0, 1): 32, (0, 2): 32, (0, 3): 20}
    assert lanes_per_half("two") == {(t, h): 32 for t in range(2) for h in range(8)}


def test_an_empty_list_is_not_pairable_and_a_lone_contact_is():
    assert not capi.debug_plan_pairable(1, np.zeros(0, np.int32), np.zeros(0, np.int32))
    # one ground contact: one lane, one phase -- pairable by the definition, if pointless
    assert capi.debug_plan_pairable(1, np.array([-1], np.int32), np.array([0], np.int32))
