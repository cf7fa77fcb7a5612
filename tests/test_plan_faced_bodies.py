"""CPU: what the staged prologue of the FACE form (step_face.hip: step_solve_face_kernel) relies on.  It takes the two
body numbers of a thread pair's group ONCE, from member A's slots, and loads those bodies' state once for both
constraints the lane owns.  That is right only if every member of every group has A's body0 and A's body1, side for
side -- which Plan::faced promises through the slots.  Here it is read off the planner's debug tables alone (tile and
lane per constraint, step_face_cases.groups), against the lists' own body numbers, on every faced scene the GPU tests
use and on one C3 pile of the benchmark; and the lists that must not take the form are not faced."""
import numpy as np
import pytest

import step_chain_cases as scc
import step_face_cases as sfc
from eggshell_amd import capi, scenes

FACED = tuple(dict.fromkeys(scc.CHAINED + sfc.GPU_SCENES)) + ("g32:tilt", "h2:tilt", "g32p:tilt")


def faced(sc):
    return capi.debug_plan_faced(sc["p"].shape[0], sc["body0"], sc["body1"])


def assert_groups_share_bodies(sc):
    b0, b1 = np.asarray(sc["body0"]), np.asarray(sc["body1"])
    groups = sfc.groups(sc)
    assert sorted(i for g in groups for i in g) == list(range(b0.shape[0]))     # every constraint is some group's member
    slots = capi.debug_plan_slots(sc["p"].shape[0], b0, b1, 256)
    for g in groups:
        a = g[0]
        assert (b0[g] == b0[a]).all() and (b1[g] == b1[a]).all(), g
        # ... and the slots the kernel reads them through are A's, with the world (no body) at slot 0 on either side
        assert (slots["slot0"][g] == slots["slot0"][a]).all() and (slots["slot1"][g] == slots["slot1"][a]).all(), g
        assert (slots["slot0"][a] == 0) == (b0[a] < 0) and (slots["slot1"][a] == 0) == (b1[a] < 0), g
    return groups


@pytest.mark.parametrize("name", FACED)
def test_every_member_has_the_first_members_bodies(name):
    sc = sfc.scene(name)
    assert faced(sc)
    groups = assert_groups_share_bodies(sc)
    sizes = sorted(set(len(g) for g in groups))
    assert sizes == ([3, 4] if name.startswith("g32p") else [4])


def test_a_c3_pile_of_the_benchmark():
    sc = scenes.box_stack(16, 16, 16, jitter=1e-3, seed=1)
    assert faced(sc)
    groups = assert_groups_share_bodies(sc)
    assert len(groups) == 4096 and all(len(g) == 4 for g in groups)
    # both kinds of group: a ground contact has no body on side 0, a contact between boxes has one on both
    kinds = set((int(sc["body0"][g[0]]) >= 0, int(sc["body1"][g[0]]) >= 0) for g in groups)
    assert kinds == {(False, True), (True, True)}


@pytest.mark.parametrize("name", ("h2half",) + scc.NOT_CHAINED)
def test_lists_that_are_not_faced(name):
    assert not faced(sfc.scene(name))


def test_two_contact_points_per_face_would_break_the_precondition():
    """Why h2half must not take the form: a group's third member there is another face, of other bodies."""
    sc = sfc.scene("h2half")
    b0, b1 = sc["body0"], sc["body1"]
    assert any(len(g) > 2 and (b0[g[2]], b1[g[2]]) != (b0[g[0]], b1[g[0]]) for g in sfc.groups(sc))
