"""The scenes of test_gpu_step_face.py and test_plan_faced.py: the chained piles of step_chain_cases.py, whose plan is
also faced (the four constraints of every thread pair of the FACE form are the four contact points of one box face:
plan.h), and variants of them.

  <name>          the pile as step_chain_cases.py builds it: one normal per face
  h2half          8 x 4 x 2 with contact points 0 and 1 of every face only: chained, not faced
  <name>:tilt     every contact carries the unit normal (0.1, 0.2, 1) / |..|
  <name>:zeroCD   members C and D of one whole group carry (-0.0, 0, 1): one normal per lane pair, two in the group
  <name>:tiltCD   ... carry the tilted normal
  <name>:zeroD    member D alone of one whole group carries (-0.0, 0, 1): two normals in a lane pair
  <name>:zeroB    member B alone
  g32p:tiltC      member C of a group of three carries the tilted normal

groups(sc) lists the groups as constraint numbers in member order, from the planner's own tables."""
import numpy as np

import step_chain_cases as scc
from eggshell_amd import capi

TILT = np.array([0.1, 0.2, 1.0]) / np.sqrt(0.1 * 0.1 + 0.2 * 0.2 + 1.0)
# one idle wavefront at period 4; groups of three; a full tile of period 8; depths 16 and 64; periods 4 and 8
GPU_SCENES = ("g32", "g32p", "h2", "two", "mixed")
# the accumulation alone plus one block, two, .. (an empty window on `two`'s deep tile up to 7), and long windows
SWEEPS = (1, 2, 3, 4, 9, 10)


def groups(sc):
    """[[A, B, ..]] for every thread pair of the FACE form that holds a constraint: member k = plan lane
    128 W + 32 k + l of one tile, l < 32 (a missing member ends the list: what follows it would not be its group's)."""
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    tile = capi.debug_plan(n, b0, b1, 256)["cons_tile"]
    lane = capi.debug_plan_slots(n, b0, b1, 256)["lane"]
    assert (tile >= 0).all() and (lane >= 0).all()
    at = {(int(t), int(l)): i for i, (t, l) in enumerate(zip(tile, lane))}
    out = []
    for (t, l), a in sorted(at.items()):
        if l % 128 < 32:
            members = [a]
            while len(members) < 4 and (t, l + 32 * len(members)) in at:
                members.append(at[(t, l + 32 * len(members))])
            out.append(members)
    return out


def scene(name):
    base, _, variant = name.partition(":")
    if base == "h2half":
        sc = scc.keep_contacts(scc.scene("h2"), 2)
    else:
        sc = dict(scc.scene(base))
    if not variant:
        return sc
    data = sc["data"].copy()
    whole = [g for g in groups(sc) if len(g) == 4]
    pick = whole[len(whole) // 2]
    zero = (-0.0, 0.0, 1.0)
    if variant == "tilt":
        data[:, 3:6] = TILT
    elif variant in ("zeroCD", "tiltCD"):
        assert data[pick[2], 3:6].tobytes() == np.array([0.0, 0.0, 1.0]).tobytes()
        data[pick[2], 3:6] = data[pick[3], 3:6] = zero if variant == "zeroCD" else TILT
    elif variant == "zeroD":
        data[pick[3], 3:6] = zero
    elif variant == "zeroB":
        data[pick[1], 3:6] = zero
    elif variant == "tiltC":
        three = [g for g in groups(sc) if len(g) == 3]
        data[three[len(three) // 2][2], 3:6] = TILT
    else:
        raise ValueError(name)
    sc["data"] = data
    return sc
