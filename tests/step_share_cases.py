"""The scenes of test_gpu_step_share.py and test_plan_share.py: the chained piles of step_chain_cases.py, whose two
contacts of every thread pair of the lane-pair form carry one normal (the piles' (0, 0, 1)), and variants of them
whose descriptors differ in the normals alone.

  <name>           the pile as step_chain_cases.py builds it: one normal per face
  <name>:tilt      every contact carries the unit normal (0.1, 0.2, 1) / |..|: one normal per face still, and Rn, the
                   linear Jacobian block, has no zero entry
  <name>:zero      the B of one thread pair carries (-0.0, 0, 1): the same normal in value, not in bits
  <name>:tiltB     the B of one thread pair carries the tilted normal
  g32p:alone       the A of a thread pair WITHOUT a B carries the tilted normal: no condition

pairs(sc) lists the thread pairs (A, B or None) as constraint numbers, from the planner's own tables."""
import numpy as np

import step_chain_cases as scc
from eggshell_amd import capi

TILT = np.array([0.1, 0.2, 1.0]) / np.sqrt(0.1 * 0.1 + 0.2 * 0.2 + 1.0)
# the smallest chained scenes: the 32-box pile, the same with twelve A-alone pairs, 8 x 4 x 2, two tiles of depth 16 / 64
SCENES = ("g32", "g32p", "h2", "two")


def pairs(sc):
    """[(A, B or None)] for every thread pair of the lane-pair form that holds a constraint: A = plan lane 64 w + l and
    B = plan lane 64 w + 32 + l of one tile, l < 32."""
    n, b0, b1 = sc["p"].shape[0], sc["body0"], sc["body1"]
    tile = capi.debug_plan(n, b0, b1, 256)["cons_tile"]
    lane = capi.debug_plan_slots(n, b0, b1, 256)["lane"]
    assert (tile >= 0).all() and (lane >= 0).all()
    at = {(int(t), int(l)): i for i, (t, l) in enumerate(zip(tile, lane))}
    out = []
    for (t, l), a in sorted(at.items()):
        if l % 64 < 32:
            out.append((a, at.get((t, l + 32))))
    return out


def scene(name):
    base, _, variant = name.partition(":")
    sc = dict(scc.scene(base))
    if not variant:
        return sc
    data = sc["data"].copy()
    both = [(a, b) for a, b in pairs(sc) if b is not None]
    alone = [a for a, b in pairs(sc) if b is None]
    if variant == "tilt":
        data[:, 3:6] = TILT
    elif variant == "zero":
        a, b = both[len(both) // 2]
        assert data[b, 3:6].tobytes() == np.array([0.0, 0.0, 1.0]).tobytes()
        data[b, 3:6] = (-0.0, 0.0, 1.0)
    elif variant == "tiltB":
        a, b = both[len(both) // 3]
        data[b, 3:6] = TILT
    elif variant == "alone":
        data[alone[len(alone) // 2], 3:6] = TILT
    else:
        raise ValueError(name)
    sc["data"] = data
    return sc
