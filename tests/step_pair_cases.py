"""The scenes of test_gpu_step_pair.py and test_plan_pairable.py: contact piles whose 256-lane tile plan is pairable
(every half-wavefront of lanes idle or in one phase of the timetable: plan.h), and lists whose plan is not.

Pairable, from the smallest pile up (lanes per half-wavefront in brackets, as the planner lays them out):
  g32   8 x 4 x 1: 32 boxes on the ground, 128 contacts, none with a body on side 0; period 4, depth 4, two idle
        wavefronts [32 32 32 32 0 0 0 0] -- the smallest pile that takes the form: a phase needs 32 lanes
  g32p  g32 without the fourth contact of its last 12 boxes [32 32 32 20 ..]: the last 12 pairs of wavefront 1 have an
        A and no B
  two   4 x 4 x 4 beside 2 x 2 x 16: two full tiles of depth 16 and 64, ground and box-box contacts
  mixed 8 x 4 x 2 beside g32: a full tile of period 8 and a half-filled one of period 4
Not pairable:
  col2   one column two boxes high: eight phases in one half-wavefront
  uneven the piles of step_steady_cases.py: tiles that mix islands of different depth, 45.5 lanes per phase
  chain  a full 2 x 2 x 16 tile beside a chain: joints, so the step does not even fuse its assembly"""
import numpy as np

PAIRABLE = ("g32", "g32p", "two", "mixed")
NOT_PAIRABLE = ("col2", "uneven", "chain")
# an empty steady window (`two`: depth 64 against 16 steps of sweeps), a short one and a long one
SWEEPS = (1, 2, 9)


def scene(name):
    from eggshell_amd import scenes
    if name in ("g32", "g32p"):
        sc = scenes.box_stack(8, 4, 1, jitter=1e-3, seed=1)
        if name == "g32p":
            keep = np.ones(sc["body0"].shape[0], bool)
            keep[[4 * b + 3 for b in range(20, 32)]] = False   # box b's contacts are 4 b .. 4 b + 3
            sc = dict(sc, **{k: sc[k][keep] for k in ("kind", "body0", "body1", "data")})
        return sc
    if name == "two":
        return scenes.concat([scenes.box_stack(4, 4, 4, jitter=1e-3, seed=1),
                              scenes.box_stack(2, 2, 16, jitter=1e-3, seed=2, origin=(0.0, 100.0))])
    if name == "mixed":
        return scenes.concat([scenes.box_stack(8, 4, 2, jitter=1e-3, seed=1),
                              scenes.box_stack(8, 4, 1, jitter=1e-3, seed=3, origin=(0.0, 200.0))])
    if name == "col2":
        return scenes.box_stack(1, 1, 2, jitter=1e-3, seed=1)
    if name == "uneven":
        import step_steady_cases
        return step_steady_cases.scene("uneven")
    if name == "chain":
        return scenes.concat([scenes.box_stack(2, 2, 16, seed=1), scenes.chain(2)])
    raise ValueError(name)
