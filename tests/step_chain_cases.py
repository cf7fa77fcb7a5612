"""The scenes of test_gpu_step_chain.py and test_plan_chained.py: the pairable piles of step_pair_cases.py, whose plan
is also chained (the two constraints of every thread pair of the lane-pair form are consecutive contacts of the same
two bodies: plan.h), one more of them, and pairable lists whose plan is not chained.

Chained: g32, g32p, two, mixed (step_pair_cases.py) and
  h2     8 x 4 x 2: one full tile of period 8 and depth 8 whose upper contacts have a body on side 0
Pairable, not chained:
  flat64 8 x 8 x 1 with only contact 0 of each box: 64 ground contacts at level 0, period 1 -- the A and the B of a pair
         are different boxes at the same level
  odd3   8 x 4 x 1 with contacts 0 .. 2 of each box: period 3
Not even pairable: col2, uneven, chain (step_pair_cases.py)."""
import numpy as np

import step_pair_cases as spc

CHAINED = spc.PAIRABLE + ("h2",)
PAIRABLE_NOT_CHAINED = ("flat64", "odd3")
NOT_CHAINED = PAIRABLE_NOT_CHAINED + spc.NOT_PAIRABLE
# an empty steady window (`two`: depth 64), a short one, and long ones of 9 and 10 sweeps
SWEEPS = (1, 2, 9, 10)


def keep_contacts(sc, per_box):
    """The box-on-ground pile sc (box b's contacts are 4 b .. 4 b + 3) with only contacts 0 .. per_box - 1 of each box."""
    keep = (np.arange(sc["body0"].shape[0]) % 4) < per_box
    return dict(sc, **{k: sc[k][keep] for k in ("kind", "body0", "body1", "data")})


def scene(name):
    from eggshell_amd import scenes
    if name == "h2":
        return scenes.box_stack(8, 4, 2, jitter=1e-3, seed=1)
    if name == "flat64":
        return keep_contacts(scenes.box_stack(8, 8, 1, jitter=1e-3, seed=1), 1)
    if name == "odd3":
        return keep_contacts(scenes.box_stack(8, 4, 1, jitter=1e-3, seed=1), 3)
    return spc.scene(name)


def steady_window(method, depth, period, sweeps):
    """[t_s, t_e) of a fresh launch's steady window as step_pair.hip sets it before the CHAIN form trims it, and the
    timetable's end; method "gs" or "sor"."""
    if method == "sor":
        t_end = depth + (depth + period * (sweeps - 1) if sweeps >= 1 else 0)
        t_s, t_e = 2 * depth - 1, min(depth + period * sweeps, t_end)
    else:
        t_end = depth + period * sweeps
        t_s, t_e = depth, min(period * (sweeps + 1), t_end)
    return (t_s, t_e, t_end) if t_e > t_s else (0, 0, t_end)
