#!/usr/bin/env python3
"""Host in/out time of egs_update_contacts_shapes: 4 096 balls on a plate against 4 096 cubes on the same plate.

  python tools/gpu_time_collide_shapes.py [--side 64] [--samples 9] [--warmup 3]

Both scenes are a --side x --side grid of bodies 1 mm into their neighbours and 2 mm into a big plate (body 0, a box
in both), the plate 1 mm into the ground: balls of radius 0.15 with shape = EGS_SHAPE_SPHERE, or 0.3 cubes with
shape = NULL (today's launches).  Each scene is timed under both broad phases (EGS_BROADPHASE = pairs / grid): wall
time of the whole call -- upload, collide, read-back -- per sample after --warmup calls; the median and the range are
printed as one JSON line per leg.  There is no target: the figure beside the balls is the cubes' of the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(side, balls):
    from eggshell_amd import capi
    n = side * side
    pitch = 0.3 - 1e-3
    ij = np.array([[i, j] for i in range(side) for j in range(side)], np.float64)
    span = pitch * (side - 1)
    p = np.vstack([[[span / 2, span / 2, 0.049]], np.column_stack([ij * pitch, np.full(n, 0.099 + 0.15 - 2e-3)])])
    R = np.tile(np.eye(3).reshape(9), (n + 1, 1))
    sides = np.vstack([[[span + 1.0, span + 1.0, 0.1]], np.full((n, 3), 0.3)])
    shape = np.concatenate([[capi.SHAPE_BOX], np.full(n, capi.SHAPE_SPHERE)]).astype(np.int32) if balls else None
    return p, R, sides, shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from eggshell_amd import capi
    ctx = capi.Context(0)
    for mode in ("pairs", "grid"):
        os.environ["EGS_BROADPHASE"] = mode
        for name, balls in (("cubes", False), ("balls", True)):
            p, R, sides, shape = scene(a.side, balls)
            cap = 32 * p.shape[0]
            times, m = [], 0
            for k in range(a.warmup + a.samples):
                t0 = time.perf_counter()
                b0, b1, data = ctx.update_contacts_shapes(p, R, sides, shape, max_contacts=cap)
                t1 = time.perf_counter()
                m = len(b0)
                if k >= a.warmup:
                    times.append((t1 - t0) * 1e3)
            print(json.dumps(dict(scene=name, broadphase=mode, bodies=int(p.shape[0]), contacts=m,
                                  ms_median=round(float(np.median(times)), 3), ms_min=round(min(times), 3),
                                  ms_max=round(max(times), 3), samples=a.samples)))
    ctx.close()


if __name__ == "__main__":
    main()
