#!/usr/bin/env python3
"""Host in/out time of egs_update_contacts_shapes: 4 096 logs on a plate, beside the balls and the cubes of
tools/gpu_time_collide_shapes.py on the same plate in the same session.

  python tools/gpu_time_collide_capsules.py [--side 64] [--samples 9] [--warmup 3] [--lib PATH]

The logs are a --side x --side grid of capsules (radius 0.1, length 0.6, shape = EGS_SHAPE_CAPSULE) lying along x, 1 mm
into their neighbours -- end to end and side by side -- and 2 mm into a big plate (body 0, a box), the plate 1 mm into
the ground.  The balls and the cubes are the other tool's scenes, unchanged.  Each scene is timed under both broad
phases (EGS_BROADPHASE = pairs / grid): wall time of the whole call -- upload, collide, read-back -- per sample after
--warmup calls; the median and the range are printed as one JSON line per leg.  --lib times another build of the
library (the parent's, for the balls and the cubes; a build that refuses EGS_SHAPE_CAPSULE skips the logs).  The
capsule figure has no target: it is reported beside the other two."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def logs(side, radius=0.1, length=0.6):
    from eggshell_amd import capi, scenes
    sc = scenes.log_pile(side, side, 1, radius=radius, length=length, sink=0.0, gap=-1e-3)
    n = sc["p"].shape[0]
    span_x, span_y = (length - 1e-3) * (side - 1), (2 * radius - 1e-3) * (side - 1)
    p = np.vstack([[[0.0, 0.0, 0.049]], sc["p"] + [0.0, 0.0, 0.099 - 2e-3]])
    R = np.vstack([[np.eye(3).reshape(9)], sc["R"]])
    sides = np.vstack([[[span_x + length + 1.0, span_y + 1.0, 0.1]], sc["side"]])
    shape = np.concatenate([[capi.SHAPE_BOX], np.full(n, capi.SHAPE_CAPSULE)]).astype(np.int32)
    return p, R, sides, shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libeggshell_amd.so to time")
    a = ap.parse_args()
    from eggshell_amd import capi
    import gpu_time_collide_shapes as other
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    for mode in ("pairs", "grid"):
        os.environ["EGS_BROADPHASE"] = mode
        for name in ("cubes", "balls", "logs"):
            p, R, sides, shape = logs(a.side) if name == "logs" else other.scene(a.side, name == "balls")
            cap = 32 * p.shape[0]
            times, m = [], 0
            try:
                for k in range(a.warmup + a.samples):
                    t0 = time.perf_counter()
                    b0, b1, data = ctx.update_contacts_shapes(p, R, sides, shape, max_contacts=cap)
                    t1 = time.perf_counter()
                    m = len(b0)
                    if k >= a.warmup:
                        times.append((t1 - t0) * 1e3)
            except capi.EgsError as e:
                if name != "logs" or e.status != capi.ERR_INVALID:
                    raise
                print(json.dumps(dict(scene=name, broadphase=mode, skipped="this build has no capsules")))
                continue
            print(json.dumps(dict(scene=name, broadphase=mode, bodies=int(p.shape[0]), contacts=m,
                                  ms_median=round(float(np.median(times)), 3), ms_min=round(min(times), 3),
                                  ms_max=round(max(times), 3), samples=a.samples, lib=a.lib or "this build")))
    ctx.close()


if __name__ == "__main__":
    main()
