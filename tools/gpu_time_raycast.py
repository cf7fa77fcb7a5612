#!/usr/bin/env python3
"""Host in/out time of egs_world_cast_rays, beside the same world's egs_world_step frame time and the host route
(egs_world_get_bodies, then egs_cast_rays per ensemble).

  python tools/gpu_time_raycast.py [--samples 9] [--warmup 3] [--cases heaps1,heaps16,heaps256,plate]

  heapsE   E ensembles in one batched world, each 64 mixed bodies (boxes, balls, logs in turn on an 8 x 8 grid, 0.7
           apart, 1 mm in the ground) with 64 rays attached to its body 0: a fan from that body's centre down over its
           own ensemble
  plate    one world of 4 096 such bodies (64 x 64) under 65 536 world-frame rays from z = 2, each down towards a random
           point of the grid

Each case is timed with the bounding-sphere cull on and off (EGS_RAY_CULL=0): wall time of the whole call per sample after
--warmup calls, the median and the range, one JSON line per leg.  `cast` is egs_world_cast_rays (one launch, one
read-back), `step` one egs_world_step of the same world followed by a synchronise, `host_route` egs_world_get_bodies and
one egs_cast_rays per ensemble with that ensemble's bodies and rays.  No figure has a target."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, ERP = 5e-3, 0.2


def grid_bodies(nx, ny, origin=(0.0, 0.0)):
    """nx x ny bodies 0.7 apart, a box, a ball, a log in turn, each 1 mm in the ground; mass 1, I = 0.1."""
    from eggshell_amd import capi
    n = nx * ny
    shape = (np.arange(n) % 3).astype(np.int32)
    side = np.where((shape == capi.SHAPE_BOX)[:, None], [0.3, 0.3, 0.3],
                    np.where((shape == capi.SHAPE_SPHERE)[:, None], [0.3, 0.3, 0.3], [0.2, 0.2, 0.6]))
    p = np.array([[origin[0] + 0.7 * (k % nx), origin[1] + 0.7 * (k // nx), 0.0] for k in range(n)])
    p[:, 2] = np.where(shape == capi.SHAPE_CAPSULE, 0.099, 0.149)
    R = np.tile(np.eye(3).reshape(9), (n, 1))
    R[shape == capi.SHAPE_CAPSULE] = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64).reshape(9)   # the logs lie along x
    Minv = np.tile(np.diag([1.0] * 3 + [10.0] * 3).reshape(36), (n, 1))
    f_ext = np.tile([0.0, 0.0, -9.8, 0.0, 0.0, 0.0], (n, 1))
    return dict(p=p, R=R, side=side.astype(np.float64), shape=shape, Minv=Minv, f_ext=f_ext)


def timed(fn, warmup, samples):
    t = []
    for k in range(warmup + samples):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= warmup:
            t.append((t1 - t0) * 1e3)
    return dict(ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4), samples=samples)


def run_case(ctx, name, a):
    from eggshell_amd import capi
    rng = np.random.default_rng(1)
    if name == "plate":
        E, ens = 1, [grid_bodies(64, 64)]
        nr = 65536
        eye = np.stack([rng.uniform(0, 44.1, nr), rng.uniform(0, 44.1, nr), np.full(nr, 2.0)], axis=1)
        target = np.stack([rng.uniform(0, 44.1, nr), rng.uniform(0, 44.1, nr), np.zeros(nr)], axis=1)
        o, d, body, rens = eye, target - eye, None, None
    else:
        E = int(name[len("heaps"):])
        ens = [grid_bodies(8, 8) for _ in range(E)]
        gx, gy = np.meshgrid(np.linspace(0, 4.9, 8), np.linspace(0, 4.9, 8))
        fan = np.stack([gx.ravel(), gy.ravel(), np.full(64, -0.149)], axis=1)     # from body 0's centre onto the grid
        o, d = np.zeros((64 * E, 3)), np.tile(fan, (E, 1))
        body = np.repeat(np.arange(E, dtype=np.int32) * 64, 64)
        rens = np.repeat(np.arange(E, dtype=np.int32), 64) if E > 1 else None
    cat = lambda k: np.concatenate([e[k] for e in ens])
    w = capi.World.batch(ctx, [e["p"].shape[0] for e in ens])[0]
    n = w.n
    w.set_bodies(cat("p"), cat("R"), np.zeros((n, 3)), np.zeros((n, 3)), cat("Minv"), cat("f_ext"), side=cat("side"))
    w.set_shapes(cat("shape"))
    w.set_rays(o, d, ray_body=body, ray_ens=rens)
    prm = capi.params(method=capi.SOR, max_iters=20, tol=0.0, cfm=0.01)
    out = (np.zeros(len(o), np.int32), np.zeros(len(o)), np.zeros((len(o), 3)))
    side, shape = cat("side"), cat("shape")
    nb = ens[0]["p"].shape[0]

    def step():
        w.step(DT, ERP, prm)
        ctx.synchronize()

    def host_route():
        p, R, _, _ = w.bodies()
        for e in range(E):
            b, r = slice(e * nb, (e + 1) * nb), slice(e * (len(o) // E), (e + 1) * (len(o) // E))
            ctx.cast_rays(p[b], R[b], side[b], shape[b], o[r], d[r], ray_body=None if body is None else body[r] - e * nb)

    base = dict(case=name, ensembles=E, bodies=n, rays=len(o))
    print(json.dumps(dict(base, leg="step", **timed(step, a.warmup, a.samples))), flush=True)
    for cull in ("1", "0"):
        os.environ["EGS_RAY_CULL"] = cull
        legs = dict(cast=lambda: w.cast_rays(out=out), host_route=host_route)
        for leg, fn in legs.items():
            print(json.dumps(dict(base, leg=leg, cull=cull == "1", **timed(fn, a.warmup, a.samples))), flush=True)
        print(json.dumps(dict(base, leg="hits", cull=cull == "1", bodies_hit=int((out[0] >= 0).sum()), ground=int((out[0] == -1).sum()),
                              none=int((out[0] == -2).sum()))), flush=True)
    os.environ.pop("EGS_RAY_CULL", None)
    w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="heaps1,heaps16,heaps256,plate")
    a = ap.parse_args()
    from eggshell_amd import capi
    ctx = capi.Context(0)
    for name in a.cases.split(","):
        run_case(ctx, name, a)
    ctx.close()


if __name__ == "__main__":
    main()
