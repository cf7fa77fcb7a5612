#!/usr/bin/env python3
"""E separate worlds stepped in turn (SimulationStep() calling Step() on every Ensemble, model.cc:37-70) against
ONE batched world holding the same E ensembles (egs_world_create_batch): box piles (4 x 4 x 4 by default), spaced apart or all
at one origin, SOR tol 1e-9 / cap 500 / cfm 0.01.  Per frame (all E ensembles one step) the device-event time
(egs_timer_*), after warm-up steps; then one traced pass of the batched world (EGS_WORLD_TRACE=1: host time per
phase, re-plan included, printed by egs_world_destroy).

  python tools/gpu_time_world_batch.py [--ensembles 16 256] [--pile 4 4 4] [--warmup 10] [--steps 30]

--pile 16 16 4 --ensembles 4 is the other shape: a few large ensembles, where every (ensemble, recorded sweep) of the
segmented residual is one workgroup walking the ensemble's whole row set.  Under rocprofv3 --kernel-trace --stats it
compares seg_residual_kernel with the separate worlds' hist_residual_kernel."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from eggshell_amd import capi, scenes  # noqa: E402

DT, ERP = 0.005, 0.2


def piles(E, spaced, pile):
    nx, ny, nz = pile
    pitch = 0.31 * max(nx, ny) + 2.0
    out = []
    for e in range(E):
        origin = (pitch * (e % 16), pitch * (e // 16)) if spaced else (0.0, 0.0)
        sc = scenes.box_stack(nx, ny, nz, jitter=1e-3, seed=e + 1, origin=origin)
        Minv, f_ext = bench.host_mass_and_force(sc)
        out.append((sc, np.asarray(Minv).reshape(-1, 36), np.asarray(f_ext).reshape(-1, 6)))
    return out


def timed(ctx, worlds, prm, warmup, steps):
    for _ in range(warmup):
        for w in worlds:
            w.step(DT, ERP, prm)
    r0 = sum(w.info()["replans"] for w in worlds)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(steps):
        for w in worlds:
            w.step(DT, ERP, prm)
    ms = ctx.timer_stop()
    return ms / steps, sum(w.info()["replans"] for w in worlds) - r0


def batched(ctx, ens):
    w, _ = capi.World.batch(ctx, [sc["p"].shape[0] for sc, _, _ in ens])
    cat = lambda k: np.concatenate([sc[k] for sc, _, _ in ens])
    w.set_bodies(cat("p"), cat("R"), cat("v"), cat("w"), np.concatenate([m for _, m, _ in ens]),
                 np.concatenate([f for _, _, f in ens]))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensembles", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--pile", type=int, nargs=3, default=[4, 4, 4], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    ctx = capi.Context(0)
    for E in a.ensembles:
        for spaced in (True, False):
            ens = piles(E, spaced, a.pile)
            singles = []
            for sc, Minv, f_ext in ens:
                w = capi.World(ctx, sc["p"].shape[0])
                w.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
                singles.append(w)
            t_sep, rp_sep = timed(ctx, singles, prm, a.warmup, a.steps)
            for w in singles:
                w.close()
            bw = batched(ctx, ens)
            t_bat, rp_bat = timed(ctx, [bw], prm, a.warmup, a.steps)
            info = bw.batch_info()
            bw.close()
            print("%dx%dx%d E=%4d %-10s separate %8.3f ms/frame (%d re-plans)  batched %8.3f ms/frame (%d re-plans)  x%.2f  "
                  "sweeps per ensemble: min %d max %d" % (*a.pile, E, "spaced" if spaced else "co-located", t_sep, rp_sep, t_bat,
                                                        rp_bat, t_sep / t_bat, info["iterations"].min(),
                                                        info["iterations"].max()), flush=True)
            os.environ["EGS_WORLD_TRACE"] = "1"   # read when a world is created
            tw = batched(ctx, ens)
            del os.environ["EGS_WORLD_TRACE"]
            for _ in range(a.warmup + a.steps):
                tw.step(DT, ERP, prm)
            ctx.synchronize()
            sys.stdout.flush()
            tw.close()   # prints the per-phase host times to stderr
            sys.stderr.flush()
    ctx.close()


if __name__ == "__main__":
    main()
