#!/usr/bin/env python3
"""E separate worlds stepped in turn (SimulationStep() calling Step() on every Ensemble, model.cc:37-70) against
ONE batched world holding the same E ensembles (egs_world_create_batch): box piles (4 x 4 x 4 by default), spaced apart or all
at one origin, SOR tol 1e-9 / cap 500 / cfm 0.01.  Per frame (all E ensembles one step) the device-event time
(egs_timer_*), after warm-up steps; then one traced pass of the batched world (EGS_WORLD_TRACE=1: host time per
phase, re-plan included, printed by egs_world_destroy).

  python tools/gpu_time_world_batch.py [--ensembles 16 256] [--pile 4 4 4] [--warmup 10] [--steps 30]

--pile 16 16 4 --ensembles 4 is the other shape: a few large ensembles, where every (ensemble, recorded sweep) of the
segmented residual is one workgroup walking the ensemble's whole row set.  Under rocprofv3 --kernel-trace --stats it
compares seg_residual_kernel with the separate worlds' hist_residual_kernel.

  python tools/gpu_time_world_batch.py --each [--repeats 7] [--lib PATH/libeggshell_amd.so]

times the batched world alone, co-located and spaced: egs_world_step against egs_world_step_each with equal rates (the
same dt and erp for every ensemble: the same trajectory, bit for bit), each sample on a fresh world over the same
steps, the two entries in turn; the median and the range of the samples.  --lib loads another build of the library
(one without egs_world_step_each is timed on egs_world_step alone): the yardstick of a comparison across commits."""
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


def timed_entry(ctx, w, prm, warmup, steps, each):
    E = w.n_ensembles
    dt, erp = np.full(E, DT), np.full(E, ERP)
    step = (lambda: w.step_each(dt, erp, prm)) if each else (lambda: w.step(DT, ERP, prm))
    for _ in range(warmup):
        step()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(steps):
        step()
    return ctx.timer_stop() / steps


def each_mode(ctx, a, prm):
    have_each = hasattr(capi.load(), "egs_world_step_each")
    for E in a.ensembles:
        for spaced in (True, False):
            ens = piles(E, spaced, a.pile)
            samples = {False: [], True: []}
            for _ in range(a.repeats):
                for each in ((False, True) if have_each else (False,)):
                    w = batched(ctx, ens)
                    samples[each].append(timed_entry(ctx, w, prm, a.warmup, a.steps, each))
                    w.close()
            for each, name in ((False, "egs_world_step"), (True, "egs_world_step_each")):
                t = np.array(samples[each])
                if t.size:
                    print("%dx%dx%d E=%4d %-10s %-20s median %8.3f ms/frame  min %8.3f  max %8.3f  (%d samples: %s)" %
                          (*a.pile, E, "spaced" if spaced else "co-located", name, np.median(t), t.min(), t.max(), t.size,
                           " ".join("%.3f" % x for x in t)), flush=True)


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
    ap.add_argument("--each", action="store_true", help="egs_world_step against egs_world_step_each with equal rates")
    ap.add_argument("--repeats", type=int, default=7, help="--each: samples per entry, each on a fresh world")
    ap.add_argument("--lib", help="--each: another build of libeggshell_amd.so")
    a = ap.parse_args()
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=0.01)
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    if a.each:
        each_mode(ctx, a, prm)
        ctx.close()
        return
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
