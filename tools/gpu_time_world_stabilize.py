#!/usr/bin/env python3
"""Ensemble::PostStabilize / InitStabilize (ensembles.cc:602-646) for E ensembles, two ways, wall time per call (host
included, the device drained at the end):
  (a) ONE world holding the E ensembles, one egs_world_stabilize call,
  (b) E one-ensemble worlds stabilised in turn.
Every repetition starts from the same state (egs_world_set_bodies before the timed call, not timed).
Cases: bent Chain(4) (POST, joints only) and overlapping 5-box cairns (INIT with contact detection) at E = 1, 16, 256.

  python tools/gpu_time_world_stabilize.py [--warmup 1] [--reps 3] [--cases chain4 cairn5] [--ensembles 1 16 256]
                                           [--direct] [--no-singles]

Prints one JSON line per (case, E): ms per call both ways, the speed-up, and the relaxation steps (max over ensembles).
A cairn takes about 8.5 s alone (its relaxation solve runs to the 20000-sweep cap), so E = 256 cairn worlds in turn
take over half an hour: time that case with --no-singles.  EGS_WORLD_TRACE=1 prints the host phases of the passes.
--direct times the direct route (egs_world_stabilize_direct) on the same cases in the same run, next to the sweep
route: direct_ms (median of the reps; batch_med_ms is the sweep route's median), the ratio, its steps and the largest
rank; --direct-only skips the sweep route (a cairn's sweep call takes seconds).  Its passes show as stab_direct_kernel.
Under rocprofv3 --kernel-trace --stats the passes show as stab_err_kernel / stab_relax_kernel next to the solve
kernels and assemble_kernel."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eggshell_amd import capi, scenes  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def ensembles(case, E):
    out = []
    for e in range(E):
        origin = (2.5 * (e % 16), 2.5 * (e // 16))
        if case == "chain4":
            sc = scenes.chain(4, anchor=(origin[0], origin[1], 2.0))
            s = 0.5 + (e % 7) / 6.0
            for i in range(1, 4):
                sc["p"][i] += s * np.array([0.01 * i, -0.02 * i, 0.015 * i])
        else:
            sc = scenes.cairn(5, seed=e + 1, origin=origin)
        n = sc["p"].shape[0]
        sc["Minv"] = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36)
        sc["f_ext"] = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6)
        out.append(sc)
    return out


class World:
    def __init__(self, ctx, ens, case):
        self.w, off = capi.World.batch(ctx, [sc["p"].shape[0] for sc in ens])
        cat = lambda k, d: np.concatenate([sc[k].reshape(-1, d) for sc in ens])
        self.state = [cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3)]
        self.w.set_bodies(*self.state, cat("Minv", 36), cat("f_ext", 6))
        if case == "chain4":
            self.w.set_joints(np.concatenate([np.where(sc["body0"] >= 0, sc["body0"] + o, -1) for sc, o in zip(ens, off)]),
                              np.concatenate([np.where(sc["body1"] >= 0, sc["body1"] + o, -1) for sc, o in zip(ens, off)]),
                              np.concatenate([sc["data"] for sc in ens]))
        self.mode = capi.STABILIZE_POST if case == "chain4" else capi.STABILIZE_INIT
        self.direct = False

    def reset(self):
        self.w.set_bodies(*self.state, None, None)

    def run(self):
        if self.direct:
            self.w.stabilize_direct(self.mode)
        else:
            self.w.stabilize(self.mode)


def timed(ctx, worlds, warmup, reps, median=False):
    best, all_ms = float("inf"), []
    for r in range(warmup + reps):
        for w in worlds:
            w.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        for w in worlds:
            w.run()
        ctx.synchronize()
        if r >= warmup:
            all_ms.append((time.perf_counter() - t0) * 1e3)
            best = min(best, all_ms[-1])
    return float(np.median(all_ms)) if median else best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=["chain4", "cairn5"])
    ap.add_argument("--ensembles", nargs="+", type=int, default=[1, 16, 256])
    ap.add_argument("--no-singles", action="store_true", help="time the batched call only")
    ap.add_argument("--direct", action="store_true", help="also time egs_world_stabilize_direct on the same world")
    ap.add_argument("--direct-only", action="store_true", help="time the direct route alone (implies --direct)")
    a = ap.parse_args()
    ctx = capi.Context(0)
    for case in a.cases:
        for E in a.ensembles:
            ens = ensembles(case, E)
            bw = World(ctx, ens, case)
            out = dict(case=case, E=E)
            if not a.direct_only:
                t_batch = timed(ctx, [bw], a.warmup, a.reps)
                steps = bw.w.stabilize_info()["steps"]
                out.update(batch_ms=round(t_batch, 3), max_steps=int(steps.max()), mean_steps=float(steps.mean()))
            if a.direct or a.direct_only:
                if not a.direct_only:
                    out["batch_med_ms"] = round(timed(ctx, [bw], 0, a.reps, median=True), 3)
                bw.direct = True
                t_direct = timed(ctx, [bw], a.warmup, a.reps, median=True)
                steps, rk = bw.w.stabilize_info()["steps"], bw.w.stabilize_rank()
                out.update(direct_ms=round(t_direct, 3), direct_max_steps=int(steps.max()), direct_mean_steps=float(steps.mean()),
                           max_rows=int(rk["rows"].max()), max_rank=int(rk["rank"].max()))
                if not a.direct_only:
                    out["direct_speedup"] = round(out["batch_med_ms"] / t_direct, 2)
                bw.direct = False
            bw.w.close()
            if not a.no_singles and not a.direct_only:
                singles = [World(ctx, [sc], case) for sc in ens]
                t_single = timed(ctx, singles, a.warmup, a.reps)
                out.update(singles_ms=round(t_single, 3), speedup=round(t_single / t_batch, 2))
                for w in singles:
                    w.w.close()
            print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
