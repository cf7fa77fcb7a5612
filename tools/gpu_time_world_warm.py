#!/usr/bin/env python3
"""What warm start (egs_world_set_warm_start) costs and what it buys: one batched world of E box piles (4 x 4 x 4 by
default, spaced apart), SOR, cfm 0.01, a fixed sweep count per step.

  python tools/gpu_time_world_warm.py [--ensembles 1 16 256] [--pile 4 4 4] [--sweeps 100] [--warmup 10]
                                      [--steps 10] [--samples 20] [--radius 0.01] [--out profiles/warm/world_warm.json]

Per E:
  cost     ms per frame (device events, egs_timer_*) with warm start off and on at --sweeps fixed sweeps: the median and
           the range of --samples samples, each --steps frames of a fresh world after --warmup frames.  The difference
           is the match and the snapshot launch.
  reached  the residual (the largest over the ensembles, egs_solve_stats.residual) of the last frame, off and on.
  sweeps   the smallest fixed sweep count at which the warm world's last frame ends at or below the residual the cold
           world reaches at --sweeps, found by stepping the count down (halving, then by ones): every candidate is a
           fresh warm world run over the same frames.

One JSON document with every sample goes to --out; the table is printed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from eggshell_amd import capi, scenes  # noqa: E402

DT, ERP, CFM = 0.005, 0.2, 0.01


def piles(E, pile):
    nx, ny, nz = pile
    pitch = 0.31 * max(nx, ny) + 2.0
    out = []
    for e in range(E):
        sc = scenes.box_stack(nx, ny, nz, jitter=1e-3, seed=e + 1, origin=(pitch * (e % 16), pitch * (e // 16)))
        Minv, f_ext = bench.host_mass_and_force(sc)
        out.append((sc, np.asarray(Minv).reshape(-1, 36), np.asarray(f_ext).reshape(-1, 6)))
    return out


def world(ctx, ens, warm, radius):
    w, _ = capi.World.batch(ctx, [sc["p"].shape[0] for sc, _, _ in ens])
    cat = lambda k: np.concatenate([sc[k] for sc, _, _ in ens])
    w.set_bodies(cat("p"), cat("R"), cat("v"), cat("w"), np.concatenate([m for _, m, _ in ens]),
                 np.concatenate([f for _, _, f in ens]))
    if warm:
        w.set_warm_start(True, radius)
    return w


def run(ctx, ens, warm, sweeps, a):
    """A fresh world: warm-up frames, then the timed frames.  ms per frame and the last frame's residual."""
    prm = capi.params(method=capi.SOR, max_iters=sweeps, tol=0.0, cfm=CFM)
    w = world(ctx, ens, warm, a.radius)
    for _ in range(a.warmup):
        w.step(DT, ERP, prm)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.steps - 1):
        w.step(DT, ERP, prm)
    st = w.step(DT, ERP, prm, want_stats=True)
    ms = ctx.timer_stop() / a.steps
    w.close()
    return ms, st.residual


def sweeps_needed(ctx, ens, target, a):
    """The smallest fixed sweep count whose warm last-frame residual is <= target: down by halves, then by ones."""
    good, tried = a.sweeps, {}
    def reaches(k):
        if k not in tried:
            tried[k] = run(ctx, ens, True, k, a)[1]
        return tried[k] <= target
    if not reaches(good):
        return None, tried
    k = good // 2
    while k >= 1 and reaches(k):
        good, k = k, k // 2
    lo = max(k, 0)          # lo fails (or is 0), good reaches
    while good - lo > 1:
        mid = (lo + good) // 2
        if reaches(mid):
            good = mid
        else:
            lo = mid
    return good, tried


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensembles", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--pile", type=int, nargs=3, default=[4, 4, 4], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm", "world_warm.json"))
    a = ap.parse_args()
    ctx = capi.Context(0)
    doc = dict(pile=a.pile, sweeps=a.sweeps, warmup=a.warmup, steps=a.steps, samples=a.samples, radius=a.radius, dt=DT, erp=ERP,
               cfm=CFM, method="sor", results=[])
    for E in a.ensembles:
        ens = piles(E, a.pile)
        ms = {False: [], True: []}
        res = {}
        for _ in range(a.samples):
            for warm in (False, True):      # in turn: a drift of the clocks hits both alike
                t, r = run(ctx, ens, warm, a.sweeps, a)
                ms[warm].append(t)
                res[warm] = r               # the same trajectory every sample: the same residual
        need, tried = sweeps_needed(ctx, ens, res[False], a)
        off, on = np.array(ms[False]), np.array(ms[True])
        print("%dx%dx%d E=%4d  %d sweeps: off %8.3f ms/frame (%.3f..%.3f)  on %8.3f (%.3f..%.3f)  +%.3f ms   residual off %.3g on %.3g   "
              "warm sweeps to reach the cold residual: %s" %
              (*a.pile, E, a.sweeps, np.median(off), off.min(), off.max(), np.median(on), on.min(), on.max(),
               np.median(on) - np.median(off), res[False], res[True], need if need is not None else "more than %d" % a.sweeps),
              flush=True)
        doc["results"].append(dict(ensembles=E, ms_off=ms[False], ms_on=ms[True], median_off=float(np.median(off)),
                                   median_on=float(np.median(on)), residual_off=res[False], residual_on=res[True],
                                   warm_sweeps_for_cold_residual=need, residual_by_warm_sweeps={str(k): v for k, v in sorted(tried.items())}))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
