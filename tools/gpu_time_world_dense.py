#!/usr/bin/env python3
"""The reference's live dense Ensemble::Step (ensembles.cc:498-538) for E ensembles per frame, three ways, wall time
per frame (host included, the device drained at the end of every timed stretch):
  (a) ONE dense world holding the E ensembles (egs_world_step_dense),
  (b) E one-ensemble dense worlds stepped in turn,
  (c) the explicit route per ensemble: contacts from egs_update_contacts (piles), Problem.assemble + dense_condition
      + step_dense + advance, the state read back and re-uploaded every step.
Cases: Chain(8) (joints only, no contact detection) at E = 1, 16, 256; 2x2x2 piles (contacts, re-plans; use_bounds =
1, the true box problem: under the reference's rule, quirk Q3, every pile fails its first step) at E = 16, 256.

  python tools/gpu_time_world_dense.py [--warmup 3] [--steps 10] [--cases chain8 pile222] [--ensembles ...]

Under rocprofv3 --kernel-trace --stats the fused kernel's time per size class shows as dense_world_fused_kernel<32, 64>
(Chain(8): 24 rows) and <112, 256> (2x2x2 piles: 96 rows)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eggshell_amd import capi, scenes  # noqa: E402
from oracle import oracle as orc  # noqa: E402

DT, ERP, CFM = 0.005, 0.2, 0.01


def ensembles(case, E):
    out = []
    for e in range(E):
        if case == "chain8":
            sc = scenes.chain(8, anchor=(2.5 * (e % 16), 2.5 * (e // 16), 2.0))
        else:
            sc = scenes.box_stack(2, 2, 2, jitter=1e-3, seed=e + 1, origin=(2.0 * (e % 16), 2.0 * (e // 16)))
        n = sc["p"].shape[0]
        sc["Minv"] = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"]).reshape(n, 36)
        sc["f_ext"] = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"]).reshape(n, 6)
        out.append(sc)
    return out


def world(ctx, ens, case):
    w, off = capi.World.batch(ctx, [sc["p"].shape[0] for sc in ens])
    cat = lambda k, d: np.concatenate([sc[k].reshape(-1, d) for sc in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6))
    if case == "chain8":
        w.set_joints(np.concatenate([np.where(sc["body0"] >= 0, sc["body0"] + o, -1) for sc, o in zip(ens, off)]),
                     np.concatenate([np.where(sc["body1"] >= 0, sc["body1"] + o, -1) for sc, o in zip(ens, off)]),
                     np.concatenate([sc["data"] for sc in ens]))
    return w


def timed(ctx, frame, warmup, steps):
    for _ in range(warmup):
        frame()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        frame()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


class Explicit:
    """(c): one Problem per ensemble, re-created when its contact topology changes."""

    def __init__(self, ctx, ens, case):
        self.ctx, self.ens, self.case = ctx, ens, case
        self.st = [dict(p=sc["p"].copy(), R=sc["R"].copy(), v=sc["v"].copy(), w=sc["w"].copy()) for sc in ens]
        self.pr = [None] * len(ens)
        self.topo = [None] * len(ens)

    def frame(self):
        for k, sc in enumerate(self.ens):
            s = self.st[k]
            if self.case == "chain8":
                b0, b1, data, kind = sc["body0"], sc["body1"], sc["data"], sc["kind"]
            else:
                b0, b1, data = self.ctx.update_contacts(s["p"], s["R"])
                kind = np.full(b0.shape[0], capi.CONTACT_BOX, np.int32)
            key = (b0.tobytes(), b1.tobytes())
            if self.topo[k] != key:
                if self.pr[k] is not None:
                    self.pr[k].close()
                self.pr[k] = capi.Problem(self.ctx, sc["p"].shape[0], b0, b1)
                self.topo[k] = key
            pr = self.pr[k]
            pr.set_state(s["p"], s["R"], s["v"], s["w"], sc["Minv"], sc["f_ext"])
            pr.set_constraints(kind, data)
            pr.assemble(DT, ERP)
            cfm = 0.0 if pr.dense_condition(0.0) < 1e7 else CFM
            ok, _ = pr.step_dense(DT, ERP, cfm, use_bounds=0 if self.case == "chain8" else 1)
            if not ok:
                raise RuntimeError("explicit route: ensemble %d failed" % k)
            pr.advance(DT)
            s["p"], s["R"], s["v"], s["w"] = pr.state()

    def close(self):
        for p in self.pr:
            if p is not None:
                p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["chain8", "pile222"])
    ap.add_argument("--ensembles", type=int, nargs="+", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    ctx = capi.Context(0)
    for case in a.cases:
        detect = case != "chain8"
        ub = 0 if case == "chain8" else 1
        for E in a.ensembles or ([1, 16, 256] if case == "chain8" else [16, 256]):
            ens = ensembles(case, E)

            def step(w):
                nf = w.step_dense(DT, ERP, CFM, use_bounds=ub, detect_contacts=detect)
                if nf:
                    raise RuntimeError("dense world: %d ensembles failed" % nf)

            bw = world(ctx, ens, case)
            t_a = timed(ctx, lambda: step(bw), a.warmup, a.steps)
            info, rp = bw.dense_info(), bw.info()["replans"]
            bw.close()
            singles = [world(ctx, [sc], case) for sc in ens]
            t_b = timed(ctx, lambda: [step(w) for w in singles], a.warmup, a.steps)
            for w in singles:
                w.close()
            ex = Explicit(ctx, ens, case)
            t_c = timed(ctx, ex.frame, a.warmup, a.steps)
            ex.close()
            print("%-8s E=%4d  (a) batched %8.3f ms/frame  (b) worlds in turn %8.3f  (c) explicit route %8.3f  "
                  "b/a x%.1f  c/a x%.1f  [pivots %d-%d, cfm added in %d, %d re-plans]"
                  % (case, E, t_a, t_b, t_c, t_b / t_a, t_c / t_a, info["pivots"].min(), info["pivots"].max(),
                     int((info["cfm"] > 0).sum()), rp), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
