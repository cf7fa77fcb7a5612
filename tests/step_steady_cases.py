"""The cases of test_gpu_step_steady.py, and the worker that runs them: `python step_steady_cases.py GROUP OUT.npz` runs
every case of GROUP on device 0 under the EGS_* switches of its environment and stores every output array.  The test
starts one such process per environment, so that no switch outlives the launches it is meant for.

A case is (scene, path, method, sweeps):
  path "step":  egs_problem_step, then egs_problem_get_stats (fp64: the fused, store-free LINSYM launch)
  path "solve": egs_problem_assemble + egs_problem_solve (fp64: the plain LINSYM launch, or what EGS_ISO_LINSYM /
                EGS_ISO leave of it)
  path "tol":   a tolerance-terminated step (tol 1e-9, at most 64 sweeps): the snapshot-recording launches."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT, ERP, CFM = 5e-3, 0.2, 0.01

# the window logic by sweeps: 2x2x4 (64 constraints, depth 16, period 8) has no window at 0 and 1 sweeps and a short
# one at 2; 2x2x16 fills a 256-lane tile at depth 64, where a forward window opens at 8 sweeps
SWEEPS = {"s4": (0, 1, 2, 3, 10), "s16": (1, 7, 8, 9, 100), "uneven": (1, 9, 30)}

# every switch that puts these small scenes on the 1-lane isotropic timetable kernel
BASE_ENV = {"EGS_QUAD": "0", "EGS_ISO": "2", "EGS_STEP": "1"}


def scene(name):
    from eggshell_amd import scenes
    if name == "s4":
        return scenes.box_stack(2, 2, 4, jitter=1e-3, seed=1)
    if name == "s16":
        return scenes.box_stack(2, 2, 16, jitter=1e-3, seed=2)
    # islands of depth 12 and 64 share tiles, and the last tile keeps inactive lanes
    return scenes.concat([scenes.box_stack(2, 2, 3, jitter=1e-3, seed=3, origin=(0.0, 0.0)),
                          scenes.box_stack(2, 2, 16, jitter=1e-3, seed=4, origin=(0.0, 100.0)),
                          scenes.box_stack(3, 1, 5, jitter=1e-3, seed=5, origin=(0.0, 200.0))])


def cases(group):
    if group == "main":     # fp64, GS and backward SOR, both paths, and the stopping loop
        out = [(sc, path, m, s) for sc in ("s4", "s16", "uneven") for path in ("step", "solve") for m in ("gs", "sor")
               for s in SWEEPS[sc]]
        return out + [("s4", "tol", "gs", 64)]
    if group == "solve":    # fp64 GS through assemble + solve
        return [(sc, "solve", "gs", s) for sc in ("s4", "s16", "uneven") for s in SWEEPS[sc]]
    if group == "f32":
        return [(sc, "step", "gs", s) for sc in ("s4", "s16") for s in SWEEPS[sc]]
    raise ValueError(group)


def key(case):
    return "%s.%s.%s.%d" % case


def params(method, sweeps, tol=0.0):
    from eggshell_amd import capi
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    return capi.params(method=meth, max_iters=sweeps, tol=tol, cfm=CFM, omega=omega)


def run_case(ctx, case, precision):
    import bench
    sc_name, path, method, sweeps = case
    pr, _ = bench.build_problem(ctx, scene(sc_name), precision)
    try:
        if path == "solve":
            pr.assemble(DT, ERP)
            st = pr.solve(params(method, sweeps))
        else:
            pr.step(DT, ERP, params(method, sweeps, tol=1e-9 if path == "tol" else 0.0))
            st = pr.stats()
        out = dict(lam=pr.lambda_(), acc=pr.accumulators(), wres=pr.wres(),
                   st=np.array([st.status, st.iterations, st.schedule], np.int64), residual=np.array([st.residual]))
        if path != "solve":
            out["v6"] = pr.velocity()
        return out
    finally:
        pr.close()


def main(group, path):
    from eggshell_amd import capi
    ctx = capi.Context(0)
    arrays = {}
    for case in cases(group):
        for name, a in run_case(ctx, case, capi.F32 if group == "f32" else capi.F64).items():
            arrays[key(case) + "." + name] = a
    ctx.close()
    np.savez(path, **arrays)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
