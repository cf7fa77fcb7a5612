"""The cases of test_gpu_step_contact_bounds.py, and the worker that runs them: `python step_contact_bounds_cases.py
GROUP OUT.npz` runs every case of GROUP on device 0 under the EGS_* switches of its environment and stores every output
array.  The test starts one such process per environment, in the manner of step_steady_cases.py.

A case is (scene, path, method, sweeps):
  path "step":  egs_problem_step, then egs_problem_get_stats (contacts only: the fused, store-free LINSYM launch, whose
                sweep projects with a contact's bounds as literals)
  path "solve": egs_problem_assemble + egs_problem_solve (the plain LINSYM launch, which reads its bounds from memory)

Scenes: s4 / s16 are the piles of step_steady_cases.py (64 contacts in one partly filled tile with side-1-only ground
lanes; one full 256-lane tile), at rest and "kicked" (random body velocities, so that friction rows reach both bounds
and normal rows reach 0); j1 / j2 add a chain with a one-body joint, resp. an anchor and a two-body joint, to s4."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT, ERP, CFM = 5e-3, 0.2, 0.01
SWEEPS = (1, 3, 10)
CONTACT_SCENES = ("s4", "s4k", "s16", "s16k")
JOINT_SCENES = ("j1", "j2")

# every switch that puts these small scenes on the 1-lane isotropic timetable kernel
BASE_ENV = {"EGS_QUAD": "0", "EGS_ISO": "2", "EGS_STEP": "1"}


def kick(sc):
    rng = np.random.default_rng(7)
    sc = dict(sc)
    sc["v"] = sc["v"] + rng.uniform(-1.0, 1.0, sc["v"].shape) * np.array([0.5, 0.5, 0.3])
    sc["w"] = sc["w"] + rng.uniform(-1.0, 1.0, sc["w"].shape) * 0.5
    return sc


def scene(name):
    from eggshell_amd import scenes
    if name in ("j1", "j2"):
        return scenes.concat([scenes.box_stack(2, 2, 4, seed=1), scenes.chain(1 if name == "j1" else 2)])
    sc = (scenes.box_stack(2, 2, 4, jitter=1e-3, seed=1) if name.startswith("s4")
          else scenes.box_stack(2, 2, 16, jitter=1e-3, seed=2))
    return kick(sc) if name.endswith("k") else sc


def cases(group):
    if group == "contacts":
        return [(sc, path, m, s) for sc in CONTACT_SCENES for path in ("step", "solve") for m in ("gs", "sor")
                for s in SWEEPS]
    if group == "joints":
        return [(sc, "step", m, s) for sc in JOINT_SCENES for m in ("gs", "sor") for s in SWEEPS]
    raise ValueError(group)


def key(case):
    return "%s.%s.%s.%d" % case


def params(method, sweeps):
    from eggshell_amd import capi
    meth, omega = (capi.GAUSS_SEIDEL, 1.0) if method == "gs" else (capi.SOR, 1.5)
    return capi.params(method=meth, max_iters=sweeps, tol=0.0, cfm=CFM, omega=omega)


def run_case(ctx, case, precision):
    import bench
    sc_name, path, method, sweeps = case
    pr, _ = bench.build_problem(ctx, scene(sc_name), precision)
    try:
        if path == "solve":
            pr.assemble(DT, ERP)
            st = pr.solve(params(method, sweeps))
        else:
            pr.step(DT, ERP, params(method, sweeps))
            st = pr.stats()
        out = dict(lam=pr.lambda_(), acc=pr.accumulators(), wres=pr.wres(),
                   st=np.array([st.status, st.iterations, st.schedule], np.int64))
        if path == "step":
            out["v6"] = pr.velocity()
        return out
    finally:
        pr.close()


def main(group, path):
    from eggshell_amd import capi
    ctx = capi.Context(0)
    arrays = {}
    for case in cases(group):
        for name, a in run_case(ctx, case, capi.F64).items():
            arrays[key(case) + "." + name] = a
    ctx.close()
    np.savez(path, **arrays)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
