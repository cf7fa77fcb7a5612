"""GPU (-m gpu): the device's model layer -- assemble_kernel and the fused assembly prologue (assemble_device.h),
mass_times_force_kernel, velocity_kernel, advance_kernel (kernels.hip), rotate_by_w (rotation_device.h) -- against the
50-digit reference of tests/model_reference.py, on the inputs and within the derived bounds that
test_model_reference_cpu.py applies to the oracle.  Every test prints its measured max error / tolerance (pytest -s).

Measured on MI355X: see DESIGN.md, "Model layer against a 50-digit reference"."""
import numpy as np
import pytest

import model_reference as ref
from eggshell_amd import capi

pytestmark = pytest.mark.gpu


def make_problem(ctx, case, compact_mass=False):
    pr = capi.Problem(ctx, case["p"].shape[0], case["body0"], case["body1"])
    if compact_mass:     # egs_problem_set_mass: 1/m and the 3x3 inverse inertia
        blocks = case["Minv"].reshape(-1, 6, 6)
        pr.set_state(case["p"], case["R"], case["v"], case["w"], None, case["f_ext"])
        pr.set_mass(blocks[:, 0, 0].copy(), blocks[:, 3:, 3:].reshape(-1, 9).copy())
    else:
        pr.set_state(case["p"], case["R"], case["v"], case["w"], case["Minv"], case["f_ext"])
    pr.set_constraints(case["kind"], case["data"])
    return pr


@pytest.mark.parametrize("cid", ref.ASSEMBLY_IDS)
def test_assembly_against_reference(ctx, cid):
    """assemble + blocks at m = 1, 255, 256, 257, 513 (assemble_kernel stages 256 x 18 values through LDS; its tail
    lanes recompute the last constraint): joints and contacts mixed, all three world-side forms, normals of any length,
    on the axes, down to 1e-5 rad from -z and inside the antiparallel branch, positions of order 1 and 100, isotropic,
    rotated-diagonal and fully coupled M^-1, every dt and erp."""
    case, asm = ref.assembly_case(cid)
    pr = make_problem(ctx, case)
    pr.assemble(case["dt"], case["erp"])
    J0, J1, is_eq, lo, hi, rhs, err = pr.blocks()
    pr.close()
    ref.check_assembly(case, asm, J0, J1, is_eq, lo, hi, err, rhs, "device " + cid)


def step_and_check(ctx, case, who, compact_mass=False, fused=None):
    """One egs_problem_step with 10 fixed Gauss-Seidel sweeps (tol 0, cfm 0.01): the blocks it leaves meet the
    assembly bounds, and velocity() equals the reference's v + dt M^-1 (f + J^T lambda) -- the reference's own J, the
    device's lambda -- within the project's bound 1e-12 max(1, |v'|) (test_gpu_step.py)."""
    asm = ref.assemble_reference(case)
    assert not asm["branch"].any()
    pr = make_problem(ctx, case, compact_mass)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=10, tol=0.0, cfm=0.01)
    st = pr.step(case["dt"], case["erp"], prm, want_stats=True)
    lam, v6 = pr.lambda_(), pr.velocity()
    J0, J1, is_eq, lo, hi, rhs, err = pr.blocks()
    pr.close()
    assert st.status == capi.OK and st.iterations == 10
    if fused is not None:
        assert bool(st.schedule & capi.SCHED_FUSED_ASSEMBLY) == fused and bool(st.schedule & capi.SCHED_LINSYM) == fused
    assert np.abs(lam).max() > 0
    ref.check_assembly(case, asm, J0, J1, is_eq, lo, hi, err, rhs, "device " + who)
    m = case["kind"].shape[0]
    vr = ref.velocity_reference(case, asm["J0"].array().reshape(m, 18), asm["J1"].array().reshape(m, 18), lam).array()
    d = np.abs(v6.reshape(-1) - vr).max()
    bound = 1e-12 * max(1.0, np.abs(vr).max())
    print("device %s: velocity max error %.3g, bound %.3g (max |v'| %.3g, max |lambda| %.3g)" % (who, d, bound, np.abs(vr).max(), np.abs(lam).max()))
    assert d <= bound


def test_step_mixed_scene(ctx):
    """Scene (a): 12 bodies, 40 mixed constraints, anisotropic M^-1 through set_state: assemble_kernel and the general
    sweep."""
    step_and_check(ctx, ref.step_scene_a(), "scene a", fused=False)


def test_step_mixed_scene_compact_mass(ctx):
    """Scene (a) with isotropic bodies, M^-1 through set_mass."""
    step_and_check(ctx, ref.step_scene_a("iso"), "scene a, set_mass", compact_mass=True)


def test_step_box_stack_fused(ctx, monkeypatch):
    """Scene (b): the 2 x 2 x 2 box stack through the fused assembly prologue and the isotropic LINSYM form.  The
    schedule policy gives so small a pile to the 4-lane kernel, so the switches that force the 1-lane timetable and its
    isotropic variant are set (EGS_QUAD=0, EGS_STEP=1, EGS_ISO=2, as test_gpu_fuzz.py sets them), and the schedule the
    step reports is asserted.  The fused launch fills every get_blocks output (step_solve.hip), so blocks() after it meets
    the assembly bounds as well."""
    monkeypatch.setenv("EGS_QUAD", "0")
    monkeypatch.setenv("EGS_STEP", "1")
    monkeypatch.setenv("EGS_ISO", "2")
    monkeypatch.delenv("EGS_FUSED_ASSEMBLY", raising=False)
    monkeypatch.delenv("EGS_ISO_LINSYM", raising=False)
    step_and_check(ctx, ref.step_scene_b(), "scene b", fused=True)


@pytest.mark.parametrize("cid", ref.ADVANCE_IDS)
def test_advance_against_reference(ctx, cid):
    """advance at 1, 255 and 257 bodies: mean angular velocities exactly zero, 1e-170 (the squared norm underflows),
    1e-9, 1, 50 and 1400 rad/s at dt = 5e-3 (7 rad, past 2 pi), and a set of R drifted 1e-6 from orthonormal, which the
    update multiplies and must not re-orthonormalise.  p within 4u mag and R within 32u of the reference, taken from
    the velocities the device itself reports; velocity() against the reference too; v, w afterwards are velocity(),
    bit for bit."""
    case = ref.advance_case(cid)
    n = case["p"].shape[0]
    pr = make_problem(ctx, case)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=10, tol=0.0, cfm=0.01)
    pr.step(case["dt"], case["erp"], prm)
    lam, v6 = pr.lambda_(), pr.velocity()
    J0, J1 = pr.blocks()[0:2]
    pr.advance(case["dt"])
    pos, R, v, w = pr.state()
    pr.close()
    assert np.array_equal(v, v6[:, :3]) and np.array_equal(w, v6[:, 3:])
    keeps = np.array([s != "torque" for s in case["spins"]])
    assert np.array_equal(v6[keeps, 3:], case["w"][keeps])          # the spins are the ones the case lists
    assert np.array_equal(v6[1:], case["v6_host"][1:]) or np.abs(v6[1:] - case["v6_host"][1:]).max() < 1e-13
    vr = ref.velocity_reference(case, J0, J1, lam).array()
    assert np.abs(v6.reshape(-1) - vr).max() <= 1e-12 * max(1.0, np.abs(vr).max())
    v6_old = np.concatenate([case["v"], case["w"]], axis=1)
    P, Q = ref.position_reference(case["p"], case["R"], v6_old, v6, case["dt"])
    (rp, wp), (rq, wq) = P.worst(pos), Q.worst(R)
    print("device %s: position max error/tolerance %.3g, rotation %.3g (%.2f u)" % (cid, rp, rq, 32 * rq))
    assert rp <= 1.0 and rq <= 1.0, (wp, wq)
    if "drift" in cid:      # R R^T - I of the inputs is of order 1e-6 and must still be: no re-orthonormalisation
        G = np.einsum("bij,bkj->bik", R.reshape(n, 3, 3), R.reshape(n, 3, 3)) - np.eye(3)
        assert np.abs(G).max() > 1e-7
