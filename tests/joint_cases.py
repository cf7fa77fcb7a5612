"""Small scenes with welds and hinges, shared by the GPU tests of the angular joint blocks.  A scene is a dict in the
layout of model_reference's cases (p, R, v, w, Minv, f_ext, kind, body0, body1, data, dt, erp) plus motor [m][2] or
None.  Every number in them is exactly representable where a closed form is compared with the device."""
import math

import numpy as np

import joint_reference as jr
import model_reference as mr
from eggshell_amd import scenes

G = 9.8
EYE = np.eye(3).reshape(9)


def _bodies(p, mass, inertia, w=None):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n = p.shape[0]
    Minv = np.zeros((n, 6, 6))
    f = np.zeros((n, 6))
    for b in range(n):
        Minv[b, :3, :3] = np.eye(3) / mass
        Minv[b, 3:, 3:] = np.eye(3) / inertia
        f[b, 2] = -mass * G
    return dict(p=p, R=np.tile(EYE, (n, 1)), v=np.zeros((n, 3)), w=np.zeros((n, 3)) if w is None else np.asarray(w, np.float64),
                Minv=Minv.reshape(n, 36), f_ext=f, mass=np.full(n, float(mass)), inertia=float(inertia))


def welded_pair(spin=0.5):
    """Two unit cubes side by side, welded (ball at the midpoint + lock); body 0 spins about z, body 1 is at rest.
    Isotropic inertia, so the gyroscopic torque vanishes."""
    sc = _bodies([[0.0, 0.0, 1.0], [0.5, 0.0, 1.0]], 2.0, 0.125, w=[[0.0, 0.0, spin], [0.0, 0.0, 0.0]])
    data = np.zeros((2, 7))
    data[0, 0:6] = [0.25, 0.0, 0.0, -0.25, 0.0, 0.0]
    data[1] = jr.lock_data(sc["R"][0], sc["R"][1])
    sc.update(kind=np.array([jr.BALL, jr.LOCK], np.int32), body0=np.zeros(2, np.int32), body1=np.ones(2, np.int32), data=data,
              dt=1.0 / 128, erp=0.25, motor=None)
    return sc


PENDULUM_R, PENDULUM_M, PENDULUM_I = 0.5, 2.0, 0.125


def pendulum(motor=None):
    """A box hinged to the world about the horizontal y axis through the origin, its centre at (r, 0, 0), from rest
    under gravity.  motor = (speed, tau) on the hinge or None.  err is exactly 0, so with cfm = 0 the step gives
    w' = dt m g r / (I + m r^2) about +y when the hinge is free."""
    sc = _bodies([[PENDULUM_R, 0.0, 0.0]], PENDULUM_M, PENDULUM_I)
    data = np.zeros((2, 7))
    data[0, 0:3] = [-PENDULUM_R, 0.0, 0.0]
    data[1, 0:6] = [0.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    sc.update(kind=np.array([jr.BALL, jr.HINGE], np.int32), body0=np.zeros(2, np.int32), body1=np.full(2, -1, np.int32),
              data=data, dt=1.0 / 128, erp=0.25, motor=None if motor is None else np.array([[0.0, -1.0], list(motor)]))
    return sc


def chain_with_weld(n=4):
    """scenes.chain(n) with its first two links welded: the chain's ball joints plus one lock."""
    from oracle import oracle as orc
    ch = scenes.chain(n)
    kind = np.append(ch["kind"], jr.LOCK).astype(np.int32)
    body0 = np.append(ch["body0"], 0).astype(np.int32)
    body1 = np.append(ch["body1"], 1).astype(np.int32)
    data = np.vstack([ch["data"], jr.lock_data(ch["R"][0], ch["R"][1])])
    # joints of a world come first; a problem takes any order
    return dict(p=ch["p"], R=ch["R"], v=ch["v"], w=ch["w"], Minv=orc.minv_blocks(ch["R"], ch["mass"], ch["I_body"]).reshape(n, 36),
                f_ext=orc.external_force(ch["R"], ch["w"], ch["mass"], ch["I_body"]).reshape(n, 6), kind=kind, body0=body0,
                body1=body1, data=data, dt=1e-3, erp=0.2, motor=None)


def motored_pair():
    """Two boxes, the first hinged to the world about z with a motor, the second hinged to the first about x with a
    motor: every axis row is a box row with 0 < tau."""
    sc = _bodies([[0.5, 0.0, 1.0], [1.0, 0.0, 1.0]], 2.0, 0.125)
    data = np.zeros((4, 7))
    data[0, 0:6] = [-0.5, 0.0, 0.0, 0.0, 0.0, 1.0]
    data[1, 0:6] = [0.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    data[2, 0:6] = [0.25, 0.0, 0.0, -0.25, 0.0, 0.0]
    data[3, 0:6] = [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    sc.update(kind=np.array([jr.BALL, jr.HINGE, jr.BALL, jr.HINGE], np.int32), body0=np.array([0, 0, 0, 0], np.int32),
              body1=np.array([-1, -1, 1, 1], np.int32), data=data, dt=1.0 / 128, erp=0.25,
              motor=np.array([[0.0, -1.0], [1.0, 0.5], [0.0, -1.0], [-2.0, math.inf]]))
    return sc


def make_problem(ctx, sc, precision=None):
    from eggshell_amd import capi
    pr = capi.Problem(ctx, sc["p"].shape[0], sc["body0"], sc["body1"], capi.F64 if precision is None else precision)
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], sc["Minv"], sc["f_ext"])
    pr.set_constraints(sc["kind"], sc["data"])
    if sc.get("motor") is not None:
        pr.set_motors(sc["motor"])
    return pr


# ---- ensembles of a world: dicts as tests/test_gpu_world_step_each.py's, with kinds and motors --------------------------------
def ens_chain_with_weld():
    """Four spaced links (no contacts between them), ball joints link to link and link 0 to the world; links 1 and 2
    welded.  The weld's ball joint is the chain's own."""
    from test_gpu_world_step_each import ensemble, spaced_chain
    sc = spaced_chain(4)
    e = ensemble(sc, joints=True)
    b0, b1, data = e["joints"]
    e["joints"] = (np.append(b0, 1).astype(np.int32), np.append(b1, 2).astype(np.int32), np.vstack([data, jr.lock_data(EYE, EYE)]))
    e["kinds"] = np.array([jr.BALL] * 4 + [jr.LOCK], np.int32)
    e["motors"] = None
    return e


def ens_motored_hinge(z=2.0, y=3.0):
    """One box hinged to the world about y at (0, y, z), its centre 0.5 along x, with a motor that clamps."""
    from test_gpu_world_step_each import bodies, ensemble
    e = ensemble(bodies([[0.5, y, z]]))
    data = np.zeros((2, 7))
    data[0, 0:6] = [-0.5, 0.0, 0.0, 0.0, y, z]
    data[1, 0:6] = [0.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    e["joints"] = (np.zeros(2, np.int32), np.full(2, -1, np.int32), data)
    e["kinds"] = np.array([jr.BALL, jr.HINGE], np.int32)
    e["motors"] = np.array([[0.0, -1.0], [1.0, 2.0]])
    return e


def ens_cairn():
    from test_gpu_world_step_each import ensemble
    e = ensemble(scenes.cairn(3, seed=2, origin=(6.0, 0.0)))
    e["kinds"], e["motors"] = None, None
    return e
