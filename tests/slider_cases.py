"""Small scenes with sliders, shared by the GPU tests of the slider block.  A scene is a dict in the layout of
joint_cases' (p, R, v, w, Minv, f_ext, kind, body0, body1, data, dt, erp, motor) plus travel [m][2] or None.  A slider
is LOCK + SLIDER_AXIS on the same two bodies."""
import math

import numpy as np

import joint_cases as jc
import joint_reference as jr
import slider_reference as sr

G = jc.G
PISTON_M, PISTON_I = 2.0, 0.125
RAIL = np.array([0.6, 0.0, -0.8])      # the tilted rail, pointing down: gravity has g cos(theta) = 0.8 g along it
COS_THETA = 0.8
INF = math.inf


def piston(motor=None, travel=None, x=0.0, across=0.0):
    """A box on a rail to the world (lock + world-side slider) from rest under gravity, its centre at travel x along
    RAIL from the rail's point and `across` off the rail along y.  motor = (speed, f) on the rail row, travel = (xlo, xhi)
    or None.  Row 5 is the rail row."""
    c = np.array([0.25, -0.5, 2.0])
    p0 = c + x * RAIL + across * np.array([0.0, 1.0, 0.0])
    sc = jc._bodies([p0], PISTON_M, PISTON_I)
    data = np.zeros((2, 7))
    data[0] = jr.lock_data(jc.EYE)
    data[1, 0:3], data[1, 3:6] = RAIL, c
    sc.update(kind=np.array([jr.LOCK, sr.SLIDER], np.int32), body0=np.zeros(2, np.int32), body1=np.full(2, -1, np.int32),
              data=data, dt=1.0 / 128, erp=0.25, motor=None if motor is None else np.array([[0.0, -1.0], list(motor)]),
              travel=None if travel is None else np.array([[-INF, INF], list(travel)]))
    return sc


def vertical_piston(travel=None, x=0.0):
    """A unit-mass box on a vertical rail (+z) to the world from rest under gravity, exactly on its rail: the lock's and
    the two equality rows' right-hand sides are 0 and A is diagonal, so the start lambda = rhs satisfies every row but
    the pinned rail row.  What a tolerance-terminated solve must still get right."""
    c = np.array([0.25, -0.5, 2.0])
    sc = jc._bodies([c + x * np.array([0.0, 0.0, 1.0])], 1.0, 0.125)
    data = np.zeros((2, 7))
    data[0] = jr.lock_data(jc.EYE)
    data[1, 0:3], data[1, 3:6] = [0.0, 0.0, 1.0], c
    sc.update(kind=np.array([jr.LOCK, sr.SLIDER], np.int32), body0=np.zeros(2, np.int32), body1=np.full(2, -1, np.int32),
              data=data, dt=1.0 / 128, erp=0.25, motor=None, travel=None if travel is None else np.array([[-INF, INF], list(travel)]))
    return sc


def make_problem(ctx, sc, precision=None):
    pr = jc.make_problem(ctx, sc, precision)
    if sc.get("travel") is not None:
        pr.set_slider_limits(sc["travel"])
    return pr


# ---- ensembles of a world: dicts as tests/test_gpu_world_step_each.py's, with kinds, motors and travel stops -------------------
def _slider_rows(R0, axis_world, p0, D, p1=None, R1=None):
    """(lock row, slider row) of a slider that stands at D now."""
    return jr.lock_data(R0, R1), sr.slider_data(p0, R0, axis_world, D, p1)


def ens_piston(x, travel, axis=(0.0, 0.0, 1.0), origin=(0.0, 0.0, 2.0), motor=None, across=0.0, mass=1.0):
    """One box of mass `mass` on a rail to the world along `axis` through `origin`, at travel x (and `across` off the
    rail along y), with the travel stops given."""
    from test_gpu_world_step_each import bodies, ensemble
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    p0 = np.asarray(origin, float) + x * a + across * np.array([0.0, 1.0, 0.0])
    sc = bodies([p0])
    sc["mass"][:] = mass
    e = ensemble(sc)
    lock, sl = _slider_rows(jc.EYE, a, p0, p0 - np.asarray(origin, float))
    e["joints"] = (np.zeros(2, np.int32), np.full(2, -1, np.int32), np.vstack([lock, sl]))
    e["kinds"] = np.array([jr.LOCK, sr.SLIDER], np.int32)
    e["motors"] = None if motor is None else np.array([[0.0, -1.0], list(motor)])
    e["travel"] = None if travel is None else np.array([[-INF, INF], list(travel)])
    return e


def ens_pushed_pair(y=5.0, motor=(-0.5, 3.0)):
    """Two free boxes (no gravity) joined by an off-centre slider along x whose motor pushes them apart (dx/dt < 0: x is
    body 0's travel relative to body 1, and body 1 lies ahead of it on the rail): the rail passes 0.2 above body 0's
    centre (c != 0), body 1 sits 0.7 along it and 0.2 up."""
    from test_gpu_world_step_each import bodies, ensemble
    p = np.array([[0.0, y, 3.0], [0.7, y, 3.2]])
    e = ensemble(bodies(p))
    e["f_ext"][:] = 0.0
    a = np.array([1.0, 0.0, 0.0])
    D = -0.7 * a      # D = p0 + R0 c - p1 along the rail: x = -0.7, err = 0
    lock, sl = _slider_rows(jc.EYE, a, p[0], D, p[1], jc.EYE)
    e["joints"] = (np.zeros(2, np.int32), np.ones(2, np.int32), np.vstack([lock, sl]))
    e["kinds"] = np.array([jr.LOCK, sr.SLIDER], np.int32)
    e["motors"] = np.array([[0.0, -1.0], list(motor)])
    e["travel"] = None
    return e


def set_joints(w, ens, off):
    """test_gpu_joints_world.set_joints, then the ensembles' hinge limits (zeros where one has none) and travel stops
    (rows (-inf, +inf) where one has none)."""
    from test_gpu_joints_world import set_joints as base
    base(w, ens, off)
    lim = [e["limits"] if e.get("limits") is not None else np.zeros((len(e["joints"][0]), 8)) for e in ens if e["joints"] is not None]
    if any(e.get("limits") is not None for e in ens):
        w.set_joint_limits(np.concatenate(lim))
    rows, any_travel = [], False
    for e in ens:
        if e["joints"] is None:
            continue
        t = e.get("travel")
        rows.append(t if t is not None else np.tile([-INF, INF], (len(e["joints"][0]), 1)))
        any_travel = any_travel or t is not None
    if any_travel:
        w.set_slider_limits(np.concatenate(rows))


def make_world(ctx, ens, precision=None):
    """A plain world for one ensemble, a batched one for several: (world, body offsets)."""
    from eggshell_amd import capi
    precision = capi.F64 if precision is None else precision
    if len(ens) == 1:
        w, off = capi.World(ctx, ens[0]["p"].shape[0], precision), np.array([0, ens[0]["p"].shape[0]])
    else:
        w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens], precision)
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6))
    set_joints(w, ens, off)
    return w, off
