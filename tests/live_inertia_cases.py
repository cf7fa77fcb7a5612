"""Shared by the live-inertia tests (CPU and GPU): the brick, the skip rule, the host route -- what the device's refresh
computes, from the oracle functions -- and the oracle twin of the free brick."""
import numpy as np

from eggshell_amd import scenes
from oracle import oracle as orc

DT = 1e-3
# a box of sides 0.1 x 0.3 x 0.6, mass 1: y is its intermediate axis
BRICK = np.diag([(0.3 ** 2 + 0.6 ** 2) / 12.0, (0.1 ** 2 + 0.6 ** 2) / 12.0, (0.1 ** 2 + 0.3 ** 2) / 12.0])
# a rotation that is no symmetry of the brick (the unit quaternion along (0.5, 0.1, -0.7, 0.5))
_Q = np.array([0.5, 0.1, -0.7, 0.5]) / np.linalg.norm([0.5, 0.1, -0.7, 0.5])
R_START = scenes._quat_to_R(*_Q)
STARTS = {"random": (R_START, np.array([1.0, 2.0, 3.0])),
          "intermediate": (np.eye(3).reshape(9), np.array([0.05, 5.0, 0.05]))}


def is_skipped(I_body):
    """The rule of egs_problem_set_live_inertia, per body: inertia_body is exactly a * I_3."""
    I = np.asarray(I_body, np.float64).reshape(-1, 9)
    off = (I[:, [1, 2, 3, 5, 6, 7]] == 0).all(axis=1)
    return off & (I[:, 0] == I[:, 4]) & (I[:, 0] == I[:, 8])


def host_mass(R, w, mass, I_body, Minv, f_ext, torque=None):
    """Minv [n][36] and f_ext [n][6] after a refresh at (R, w): the oracle's values in the angular 3x3 / the torque rows
    of every body that is not skipped, everything else as given."""
    n = mass.shape[0]
    live = ~is_skipped(I_body)
    Mo = orc.minv_blocks(R, mass, I_body).reshape(n, 6, 6)
    fo = orc.external_force(R, w, mass, I_body).reshape(n, 6)
    M = np.array(Minv, np.float64).reshape(n, 6, 6).copy()
    f = np.array(f_ext, np.float64).reshape(n, 6).copy()
    M[live, 3:, 3:] = Mo[live, 3:, 3:]
    f[live, 3:] = fo[live, 3:] if torque is None else np.asarray(torque, np.float64).reshape(n, 3)[live] + fo[live, 3:]
    return M.reshape(n, 36), f


def momentum(R, w, I_body=BRICK):
    Rm = np.asarray(R).reshape(3, 3)
    return Rm @ I_body @ Rm.T @ np.asarray(w).reshape(3)


class Tumble:
    """Follows one free brick step by step: the drift of L = I_g w, the kinetic energy, the sign changes of the
    body-frame w_y."""

    def __init__(self, R, w):
        self.L0 = momentum(R, w)
        self.E0 = 0.5 * np.dot(np.asarray(w).reshape(3), self.L0)
        self.drift, self.energy_change, self.flips, self.step = 0.0, 0.0, [], 0
        self.last = (np.asarray(R).reshape(3, 3).T @ np.asarray(w).reshape(3))[1]

    def see(self, R, w):
        self.step += 1
        L = momentum(R, w)
        self.drift = max(self.drift, np.linalg.norm(L - self.L0) / np.linalg.norm(self.L0))
        self.energy_change = abs(0.5 * np.dot(np.asarray(w).reshape(3), L) - self.E0) / self.E0
        wy = (np.asarray(R).reshape(3, 3).T @ np.asarray(w).reshape(3))[1]
        if wy * self.last < 0:
            self.flips.append(self.step)
        if wy != 0:
            self.last = wy


def free_brick_bodies(start, z=50.0):
    """The one-body scene of a start: arrays for World.set_bodies, with the oracle's Minv / f_ext at the start."""
    R, w = STARTS[start]
    sc = dict(p=np.array([[0.0, 0.0, z]]), R=np.asarray(R, np.float64).reshape(1, 9).copy(), v=np.zeros((1, 3)),
              w=w.reshape(1, 3).copy(), mass=np.ones(1), I_body=BRICK.reshape(1, 9).copy())
    sc["Minv"] = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    sc["f_ext"] = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    return sc


def twin_run(start, steps, live):
    """The oracle twin: Ensemble::Step of the free brick (no constraints: v_dot = M^-1 f, ensembles.cc:504-505), with
    Minv / f_ext recomputed at every step's start state (live) or frozen at the first (quirk Q5)."""
    sc = free_brick_bodies(start)
    p, R, v, w, Minv, f_ext = sc["p"], sc["R"], sc["v"], sc["w"], sc["Minv"], sc["f_ext"]
    none = np.zeros(0, np.int32)
    J, lam = np.zeros((0, 18)), np.zeros(0)
    t = Tumble(R, w)
    for _ in range(steps):
        if live:
            Minv, f_ext = host_mass(R, w, sc["mass"], sc["I_body"], Minv, f_ext)
        v6 = orc.velocity_update(v, w, Minv, f_ext, none, none, J, J, lam, DT)
        p, R = orc.position_update(p, R, np.concatenate([v, w], axis=1), v6, DT)
        v, w = v6[:, :3].copy(), v6[:, 3:].copy()
        t.see(R, w)
    return t, dict(p=p, R=R, v=v, w=w)


def brick_chain(n=4, seed=5):
    """scenes.chain(n) with brick inertias and small seeded spins: the joints hold, the links tumble."""
    sc = scenes.chain(n)
    rng = np.random.default_rng(seed)
    sc["I_body"] = np.tile(BRICK.reshape(9), (n, 1))
    sc["w"] = rng.uniform(-0.3, 0.3, (n, 3))
    sc["Minv"] = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    sc["f_ext"] = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    return sc
