"""The combined-feature scenes of tests/test_combo_reference_cpu.py and tests/test_gpu_world_combo.py: small seeded
worlds in which the features that each have a test of their own are on TOGETHER.

Features
  K   joint kinds: a ball joint to the world, a weld (ball + lock), a hinge (ball + axis) whose motor sits on its
      torque limit; the hinged body stands on the ground, so joints and contacts share an island
  P   the friction pyramid, mu >= 0
  R   restitution with vth > 0; a bouncing, a floor and a slow contact are all present in the first step
  W   warm start
  L   live inertia: box inertias (non-spherical) and non-zero w
  S   shapes: spheres beside boxes of unequal sides
  E   a batched world driven by step_each
  32  fp32
  H   hinge angle limits: a door on a vertical hinge to the world, with a motor and both stops, that swings past its
      upper stop after the first step
  D   sliders with a motor and travel stops: a drawer on a cabinet that starts past its lower stop, is driven through its
      range and past its upper stop; a platform on a rail to the world that is dropped onto its lower stop
  C   capsules: a log lying in the ground, a ball on its side and a log across it, a log leaning on the cabinet, a log on
      the platform
  Y   a table of rays cast between the steps: fixed ones and ones riding on a loose body, on the door and on a capsule

The scenes of the first eight features are TABLE / NAMES; those that add H, D, C and Y are PLUS_TABLE / PLUS_NAMES (up to
18 bodies and about 45 constraints), kept in a list of their own because the CPU test holds the first to 12 bodies.

A scene is a Scene (below): the ensembles (dicts as tests/test_gpu_world_step_each.py's, plus mass, I_body, side, shape,
kinds, motors), the world's settings, and per step the (dt [E], erp [E]) it is stepped with.  Each is 4 steps long.
The bodies are drawn from a seed; SEEDS holds, per scene, the first seed from 1 on at which no decision of any
reference lies inside a guard band in any of the four steps (redraw(); combo_reference.left_out counts them) and the
scene shows what it is there to show (accepts()).  tests/test_combo_reference_cpu.py asserts both for the seeds recorded
here."""
import functools
import math

import numpy as np

import inertia_reference as ir
import joint_reference as jr
from oracle import oracle as orc

BOX, SPHERE, CAPSULE = 0, 1, 2
SLIDER = 5      # EGS_JOINT_SLIDER_AXIS (slider_reference.SLIDER)
FEATURES = ("K", "P", "R", "W", "L", "S", "E", "32", "H", "D", "C", "Y")
INF = math.inf
STEPS = 4
DT, ERP, VTH, RADIUS = 5e-3, 0.2, 0.1, 0.01
MU, REST = 0.5, 0.5
SWEEPS, CFM = 12, 0.01
MOTOR = (3.0, 0.05)      # rad/s, N m: the ground holds the hinged body back, the motor saturates
DOOR_MOTOR = (3.0, 0.05)      # the door turns at 1 rad/s: this motor saturates too, until the stop takes its row
DOOR_HOLD = (1.0, 0.05)       # DENSE+: no stop ever takes the row, so the motor holds the door's own speed and the cold start
                              # lambda = rhs is near the solution (a start of 600 on a 1 kg door puts 2e4 into a carried
                              # accumulator, whose rounding the class bounds, stated at the final x, do not cover)
DOOR_RANGE, DOOR_GAP = (-0.5, 0.3), 3e-3      # rad; the door starts DOOR_GAP short of its upper stop
DRAWER_MOTOR = (0.4, 30.0)      # m/s, N: holds the drawer's speed, 2 mm a step
DRAWER_TRAVEL = (2e-4, 4.4e-3)      # m, from x = 0 at the start: past the lower stop, then inside, past the upper in step 3
PLATFORM_STOP, PLATFORM_V = -4e-4, -0.2      # m, m/s: under its stop after the first step


class Scene:
    def __init__(self, name, features, ens, mu, rest, rates, entry="step", f32=False, method=1):
        self.name, self.features, self.ens = name, frozenset(features), ens
        self.mu, self.rest, self.vth = mu, rest, VTH       # per ensemble, or None: never set
        self.warm, self.radius = "W" in features, RADIUS
        self.live, self.shapes, self.kinds = "L" in features, "S" in features, "K" in features
        self.limits, self.travel, self.capsules, self.rays = ("H" in features, "D" in features, "C" in features, "Y" in features)
        self.rates, self.entry, self.f32 = rates, entry, f32
        self.prm = dict(method=method, max_iters=SWEEPS, tol=0.0, cfm=CFM, omega=1.5)
        self.base, self.index = name, 0                    # single(): the scene it was taken from, and which ensemble

    def single(self, e):
        """The scene that holds ensemble e alone, stepped with that ensemble's rates through plain step."""
        s = Scene("%s[%d]" % (self.name, e), self.features - {"E"}, [self.ens[e]], None if self.mu is None else [self.mu[e]],
                  None if self.rest is None else [self.rest[e]], [([dt[e]], [erp[e]]) for dt, erp in self.rates], "step", self.f32,
                  self.prm["method"])
        s.base, s.index = self.name, e
        return s


# ---- bodies ------------------------------------------------------------------------------------------------------------------
def _yaw(a):
    c, s = math.cos(a), math.sin(a)
    return [c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0]


def _axis_frame(u):
    """Row-major R whose column 2 is the unit vector along u (a capsule's axis), column 1 horizontal."""
    u = np.asarray(u, np.float64) / np.linalg.norm(u)
    b = np.cross([0.0, 0.0, 1.0], u)
    b = np.array([0.0, 1.0, 0.0]) if np.linalg.norm(b) < 1e-12 else b / np.linalg.norm(b)
    return list(np.stack([np.cross(b, u), b, u], axis=1).reshape(9))


class _Bodies:
    def __init__(self, rng):
        self.rng, self.rows = rng, []

    def add(self, p, side, shape=BOX, yaw=None, v=(0.0, 0.0, 0.0), spin=0.2, jitter=0.01, axis=None, w=None):
        """axis: a capsule's axis in the world (side = (d, d, l); a box's inertia, so that live inertia follows it).
        w: added to the drawn spin."""
        rng = self.rng
        mass = float(rng.uniform(0.5, 2.0))
        p = np.array(p, np.float64) + np.append(rng.uniform(-jitter, jitter, 2), 0.0)
        if shape == SPHERE:
            side = (side, side, side)
            I = np.eye(3) * (0.4 * mass * (side[0] / 2) ** 2)
            yaw = 0.0
        else:
            I = np.diag(ir.box_inertia(*side, m=mass))
            yaw = float(rng.uniform(-0.3, 0.3)) if yaw is None else yaw
        R = _yaw(yaw) if axis is None else _axis_frame(axis)
        spun = rng.uniform(-spin, spin, 3) + (0.0 if w is None else np.asarray(w, np.float64))
        self.rows.append(dict(p=p, R=R, v=v, w=spun, mass=mass, I=I.reshape(9), side=side, shape=shape))
        return len(self.rows) - 1

    def ensemble(self):
        n = len(self.rows)
        col = lambda k, d: np.array([r[k] for r in self.rows], np.float64).reshape(n, d)
        e = dict(p=col("p", 3), R=col("R", 9), v=col("v", 3), w=col("w", 3), mass=col("mass", 1).reshape(n), I_body=col("I", 9),
                 side=col("side", 3), shape=np.array([r["shape"] for r in self.rows], np.int32))
        e["Minv"] = orc.minv_blocks(e["R"], e["mass"], e["I_body"]).reshape(n, 36)
        e["f_ext"] = orc.external_force(e["R"], e["w"], e["mass"], e["I_body"]).reshape(n, 6)
        e.update(joints=None, kinds=None, motors=None, limits=None, travel=None, rays=None)
        return e


def _loose(b, x0=0.0, y0=0.0):
    """Six bodies that meet the ground and each other: a flat box at rest (slow contacts) with a ball leaning on its
    +x face; a ball arriving at 2 m/s (it bounces, and leaves the ground two steps later); a box 5 mm deep sinking at
    0.2 m/s (the Baumgarte floor wins) that carries a smaller turned box; a cube that lands in the second step."""
    b.add([x0, y0, 0.1 - 1e-3], (0.4, 0.3, 0.2), yaw=0.0, jitter=0.0)
    b.add([x0 + 0.2 + 0.15 - 2e-3, y0, 0.15 - 1e-3], 0.3, SPHERE, jitter=0.0)
    b.add([x0 + 1.0, y0, 0.12 - 1e-3], 0.24, SPHERE, v=(0.0, 0.0, -2.0))
    k = b.add([x0, y0 + 1.0, 0.125 - 5e-3], (0.3, 0.5, 0.25), v=(0.0, 0.0, -0.2), spin=0.02)
    top = b.rows[k]["p"] + np.array([0.0, 0.0, 0.125 + 0.15 - 1e-3])
    b.add(top, (0.2, 0.2, 0.3), v=(0.0, 0.0, -0.2), spin=0.02, jitter=0.0)
    b.add([x0 + 2.0, y0, 0.15 + 4e-3], (0.3, 0.3, 0.3), v=(0.0, 0.0, -1.0))


def _jointed(b, kinds, y0=-1.5, z0=0.3, grounded=True):
    """Three links along x: link A on a ball joint to the world, link B welded to A, link C hinged to B about y with a
    motor.  C is a tall box whose foot is 1 mm in the ground (grounded) -- the contacts and the joints share an island.
    kinds False: the ball joints alone (no lock, no axis row, no motor)."""
    first = len(b.rows)
    for i, side in enumerate(((0.3, 0.3, 0.2), (0.3, 0.2, 0.2), (0.2, 0.2, 2 * z0 + 2e-3 if grounded else 0.3))):
        b.add([0.6 * i, y0, z0], side, yaw=0.0, jitter=0.0, spin=0.1)
    A, B, C = first, first + 1, first + 2
    eye = np.eye(3).reshape(9)
    ball = lambda c0, c1: np.array(list(c0) + list(c1) + [0.0])
    rows = [(jr.BALL, A, -1, ball((-0.3, 0.0, 0.0), (-0.3, y0, z0)), (0.0, -1.0)),
            (jr.BALL, A, B, ball((0.3, 0.0, 0.0), (-0.3, 0.0, 0.0)), (0.0, -1.0)),
            (jr.BALL, B, C, ball((0.3, 0.0, 0.0), (-0.3, 0.0, 0.0)), (0.0, -1.0))]
    if kinds:
        rows.insert(2, (jr.LOCK, A, B, jr.lock_data(eye, eye), (0.0, -1.0)))
        rows.append((jr.HINGE, B, C, jr.hinge_data(eye, (0.0, 1.0, 0.0), eye), MOTOR))
    return rows


def _with_joints(e, rows, kinds):
    """rows: (kind, body0, body1, data, motor) and, for the stops, two further entries: the hinge-limit row [8] and the
    travel row (xlo, xhi), either None."""
    e["joints"] = (np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows]))
    if kinds:
        e["kinds"], e["motors"] = np.array([r[0] for r in rows], np.int32), np.array([r[4] for r in rows], np.float64)
    if any(len(r) > 5 and r[5] is not None for r in rows):
        e["limits"] = np.array([r[5] if len(r) > 5 and r[5] is not None else np.zeros(8) for r in rows])
    if any(len(r) > 6 and r[6] is not None for r in rows):
        e["travel"] = np.array([r[6] if len(r) > 6 and r[6] is not None else (-INF, INF) for r in rows], np.float64)
    return e


NO_MOTOR = (0.0, -1.0)
EYE9 = np.eye(3).reshape(9)


def _door(b, limits, y0=-3.0, z0=1.0, motor=None):
    """A door, 0.6 long, on a vertical hinge (ball joint + hinge axis) to the world through (0, y0, z0), turning at
    1 rad/s towards its upper stop DOOR_GAP away; the motor asks for 3 rad/s and sits on its torque limit while it owns
    the row.  limits False: the same door without the table."""
    import limit_reference as lr
    D = b.add([0.3, y0, z0], (0.6, 0.05, 0.4), yaw=0.0, jitter=0.0, spin=0.02, v=(0.0, 0.3, 0.0), w=(0.0, 0.0, 1.0))
    lim = lr.limit_row(EYE9, (0.0, 0.0, 1.0), None, DOOR_RANGE[1] - DOOR_GAP, *DOOR_RANGE) if limits else None
    return D, [(jr.BALL, D, -1, np.array([-0.3, 0.0, 0.0, 0.0, y0, z0, 0.0]), NO_MOTOR),
               (jr.HINGE, D, -1, jr.hinge_data(EYE9, (0.0, 0.0, 1.0)), DOOR_MOTOR if motor is None else motor, lim, None)]


LEAN = math.radians(60.0)      # the leaning log's angle to the ground
LOG_R = 0.05


def _drawer(b, travel, capsules, y0=-4.5):
    """A cabinet standing 1 mm in the ground and a drawer hung beside it on a rail along x (lock + slider between the
    two), moving at the motor's speed; with capsules a log leans on the cabinet's upper -x edge, its foot 1 mm in the
    ground and its shaft 1 mm in the edge.  travel False: no table (the motor owns the rail row throughout)."""
    import slider_reference as sr
    cab = b.add([0.0, y0, 0.2 - 1e-3], (0.4, 0.4, 0.4), yaw=0.0, jitter=0.0, spin=0.02)
    drw = b.add([0.6, y0, 0.3], (0.3, 0.2, 0.1), yaw=0.0, jitter=0.0, spin=0.0, v=(DRAWER_MOTOR[0], 0.0, 0.0))
    p0, p1 = b.rows[drw]["p"], b.rows[cab]["p"]
    rows = [(jr.LOCK, drw, cab, jr.lock_data(EYE9, EYE9), NO_MOTOR),
            (SLIDER, drw, cab, sr.slider_data(p0, EYE9, (1.0, 0.0, 0.0), np.zeros(3), p1), DRAWER_MOTOR, None,
             DRAWER_TRAVEL if travel else None)]
    if capsules:
        d = LOG_R - 1e-3                                    # the shaft's distance from the edge
        edge, foot_z = np.array([-0.2, 0.2 - 1e-3 + 0.2]), LOG_R - 1e-3
        u = np.array([math.cos(LEAN), 0.0, math.sin(LEAN)])
        foot_x = edge[0] - (d + (edge[1] - foot_z) * math.cos(LEAN)) / math.sin(LEAN)
        half = 0.3
        b.add(np.array([foot_x, y0, foot_z]) + half * u, (2 * LOG_R, 2 * LOG_R, 2 * half + 2 * LOG_R), CAPSULE, axis=u, jitter=0.0, spin=0.02)
    return rows


def _platform(b, travel, capsules, y0=-6.0, z0=1.0):
    """A platform on a vertical rail to the world (lock + slider, no motor) with a lower stop only, dropped at PLATFORM_V
    from just above the stop; with capsules a log lies on it, moving with it, 1 mm in its top face."""
    import slider_reference as sr
    v = (0.0, 0.0, PLATFORM_V)
    P = b.add([0.0, y0, z0], (0.5, 0.5, 0.1), yaw=0.0, jitter=0.0, spin=0.0, v=v)
    p0 = b.rows[P]["p"]
    rows = [(jr.LOCK, P, -1, jr.lock_data(EYE9), NO_MOTOR),
            (SLIDER, P, -1, sr.slider_data(p0, EYE9, (0.0, 0.0, 1.0), np.zeros(3)), NO_MOTOR, None, (PLATFORM_STOP, INF) if travel else None)]
    if capsules:
        b.add([0.0, y0, z0 + 0.05 + LOG_R - 1e-3], (2 * LOG_R, 2 * LOG_R, 0.4), CAPSULE, axis=(1.0, 0.02, 0.0), jitter=0.0, spin=0.02, v=v)
    return rows


def _logs(b, x0=0.0, y0=-7.5):
    """A log lying along x 1 mm in the ground (two contacts under the flat rule), a ball 1 mm in its side off the crest,
    and a thinner log across it, 1 mm in its crest."""
    r = 0.1
    g = b.add([x0, y0, r - 1e-3], (2 * r, 2 * r, 0.6), CAPSULE, axis=(1.0, 0.0, 0.0), jitter=0.0, spin=0.02)
    n = np.array([0.0, 0.6, 0.8])
    b.add(b.rows[g]["p"] + np.array([0.05, 0.0, 0.0]) + n * (2 * r - 1e-3), 2 * r, SPHERE, jitter=0.0, spin=0.1)
    b.add(b.rows[g]["p"] + np.array([-0.15, 0.0, r + LOG_R - 1e-3]), (2 * LOG_R, 2 * LOG_R, 0.5), CAPSULE, axis=(0.03, 1.0, 0.0), jitter=0.0, spin=0.02)
    return g


def _rays(b, fixed, riders):
    """The ray table of an ensemble: fixed = [(origin, dir, tmax)] in the world frame, riders = [(body, origin, dir,
    tmax)] with a world direction turned into the carrier's frame at its first pose."""
    o, d, t, body = [], [], [], []
    for origin, dirn, tmax in fixed:
        o.append(origin); d.append(dirn); t.append(tmax); body.append(-1)
    for k, origin, dirn, tmax in riders:
        R = np.array(b.rows[k]["R"]).reshape(3, 3)
        o.append(origin); d.append(R.T @ np.asarray(dirn, np.float64)); t.append(tmax); body.append(k)
    return dict(origin=np.array(o, np.float64), dir=np.array(d, np.float64), tmax=np.array(t, np.float64), body=np.array(body, np.int32))


def ens_plus(seed, feats, part="all", dense=False):
    """An ensemble of the PLUS scenes.  part "all": the loose bodies, the jointed links, the door, the drawer, the
    platform and the logs; "loose": the loose bodies and the logs, no joints; "joints": links off the ground, a door and a
    platform, no contacts.  dense: every rail and axis row is motored and none has a stop, and the platform is left out
    (a rail row without a motor is a pinned row, which the dense step refuses)."""
    on = lambda f: f in feats
    kinds = on("K")      # without K: the links' ball joints alone, no door, drawer or platform
    b = _Bodies(np.random.default_rng(seed))
    rows, riders, fixed, door = [], [], [], None
    down, y_loose = (0.0, 0.0, -1.0), 4.0 if part == "loose" else 0.0
    if part != "joints":
        _loose(b, y0=y_loose)
        # onto the flat box, the leaning ball, the arriving ball, past everything to the ground; two that miss
        fixed += [((0.05, y_loose + 0.02, 2.0), down, INF), ((0.34, y_loose, 2.0), down, INF), ((1.0, y_loose + 0.01, 2.0), down, 5.0),
                  ((3.0, y_loose + 0.5, 2.0), down, INF), ((3.0, y_loose, 2.0), (0.0, 0.0, 1.0), INF), ((3.0, y_loose, 2.0), down, 1.5)]
        riders += [(2, (0.0, 0.0, 0.0), down, INF), (4, (0.0, 0.0, 0.0), down, INF), (5, (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), INF)]
    if part == "all":
        rows += _jointed(b, kinds)
    elif part == "joints":
        rows += _jointed(b, True, y0=8.0, z0=2.0, grounded=False)
        fixed += [((0.6, 8.0, 4.0), down, INF), ((0.6, 8.0, 4.0), (0.0, 0.0, 1.0), INF)]
        riders += [(0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), INF)]
    if part != "loose" and kinds:
        door, r = _door(b, on("H") and not dense, motor=DOOR_HOLD if dense else None)
        rows += r
        # a fixed ray down just ahead of the door's leading face (it is swept after two steps), one riding on the door
        fixed += [((0.55, -3.0 + 0.025 + 3.0e-3, 3.0), down, INF)]
        riders += [(door, (0.0, 0.0, -0.25), down, INF), (door, (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), 2.0)]
    if part == "all" and kinds and (on("D") or dense):
        rows += _drawer(b, not dense, on("C"))
        fixed += [((0.6, -4.5, 2.0), down, INF), ((-2.0, -4.5, 0.3), (1.0, 0.0, 0.0), INF)]
    if part != "loose" and kinds and on("D") and not dense:
        rows += _platform(b, True, on("C") and part == "all", y0=-6.0 if part == "all" else 12.0)
        if part == "all":
            fixed += [((0.01, -6.0, 3.0), down, INF)]
    if part != "joints" and on("C"):
        g = _logs(b, y0=-7.5 if part == "all" else y_loose - 3.0)
        gy = b.rows[g]["p"][1]
        fixed += [((0.25, gy, 2.0), down, INF), ((-0.15, gy + 0.1, 2.0), down, INF)]
        riders += [(g + 2, (0.0, 0.0, 0.0), down, INF)]
    if part == "loose":
        fixed += [((0.05, 0.02, 2.0), down, INF)]      # over another ensemble's flat box: the ground, for this one
    e = b.ensemble()
    if rows:
        _with_joints(e, rows, kinds)
    if on("Y"):
        e["rays"] = _rays(b, fixed, riders)
    return e


def ens_all(seed, kinds=True):
    """The loose bodies and the jointed links in one ensemble."""
    b = _Bodies(np.random.default_rng(seed))
    _loose(b)
    rows = _jointed(b, kinds)      # (adds the links' bodies: before ensemble() is taken)
    return _with_joints(b.ensemble(), rows, kinds)


def ens_loose(seed):
    b = _Bodies(np.random.default_rng(seed))
    _loose(b, y0=4.0)
    return b.ensemble()


def ens_joints_only(seed):
    b = _Bodies(np.random.default_rng(seed))
    rows = _jointed(b, True, y0=8.0, z0=2.0, grounded=False)
    return _with_joints(b.ensemble(), rows, True)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
ALL6 = ("K", "P", "R", "W", "L", "S")
PLAIN = [([DT], [ERP])] * STEPS
BATCH_RATES = [([5e-3, 2.5e-3, 4e-3], [0.2, 0.1, 0.3]), ([5e-3, 0.0, 4e-3], [0.2, 0.1, 0.3]),
               ([5e-3, 2.5e-3, 4e-3], [0.2, 0.1, 0.3]), ([4e-3, 5e-3, 2.5e-3], [0.3, 0.2, 0.1])]
# name -> (features, entry, f32)
TABLE = {"ALL": (ALL6, "step", False), "ALL32": (ALL6 + ("32",), "step", True),
         "ALL32-each": (ALL6 + ("32", "E"), "step_each", True),
         "BATCH": (ALL6 + ("E",), "step_each", False), "BATCH-step": (ALL6, "step", False),
         "DENSE": (("K", "R", "W", "L", "S"), "dense", False)}
for _x in ALL6:
    TABLE["ALL-minus-" + _x] = (tuple(f for f in ALL6 if f != _x), "step", False)
TABLE["ALL-minus-R-each"] = (tuple(f for f in ALL6 if f != "R") + ("E",), "step_each", False)
NAMES = sorted(TABLE)

# the scenes with hinge stops, sliders, capsules and rays beside the first six
ALL10 = ALL6 + ("H", "D", "C", "Y")
PLUS_TABLE = {"ALL+": (ALL10, "step", False), "ALL+32": (ALL10 + ("32",), "step", True),
              "ALL+32-each": (ALL10 + ("32", "E"), "step_each", True),
              "BATCH+": (ALL10 + ("E",), "step_each", False), "BATCH+-step": (ALL10, "step", False),
              "DENSE+": (("K", "R", "W", "L", "S", "C"), "dense", False)}
for _x in ("H", "D", "C"):
    PLUS_TABLE["ALL+-minus-" + _x] = (tuple(f for f in ALL10 if f != _x), "step", False)
PLUS_TABLE["ALL+-minus-R-each"] = (tuple(f for f in ALL10 if f != "R") + ("E",), "step_each", False)
# ... and the rows that launch the assemble_kernel instantiations no row above reaches (tests/test_gpu_world_combo.py has the table)
_less = lambda *out: tuple(f for f in ALL10 if f not in out)
PLUS_TABLE.update({"ALL+32-minus-R": (_less("R") + ("32",), "step", True), "ALL+32-minus-D": (_less("D") + ("32",), "step", True),
                   "ALL+32-minus-DR": (_less("D", "R") + ("32",), "step", True),
                   "ALL+32-minus-R-each": (_less("R") + ("32", "E"), "step_each", True),
                   "ALL+-minus-D-each": (_less("D") + ("E",), "step_each", False),
                   "ALL+32-minus-D-each": (_less("D") + ("32", "E"), "step_each", True),
                   "ALL+32-minus-DR-each": (_less("D", "R") + ("32", "E"), "step_each", True),
                   # fp32 without a stop table and without restitution (the angular sites), and without joint kinds (the plain ones)
                   "ALL+32-minus-HDR": (_less("H", "D", "R") + ("32",), "step", True),
                   "ALL+32-minus-HDR-each": (_less("H", "D", "R") + ("32", "E"), "step_each", True),
                   "ALL+32-minus-KHDY": (_less("K", "H", "D", "Y") + ("32",), "step", True),
                   "ALL+32-minus-KHDY-each": (_less("K", "H", "D", "Y") + ("32", "E"), "step_each", True)})
PLUS_NAMES = sorted(PLUS_TABLE)
EVERY_TABLE = dict(TABLE, **PLUS_TABLE)


def pairs_covered():
    """{frozenset((a, b)): [scene names]} over both tables above: which scenes have both features on.  (The dense
    entry is no feature; that it refuses a stop is tests/test_gpu_world_combo.py's refusal test.)"""
    out = {}
    for a in FEATURES:
        for b in FEATURES:
            if a < b:
                out[frozenset((a, b))] = [n for n in sorted(EVERY_TABLE) if a in EVERY_TABLE[n][0] and b in EVERY_TABLE[n][0]]
    return out


def build_plus(name, seed):
    feats, entry, f32 = PLUS_TABLE[name]
    on = lambda f: f in feats
    if name.startswith("BATCH"):
        ens = [ens_plus(seed, feats), ens_plus(seed + 1000, feats, "loose"), ens_plus(seed + 2000, feats, "joints")]
        rates = BATCH_RATES if entry == "step_each" else [([DT] * 3, [ERP] * 3)] * STEPS
        return Scene(name, feats, ens, [0.5, 0.2, 0.8], [0.5, -1.0, 0.3], rates, entry, f32)
    ens = [ens_plus(seed, feats, dense=entry == "dense")]
    rates = [([4e-3], [0.3])] * STEPS if entry == "step_each" else PLAIN
    return Scene(name, feats, ens, [MU] if on("P") else None, [REST] if on("R") else None, rates, entry, f32)


def build(name, seed):
    if name in PLUS_TABLE:
        return build_plus(name, seed)
    feats, entry, f32 = TABLE[name]
    on = lambda f: f in feats
    if name.startswith("BATCH"):
        ens = [ens_all(seed), ens_loose(seed + 1000), ens_joints_only(seed + 2000)]
        rates = BATCH_RATES if entry == "step_each" else [([DT] * 3, [ERP] * 3)] * STEPS
        return Scene(name, feats, ens, [0.5, 0.2, 0.8], [0.5, -1.0, 0.3], rates, entry, f32)
    ens = [ens_all(seed, kinds=on("K"))]
    rates = [([4e-3], [0.3])] * STEPS if entry == "step_each" else PLAIN
    return Scene(name, feats, ens, [MU] if on("P") else None, [REST] if on("R") else None, rates, entry, f32)


# the first accepted seed of every scene (redraw(name) finds it; the CPU test holds them to accepts() and left_out == 0)
SEEDS = {n: 1 for n in NAMES}
SEEDS.update({n: 1 for n in PLUS_NAMES})


@functools.lru_cache(maxsize=None)
def scene(name):
    return build(name, SEEDS[name])


def redraw(name, first=1, tries=50):
    """The first seed from `first` on whose twin run leaves nothing out of any property and shows what the scene is
    there to show."""
    import combo_reference as cr
    for seed in range(first, first + tries):
        sc = build(name, seed)
        runs = [cr.twin_run(sc.single(e) if len(sc.ens) > 1 else sc) for e in range(len(sc.ens))]
        if all(sum(r["left_out"].values()) == 0 for run in runs for r in run) and not accepts(sc, runs):
            return seed
    raise AssertionError("%s: no seed in %d..%d is clear of the guard bands" % (name, first, first + tries - 1))


def accepts(sc, runs):
    """What the twin run of a scene must show, as a list of complaints (empty: accepted).  runs[e] = the records of
    ensemble e (combo_reference.twin_run)."""
    bad = []
    run = runs[0]                                     # ensemble 0 holds every feature of the scene
    counts = [len(r["contacts"][0]) for r in run]
    if not any(a != b for a, b in zip(counts, counts[1:])):
        bad.append("the contact count never changes: %s" % counts)
    if sc.rest is not None and sc.entry != "dense":
        seen = set(run[0]["what"])
        if not {"bounce", "floor", "slow"} <= seen:
            bad.append("restitution decisions of step 0: %s" % sorted(seen))
    if sc.kinds:
        e = sc.ens[0]
        hinge = int(np.nonzero(e["kinds"] == jr.HINGE)[0][0])
        C = int(e["joints"][1][hinge])
        if not all(abs(r["lam"][3 * hinge + 2]) == MOTOR[1] for r in run if r["dt"] != 0 and not r.get("dense")):
            bad.append("the motor is not on its torque limit in every sweep step")
        if not any((r["contacts"][1] == C).any() for r in run):
            bad.append("the hinged body never touches anything")
    mj = len(sc.ens[0]["joints"][0])
    if sc.warm and sc.entry == "dense":
        if not (run[2]["src"][mj:] >= 0).any():
            bad.append("warm start: no contact of the sweep step after a dense step takes the dense lambda")
    elif sc.warm and not any((r["src"][mj:] >= 0).any() and (r["src"][mj:] == -1).any() for r in run if r["src"] is not None):
        bad.append("warm start: no step with matched and unmatched contacts")
    return bad + _accepts_plus(sc, run, mj, counts)


def _accepts_plus(sc, run, mj, counts):
    """What the scenes with stops, capsules and rays must show beside the above."""
    bad = []
    e = sc.ens[0]
    swept = [r for r in run if r["dt"] != 0 and not r.get("dense")]
    if (sc.limits and e["limits"] is not None) or (sc.travel and e["travel"] is not None):
        stopped = [i for i in range(mj) if (sc.limits and e["limits"] is not None and e["limits"][i, 4:8].any()) or
                   (sc.travel and e["travel"] is not None and np.isfinite(e["travel"][i]).any())]
        for i in stopped:
            acts = {int(r["tw"]["active"][i]) for r in swept}
            if not (0 in acts and len(acts) > 1):
                bad.append("the stop of joint %d is not seen both inactive and active: %s" % (i, sorted(acts)))
        if sc.warm:
            changed = 0
            for a, r in zip(run, run[1:]):
                for i in stopped:
                    k = 3 * i + 2
                    if (a["tw"]["lo"][k], a["tw"]["hi"][k]) != (r["tw"]["lo"][k], r["tw"]["hi"][k]):
                        changed += 1
                        if r["src"][i] != i or not np.array_equal(r["x0"][3 * i:3 * i + 3], a["lam"][3 * i:3 * i + 3]):
                            bad.append("joint %d: a row whose bounds changed does not start from its own previous rows" % i)
            if not changed:
                bad.append("warm start: no stop row changes its bounds between two steps")
        if not any(a != b and r["tw"]["active"].any() for a, b, r in zip(counts, counts[1:], run[1:])):
            bad.append("the contact count never changes in a step with an active stop: %s" % counts)
    if sc.capsules:
        shape = e["shape"]
        kinds = {tuple(sorted((int(shape[i]) if i >= 0 else -1, int(shape[j])))) for r in run for i, j in zip(*r["contacts"][:2])}
        want = {(-1, CAPSULE), (SPHERE, CAPSULE), (CAPSULE, CAPSULE)} | ({(BOX, CAPSULE)} if e["kinds"] is not None and (e["kinds"] == SLIDER).any() else set())
        if not want <= kinds:
            bad.append("capsule pair kinds without a contact: %s" % sorted(want - kinds))
        logs = [b for b in np.nonzero(shape == CAPSULE)[0] if sum(1 for i, j in zip(*run[0]["contacts"][:2]) if i == -1 and j == b) == 2]
        if not logs:
            bad.append("no log with two ground contacts in the first step")
    if sc.rays:
        hits = [r["rays"][0] for r in run]
        if not any(((a != b) & (a > -2) & (b > -2)).any() for a, b in zip(hits, hits[1:])):
            bad.append("no ray's nearest hit changes body between two steps")
        seen = {int(shape_of) for h in hits for shape_of in np.where(h >= 0, e["shape"][np.maximum(h, 0)], h)}
        if not {-2, -1, BOX, SPHERE} | ({CAPSULE} if sc.capsules else set()) <= seen:
            bad.append("rays: not every shape, the ground and a miss are seen: %s" % sorted(seen))
    return bad


# ---- worlds ----------------------------------------------------------------------------------------------------------------------
def make_world(ctx, sc):
    """The scene's world with every setting applied: (world, body offsets)."""
    from eggshell_amd import capi
    ens = sc.ens
    prec = capi.F32 if sc.f32 else capi.F64
    if len(ens) == 1:
        w, off = capi.World(ctx, ens[0]["p"].shape[0], prec), np.array([0, ens[0]["p"].shape[0]])
    else:
        w, off = capi.World.batch(ctx, [e["p"].shape[0] for e in ens], prec)
    cat = lambda k, d: np.concatenate([e[k].reshape(-1, d) for e in ens])
    w.set_bodies(cat("p", 3), cat("R", 9), cat("v", 3), cat("w", 3), cat("Minv", 36), cat("f_ext", 6), side=cat("side", 3))
    if sc.shapes:
        w.set_shapes(np.concatenate([e["shape"] for e in ens]))
    j = joint_table(sc, off)
    if j is not None:
        kind, b0, b1, data, motor = j
        if sc.kinds:
            w.set_joints_kinds(kind, b0, b1, data)
            w.set_joint_motors(motor)
        else:
            w.set_joints(b0, b1, data)
    lim, travel = stop_tables(sc)
    if lim is not None:
        w.set_joint_limits(lim)
    if travel is not None:
        w.set_slider_limits(travel)
    rays = ray_table(sc, off)
    if rays is not None:
        w.set_rays(rays["origin"], rays["dir"], rays["tmax"], rays["body"], rays["ens"] if len(ens) > 1 else None)
    if sc.live:
        w.set_live_inertia(cat("I_body", 9))
    if sc.mu is not None:
        w.set_friction(np.array(sc.mu))
    if sc.rest is not None:
        w.set_restitution(np.array(sc.rest), sc.vth)
    if sc.warm:
        w.set_warm_start(True, sc.radius)
    return w, off


def joint_table(sc, off):
    """(kind, body0, body1, data, motor) of all ensembles' joints with global body indices, or None."""
    kind, b0, b1, data, motor = [], [], [], [], []
    for e, o in zip(sc.ens, off):
        if e["joints"] is None:
            continue
        j0, j1, jd = e["joints"]
        b0.append(np.where(j0 >= 0, j0 + o, -1)); b1.append(np.where(j1 >= 0, j1 + o, -1)); data.append(jd)
        kind.append(e["kinds"] if e["kinds"] is not None else np.zeros(len(j0), np.int32))
        motor.append(e["motors"] if e["motors"] is not None else np.tile([0.0, -1.0], (len(j0), 1)))
    if not b0:
        return None
    return (np.concatenate(kind).astype(np.int32), np.concatenate(b0).astype(np.int32), np.concatenate(b1).astype(np.int32),
            np.concatenate(data), np.concatenate(motor))


def stop_tables(sc):
    """(hinge limits [mj][8] or None, travel stops [mj][2] or None) over all ensembles' joints: an ensemble without a
    table has rows of zeros (no stop) and (-inf, +inf)."""
    with_joints = [e for e in sc.ens if e["joints"] is not None]
    lim = travel = None
    if sc.limits and any(e["limits"] is not None for e in with_joints):
        lim = np.concatenate([e["limits"] if e["limits"] is not None else np.zeros((len(e["joints"][0]), 8)) for e in with_joints])
    if sc.travel and any(e["travel"] is not None for e in with_joints):
        travel = np.concatenate([e["travel"] if e["travel"] is not None else np.tile([-INF, INF], (len(e["joints"][0]), 1))
                                 for e in with_joints])
    return lim, travel


def ray_table(sc, off):
    """The world's ray table: the ensembles' rays one after the other with global carrier indices and `ens` per ray, or
    None for a scene without rays."""
    if not sc.rays:
        return None
    out = {k: np.concatenate([e["rays"][k] for e in sc.ens]) for k in ("origin", "dir", "tmax")}
    out["body"] = np.concatenate([np.where(e["rays"]["body"] >= 0, e["rays"]["body"] + o, -1) for e, o in zip(sc.ens, off)]).astype(np.int32)
    out["ens"] = np.concatenate([np.full(len(e["rays"]["body"]), k, np.int32) for k, e in enumerate(sc.ens)])
    return out
