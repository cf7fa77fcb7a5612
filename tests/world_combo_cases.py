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

BOX, SPHERE = 0, 1
FEATURES = ("K", "P", "R", "W", "L", "S", "E", "32")
STEPS = 4
DT, ERP, VTH, RADIUS = 5e-3, 0.2, 0.1, 0.01
MU, REST = 0.5, 0.5
SWEEPS, CFM = 12, 0.01
MOTOR = (3.0, 0.05)      # rad/s, N m: the ground holds the hinged body back, the motor saturates


class Scene:
    def __init__(self, name, features, ens, mu, rest, rates, entry="step", f32=False, method=1):
        self.name, self.features, self.ens = name, frozenset(features), ens
        self.mu, self.rest, self.vth = mu, rest, VTH       # per ensemble, or None: never set
        self.warm, self.radius = "W" in features, RADIUS
        self.live, self.shapes, self.kinds = "L" in features, "S" in features, "K" in features
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


class _Bodies:
    def __init__(self, rng):
        self.rng, self.rows = rng, []

    def add(self, p, side, shape=BOX, yaw=None, v=(0.0, 0.0, 0.0), spin=0.2, jitter=0.01):
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
        self.rows.append(dict(p=p, R=_yaw(yaw), v=v, w=rng.uniform(-spin, spin, 3), mass=mass, I=I.reshape(9), side=side, shape=shape))
        return len(self.rows) - 1

    def ensemble(self):
        n = len(self.rows)
        col = lambda k, d: np.array([r[k] for r in self.rows], np.float64).reshape(n, d)
        e = dict(p=col("p", 3), R=col("R", 9), v=col("v", 3), w=col("w", 3), mass=col("mass", 1).reshape(n), I_body=col("I", 9),
                 side=col("side", 3), shape=np.array([r["shape"] for r in self.rows], np.int32))
        e["Minv"] = orc.minv_blocks(e["R"], e["mass"], e["I_body"]).reshape(n, 36)
        e["f_ext"] = orc.external_force(e["R"], e["w"], e["mass"], e["I_body"]).reshape(n, 6)
        e.update(joints=None, kinds=None, motors=None)
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
    e["joints"] = (np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows]))
    if kinds:
        e["kinds"], e["motors"] = np.array([r[0] for r in rows], np.int32), np.array([r[4] for r in rows], np.float64)
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


def pairs_covered():
    """{frozenset((a, b)): [scene names]} over the table above: which scenes have both features on."""
    out = {}
    for a in FEATURES:
        for b in FEATURES:
            if a < b:
                out[frozenset((a, b))] = [n for n in NAMES if a in TABLE[n][0] and b in TABLE[n][0]]
    return out


def build(name, seed):
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
