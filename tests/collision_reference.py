"""Box-box and box-ground contact geometry as mathematics, in mpmath at 50 digits: an INDEPENDENT reference for what
oracle/collision.c restates in fp64 and collide.hip mirrors bit for bit.  Nothing here follows collision.c's operation
order, works in a box's own frame, clips a polygon or returns a "code": it states which pairs are separated, which axis
carries the contact normal and how deep the boxes are, and which properties every reported contact has.

A box is (centre c, row-major R whose COLUMNS are its axes in world coordinates, side lengths); h = side / 2.

  axes         the 15 candidates of the separating-axis theorem: A_0..A_2, B_0..B_2 and A_i x B_j.  A cross product of
               length zero is no axis; the reference skips those shorter than 1e-9
  separation   s(a) = (|a.d| - sum_k h1_k |a.A_k| - sum_k h2_k |a.B_k|) / |a|,  d = c2 - c1
  decision     separated  <=>  max s > 0
  aacount      number of columns of |R1^T R2| (entries |A_i.B_j|) whose largest entry exceeds 0.9962
  sF, sE       largest separation over the face axes / over the edge axes

Colliding pairs (collision.cc:166-388):

  edge case    aacount == 0 and sE > sF: exactly ONE contact; normal = that edge axis, unit, signed towards box 2
               (sgn(a.d)); depth = -sE.  Beyond the issue's list: the two points pos +- depth/2 normal lie on the two
               edge LINES (|q_m| = h_m for the two coordinates across the edge direction), which pins the position.
  face case    otherwise.  The normal of every contact is the face axis of sF signed towards box 2.  Its owner is box
               A, the other is B, An = the normal pointing from A to B, face centre = cA + h_k An.  For every contact
                 depth == -(An.(pos - face centre)),  depth >= 0,
                 pos on the surface of B: max_k |q_k| / hB_k - 1 == 0 with q = RB^T (pos - cB),
                 pos inside A's two lateral slabs: |A_m.(pos - cA)| <= hA_m, m != k.
  fallback     one contact at c2 (these bits) with the face normal and depth == -sF.

Ground (collision.cc:408-436): the corners c + R (+-h) in the reference's order (x outermost, z innermost, -1 before
+1); a corner is a contact iff z < 0, and the contact is (corner, (0,0,1), -z).

Knife edges.  The reference's constants make some decisions arbitrarily close calls in fp64.  A pair (or contact, or
body) is left out of a property, and COUNTED, when the deciding quantity lies within a guard band of its threshold:
1e-9 for separations, lengths and the 0.9962 test, 1e-12 for a corner's z.  Deciding quantities: max s, and any single
s, against 0; a column maximum against 0.9962; a non-zero edge-axis length against 1e-9; only where they decide (edge
case possible, i.e. aacount == 0): sF against sE and the two largest edge separations against each other; in the face
case the face separations within 1e-9 of sF: one -> that axis; two that are parallel axes of the two boxes (a shared
axis, |A_k x B_l| < 1e-9) -> the normal must be one of them and the face properties may hold under either owner;
anything else -> left out.  |a.d| / |a| of the deciding axis against 0 (the sign of the normal).  |depth| of a reported
face contact against 1e-9 unless aacount >= 2 (the reference drops clipped vertices that shallow).

Tolerance: normals, depths, on-surface and slab distances at 1e-12 absolute (TOL), the project's bound for short fp64
chains on quantities of order 1; see DESIGN.md "Collision against a 50-digit reference".

The seeded case families at the end are shared by the CPU test (oracle against this reference) and the GPU tests
(device against this reference), so both see identical inputs; their references are computed once per process."""
import functools

import mpmath as mp
import numpy as np
from scipy.spatial.transform import Rotation

DPS = 50
ALIGN = mp.mpf("0.9962")
LEN_TOL = mp.mpf("1e-9")
GUARD = mp.mpf("1e-9")
GUARD_Z = mp.mpf("1e-12")
TOL = 1e-12


def _v(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def _cols(R):
    f = _v(R)
    return [[f[j], f[3 + j], f[6 + j]] for j in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return mp.sqrt(_dot(a, a))


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _axpy(a, s, x):
    return [a[0] + s * x[0], a[1] + s * x[1], a[2] + s * x[2]]


class Axis:
    """One candidate axis: owner 1 / 2 (a face axis of that box, index k) or 0 (A_i x B_j); n = the unit axis signed
    towards box 2; s = the normalised separation; ad = |a.d| / |a|."""
    __slots__ = ("owner", "k", "i", "j", "n", "s", "ad")

    def __init__(self, owner, k, i, j, n, s, ad):
        self.owner, self.k, self.i, self.j, self.n, self.s, self.ad = owner, k, i, j, n, s, ad


class Box:
    __slots__ = ("c", "ax", "h")

    def __init__(self, c, R, side):
        self.c, self.ax, self.h = _v(c), _cols(R), [x / 2 for x in _v(side)]


class PairRef:
    """What the mathematics says about one ordered pair (box 1, box 2)."""

    def __init__(self, c1, R1, s1, c2, R2, s2):
        with mp.workdps(DPS):
            self.box = (None, Box(c1, R1, s1), Box(c2, R2, s2))
            b1, b2 = self.box[1], self.box[2]
            self.c2_bits = np.asarray(c2, dtype=np.float64).reshape(3).copy()
            d = _sub(b2.c, b1.c)
            r1 = mp.sqrt(_dot(b1.h, b1.h)); r2 = mp.sqrt(_dot(b2.h, b2.h))
            self.spheres_apart = mp.sqrt(_dot(d, d)) > r1 + r2     # then the boxes are separated, whatever the axes say
            self.guards = []                  # why the pair is left out of the properties that follow the decision
            self.faces, self.edges = [], []

            def axis(a, owner, k, i, j):
                ln = mp.sqrt(_dot(a, a))
                ad = _dot(a, d)
                span = sum(b1.h[q] * abs(_dot(a, b1.ax[q])) for q in range(3)) + \
                    sum(b2.h[q] * abs(_dot(a, b2.ax[q])) for q in range(3))
                sg = 1 if ad >= 0 else -1
                return Axis(owner, k, i, j, [sg * x / ln for x in a], (abs(ad) - span) / ln, abs(ad) / ln)

            for k in range(3):
                self.faces.append(axis(b1.ax[k], 1, k, None, None))
            for k in range(3):
                self.faces.append(axis(b2.ax[k], 2, k, None, None))
            for i in range(3):
                for j in range(3):
                    a = _cross(b1.ax[i], b2.ax[j])
                    ln = mp.sqrt(_dot(a, a))
                    if ln == 0:
                        continue
                    if abs(ln - LEN_TOL) < GUARD:
                        self.guards.append("edge-axis length")
                    if ln > LEN_TOL:
                        self.edges.append(axis(a, 0, None, i, j))
            allax = self.faces + self.edges
            self.max_s = max(a.s for a in allax)
            self.decision_guard = any(abs(a.s) < GUARD for a in allax)
            self.separated = self.max_s > 0
            colmax = [max(abs(_dot(b1.ax[i], b2.ax[j])) for i in range(3)) for j in range(3)]
            self.aacount = sum(1 for m in colmax if m > ALIGN)
            if any(abs(m - ALIGN) < GUARD for m in colmax):
                self.guards.append("0.9962")
            self.sF = max(a.s for a in self.faces)
            self.sE = max(a.s for a in self.edges) if self.edges else None
            self.kind, self.normals = None, []
            edge_possible = self.aacount == 0 and self.sE is not None
            if edge_possible and abs(self.sF - self.sE) < GUARD:
                self.guards.append("sF against sE")
            if edge_possible and self.sE > self.sF:
                self.kind = "edge"
                top = sorted(self.edges, key=lambda a: a.s, reverse=True)
                if len(top) > 1 and top[0].s - top[1].s < GUARD:
                    self.guards.append("two largest edge separations")
                self.normals = [top[0]]
            else:
                self.kind = "face"
                top = [a for a in self.faces if self.sF - a.s < GUARD]
                if len(top) == 2 and top[0].owner != top[1].owner and _norm(_cross(top[0].n, top[1].n)) < LEN_TOL:
                    self.normals = top        # a shared axis: either owner
                elif len(top) == 1:
                    self.normals = top
                else:
                    self.guards.append("two largest face separations")
                    self.normals = top
            if any(a.ad < GUARD for a in self.normals):
                self.guards.append("sign of the normal")

    @property
    def excluded(self):
        return self.decision_guard or bool(self.guards)


class Tally:
    """Worst errors and the counts the caps are stated in."""

    def __init__(self):
        self.normal = self.depth = self.surface = self.slab = self.edge_pos = self.ground = 0.0
        self.candidates = self.colliding = self.excluded = 0
        self.decision_checked = self.normal_checked = self.face_checked = self.edge_checked = self.fallbacks = 0
        self.contacts_checked = self.contacts_excluded = 0
        self.bodies = self.bodies_excluded = self.ground_contacts = 0
        self.aacount_seen = set()

    def line(self, who):
        return ("%s: worst normal %.3g depth %.3g on-surface %.3g slab %.3g edge-position %.3g ground %.3g | "
                "%d candidate pairs, %d colliding, %d excluded; decision on %d, normal on %d, face properties on %d "
                "(%d contacts, %d shallow ones left out), edge on %d, fallback %d; aacount seen %s; "
                "%d ground contacts, %d of %d bodies left out"
                % (who, self.normal, self.depth, self.surface, self.slab, self.edge_pos, self.ground, self.candidates,
                   self.colliding, self.excluded, self.decision_checked, self.normal_checked, self.face_checked,
                   self.contacts_checked, self.contacts_excluded, self.edge_checked, self.fallbacks,
                   sorted(self.aacount_seen), self.ground_contacts, self.bodies_excluded, self.bodies))

    def assert_caps(self, f):
        """The share of pairs the properties must reach: a condition of the test, so that leaving pairs out cannot
        pass for checking them."""
        if f in (2, 3):     # shared axes: ties everywhere, yet the normal is decided and half the pairs have a face
            assert self.normal_checked >= 0.9 * self.colliding, (self.normal_checked, self.colliding)
            assert self.face_checked >= 0.5 * self.colliding, (self.face_checked, self.colliding)
        else:
            assert self.excluded <= 0.02 * self.candidates, (self.excluded, self.candidates)
        assert self.bodies_excluded <= 0.02 * self.bodies, (self.bodies_excluded, self.bodies)
        assert self.colliding >= 200 and self.ground_contacts >= 20     # the family still collides


def _err(a, b):
    return float(max(abs(x - y) for x, y in zip(a, b)))


def _face_errors(ref, ax, contacts, shallow_ok):
    """The face-case properties of `contacts` (rows pos, normal, depth) with `ax` as the normal's axis.
    Returns (normal, depth, surface, slab, most negative depth) errors and how many shallow contacts were left out."""
    A, B = ref.box[ax.owner], ref.box[3 - ax.owner]
    An = ax.n if ax.owner == 1 else [-x for x in ax.n]
    fc = _axpy(A.c, A.h[ax.k], An)
    en = ed = es = el = neg = 0.0
    left_out = 0
    for row in contacts:
        pos, nrm, depth = _v(row[0:3]), _v(row[3:6]), mp.mpf(float(row[6]))
        en = max(en, _err(nrm, ax.n))
        if not shallow_ok and abs(abs(depth) - LEN_TOL) < GUARD:
            left_out += 1
            continue
        ed = max(ed, float(abs(depth + _dot(An, _sub(pos, fc)))))
        q = _sub(pos, B.c)
        es = max(es, float(abs(max(abs(_dot(B.ax[k], q)) / B.h[k] for k in range(3)) - 1)))
        q = _sub(pos, A.c)
        for m in range(3):
            if m != ax.k:
                el = max(el, float(abs(_dot(A.ax[m], q)) - A.h[m]))
        neg = max(neg, float(-depth))
    return (en, ed, es, el, neg), left_out


def check_pair(ref, contacts, tally, who=""):
    """Asserts every property the reference states for this pair on `contacts` ([n][7]: pos, normal, depth; n == 0:
    the pair was reported separated), and records errors and counts in `tally`."""
    contacts = np.asarray(contacts, dtype=np.float64).reshape(-1, 7)
    with mp.workdps(DPS):
        tally.candidates += 1
        if ref.decision_guard:
            tally.excluded += 1
            tally.colliding += 0 if ref.separated else 1
            return
        tally.decision_checked += 1
        assert (len(contacts) == 0) == bool(ref.separated), \
            "%s: %d contacts, but the largest separation is %s" % (who, len(contacts), mp.nstr(ref.max_s, 6))
        if ref.separated:
            return
        tally.colliding += 1
        if ref.guards:
            tally.excluded += 1
            return
        tally.aacount_seen.add(ref.aacount)
        if ref.kind == "edge":
            ax = ref.normals[0]
            assert len(contacts) == 1, "%s: edge case with %d contacts" % (who, len(contacts))
            pos, nrm, depth = _v(contacts[0, 0:3]), _v(contacts[0, 3:6]), mp.mpf(float(contacts[0, 6]))
            en, ed = _err(nrm, ax.n), float(abs(depth + ax.s))
            ep = 0.0
            for sign, box, along in ((1, ref.box[1], ax.i), (-1, ref.box[2], ax.j)):
                q = _sub(_axpy(pos, sign * depth / 2, nrm), box.c)
                for m in range(3):
                    if m != along:
                        ep = max(ep, float(abs(abs(_dot(box.ax[m], q)) - box.h[m])))
            tally.normal, tally.depth, tally.edge_pos = max(tally.normal, en), max(tally.depth, ed), max(tally.edge_pos, ep)
            tally.normal_checked += 1
            tally.edge_checked += 1
            assert en <= TOL and ed <= TOL and ep <= TOL, "%s: edge contact: normal %.3g depth %.3g position %.3g" % (who, en, ed, ep)
            return
        if len(contacts) == 1 and np.array_equal(contacts[0, 0:3], ref.c2_bits):       # the fallback
            nrm, depth = _v(contacts[0, 3:6]), mp.mpf(float(contacts[0, 6]))
            en = min(_err(nrm, ax.n) for ax in ref.normals)
            ed = float(abs(depth + ref.sF))
            tally.normal, tally.depth = max(tally.normal, en), max(tally.depth, ed)
            tally.normal_checked += 1
            tally.fallbacks += 1
            assert en <= TOL and ed <= TOL, "%s: fallback contact: normal %.3g depth %.3g" % (who, en, ed)
            return
        best = None
        for ax in ref.normals:                                   # one axis, or the two owners of a shared axis
            e, left_out = _face_errors(ref, ax, contacts, ref.aacount >= 2)
            if best is None or max(e) < max(best[0]):
                best = (e, left_out)
        (en, ed, es, el, neg), left_out = best
        tally.normal, tally.depth = max(tally.normal, en), max(tally.depth, ed)
        tally.surface, tally.slab = max(tally.surface, es), max(tally.slab, el)
        tally.normal_checked += 1
        tally.contacts_excluded += left_out
        tally.contacts_checked += len(contacts) - left_out
        if left_out:
            tally.excluded += 1
        if left_out < len(contacts):
            tally.face_checked += 1
        assert en <= TOL and ed <= TOL and es <= TOL and el <= TOL and neg <= TOL, \
            "%s: face contacts: normal %.3g depth %.3g on-surface %.3g outside a slab by %.3g, depth below zero by %.3g" \
            % (who, en, ed, es, el, neg)


def ground_reference(c, R, side):
    """[(corner, z)] in the reference's order, and whether some corner's z is within GUARD_Z of 0."""
    with mp.workdps(DPS):
        b = Box(c, R, side)
        out = []
        for x in (-1, 1):
            for y in (-1, 1):
                for z in (-1, 1):
                    v = _axpy(_axpy(_axpy(b.c, x * b.h[0], b.ax[0]), y * b.h[1], b.ax[1]), z * b.h[2], b.ax[2])
                    out.append(v)
        return out, any(abs(v[2]) < GUARD_Z for v in out)


def check_ground(gref, contacts, tally, who=""):
    corners, guard = gref
    contacts = np.asarray(contacts, dtype=np.float64).reshape(-1, 7)
    tally.bodies += 1
    if guard:
        tally.bodies_excluded += 1
        return
    with mp.workdps(DPS):
        below = [v for v in corners if v[2] < 0]
        assert len(contacts) == len(below), "%s: %d ground contacts, %d corners below z = 0" % (who, len(contacts), len(below))
        for row, v in zip(contacts, below):
            assert row[3] == 0.0 and row[4] == 0.0 and row[5] == 1.0, who
            e = max(_err(_v(row[0:3]), v), float(abs(mp.mpf(float(row[6])) + v[2])))
            tally.ground = max(tally.ground, e)
            tally.ground_contacts += 1
            assert e <= TOL, "%s: ground contact off by %.3g" % (who, e)


# ---- seeded case families ------------------------------------------------------------------------------------------
N_BODIES = 50
FAMILIES = (0, 1, 2, 3, 4)
SEEDS = {0: 7100, 1: 7101, 2: 7102, 3: 7103, 4: 7104}


def _permuted(M, shift):
    """Cyclic permutation of the columns (the box's axes change names, the box does not turn; det stays +1)."""
    return M[:, [(k + shift) % 3 for k in range(3)]]


@functools.lru_cache(maxsize=None)
def family(f):
    """(p[50][3], R[50][9], side[50][3]), read-only.  0: random rotations; 1: one frame x a small rotation x a cyclic
    axis permutation (nearly aligned, aacount 1-3); 2: the frame x a rotation about its own z x the permutation (the
    z axis is shared EXACTLY: the same bits in every body); 3: the frame x the permutation (exactly parallel boxes);
    4: family 0 with three of every ten bodies thin (a side of 0.01) or long (a side of 1.2)."""
    rng = np.random.default_rng(SEEDS[f])
    n = N_BODIES
    p = rng.uniform([-0.5, -0.5, 0.0], [0.5, 0.5, 0.7], (n, 3))
    side = rng.uniform(0.08, 0.6, (n, 3))
    frame = Rotation.from_quat(rng.normal(size=4)).as_matrix()
    R = np.zeros((n, 3, 3))
    if f in (0, 4):
        R[:] = Rotation.from_quat(rng.normal(size=(n, 4))).as_matrix()
    for b in range(n):
        if f == 1:
            R[b] = _permuted(frame @ Rotation.from_rotvec(rng.normal(size=3) * 0.03).as_matrix(), b % 3)
        elif f == 2:
            M = frame @ Rotation.from_rotvec([0.0, 0.0, rng.uniform(0.2, 1.4)]).as_matrix()
            M[:, 2] = frame[:, 2]
            R[b] = _permuted(M, b % 3)
        elif f == 3:
            R[b] = _permuted(frame, b % 3)
    if f == 4:
        for b in range(n):
            if b % 10 < 3:
                side[b, rng.integers(3)] = 0.01 if rng.integers(2) else 1.2
    out = (p, R.reshape(n, 9).copy(), side)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family_reference(f):
    """({(i, j): PairRef} for every pair i < j whose bounding spheres touch, [ground_reference per body]); every other
    pair is separated.  Computed once per process and shared."""
    p, R, side = family(f)
    return scene_reference(p, R, side)


def scene_reference(p, R, side):
    n = p.shape[0]
    r = 0.5 * np.linalg.norm(side, axis=1)
    pairs = {}
    for i in range(n):
        for j in range(i + 1, n):
            if np.linalg.norm(p[i] - p[j]) > (r[i] + r[j]) * (1 + 1e-9):
                continue                    # clearly apart in fp64; PairRef decides the rest exactly
            ref = PairRef(p[i], R[i], side[i], p[j], R[j], side[j])
            if not ref.spheres_apart:
                pairs[(i, j)] = ref
    return pairs, [ground_reference(p[b], R[b], side[b]) for b in range(n)]


def check_scene(refs, b0, b1, data, tally, who=""):
    """A whole contact list (ground contacts (-1, b), then pairs (i, j)) against a scene's reference: every reported
    pair collides, every omitted pair is separated, and every property holds."""
    pairs, grounds = refs
    b0, b1, data = np.asarray(b0), np.asarray(b1), np.asarray(data, dtype=np.float64).reshape(-1, 7)
    by_pair = {}
    for k in range(len(b0)):
        by_pair.setdefault((int(b0[k]), int(b1[k])), []).append(k)
    for b, g in enumerate(grounds):
        check_ground(g, data[by_pair.pop((-1, b), [])], tally, "%s ground %d" % (who, b))
    for key, ref in pairs.items():
        check_pair(ref, data[by_pair.pop(key, [])], tally, "%s pair %s" % (who, key))
    assert not by_pair, "%s: contacts between pairs whose bounding spheres are apart: %s" % (who, sorted(by_pair))
