"""ctypes binding of libeggshell_amd.so (the C ABI in include/eggshell_amd.h).

Plumbing only: numpy arrays in, numpy arrays out.  There is NO CPU fallback;
if the library is missing or no gfx950 device is usable the calls raise.
"""
import ctypes as C
import ctypes as _ct   # for the methods that call an argument C, as the reference does
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libeggshell_amd.so")

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_STALL, ERR_UNSUPPORTED, ERR_LCP_FAILED, ERR_INTERNAL = range(8)
JACOBI, GAUSS_SEIDEL, SOR = 0, 1, 2
F64, F32 = 0, 1
JOINT_BALL, CONTACT_BOX, JOINT_LOCK, JOINT_HINGE_AXIS = 0, 1, 2, 3
JOINT_SLIDER_AXIS = 5   # 4 is no kind (it stays invalid)
SHAPE_BOX, SHAPE_SPHERE, SHAPE_CAPSULE = 0, 1, 2
MV_LOWER, MV_UPPER, MV_DIAG, MV_FULL = 1, 2, 4, 8
SCHED_QUAD, SCHED_ISO, SCHED_QUAD_PATCHES, SCHED_LANE_PATCHES, SCHED_ALL_GLOBAL, SCHED_STATIC, SCHED_LEAN = 1, 2, 4, 8, 16, 32, 64   # SCHED_LEAN: reserved, never reported
SCHED_LINSYM = 128
SCHED_FUSED_ASSEMBLY = 256
SCHED_DEFERRED_SYSTEM = 512
SCHED_START = 1024
SCHED_FRICTION = 2048
SCHED_PAIR = 4096
SCHED_CHAIN = 8192
SCHED_SHARE = 16384
SCHED_FACE = 32768
SCHED_FACE_SPLIT = 65536
SCHED_FACE_LEAN = 131072
START_RHS, START_GIVEN, START_PREVIOUS = 0, 1, 2
STABILIZE_INIT, STABILIZE_POST = 0, 1

# every symbol include/eggshell_amd.h declares
EXPORTS = [
    "egs_default_params", "egs_context_create", "egs_context_destroy", "egs_last_error",
    "egs_context_synchronize", "egs_context_cu_count", "egs_timer_start", "egs_timer_stop", "egs_kernel_time",
    "egs_solve_blocks", "egs_problem_create", "egs_problem_create_batch", "egs_problem_destroy", "egs_problem_set_blocks",
    "egs_problem_solve", "egs_problem_get_lambda", "egs_problem_get_accumulators",
    "egs_problem_set_state", "egs_problem_set_mass", "egs_problem_set_constraints", "egs_problem_assemble",
    "egs_problem_step", "egs_problem_get_blocks", "egs_problem_get_velocity",
    "egs_problem_advance", "egs_problem_get_state",
    "egs_problem_get_stats", "egs_problem_get_schedule", "egs_problem_get_schedule_full", "egs_problem_get_schedule_forms", "egs_mixed_constraints_solve", "egs_debug_plan", "egs_debug_plan_slots",
    "egs_update_contacts", "egs_update_contacts_joints", "egs_world_create", "egs_world_destroy", "egs_world_set_bodies",
    "egs_world_set_joints", "egs_world_step", "egs_world_get_bodies", "egs_world_get_contacts",
    "egs_world_get_lambda", "egs_world_info", "egs_world_create_batch", "egs_world_batch_info",
    "egs_problem_matvec", "egs_problem_get_matvec", "egs_problem_get_wres", "egs_matvec_blocks",
    "egs_debug_matvec_plan", "egs_debug_choose_oversize_schedule", "egs_debug_plan_timetable", "egs_debug_plan_pairable", "egs_debug_plan_chained", "egs_debug_plan_share", "egs_debug_plan_faced", "egs_debug_plan_face_normals", "egs_debug_face_split", "egs_debug_face_form", "egs_box_lcp_dantzig", "egs_box_lcp_murty",
    "egs_box_lcp_batch", "egs_box_lcp_schur", "egs_box_lcp_schur_batch", "egs_dense_condition", "egs_dense_iterate", "egs_dense_iterate_batch", "egs_debug_plan_patches", "egs_problem_debug_trace",
    "egs_mixed_constraints_solve_limits", "egs_mixed_constraints_solve_batch", "egs_problem_dense_system", "egs_problem_dense_condition", "egs_problem_step_dense",
    "egs_world_step_dense", "egs_world_dense_info", "egs_world_stabilize", "egs_world_stabilize_info",
    "egs_world_stabilize_direct", "egs_world_stabilize_rank", "egs_relax_blocks_direct",
    "egs_world_step_each", "egs_world_step_dense_each",
    "egs_problem_set_start", "egs_match_contacts", "egs_world_set_warm_start", "egs_world_get_start",
    "egs_problem_set_friction", "egs_world_set_friction",
    "egs_update_contacts_shapes", "egs_world_set_shapes",
    "egs_mixed_friction_solve_batch", "egs_problem_set_dense_friction", "egs_problem_dense_friction_info",
    "egs_world_set_dense_friction", "egs_world_dense_friction_info",
    "egs_problem_set_live_inertia", "egs_problem_get_mass", "egs_world_set_live_inertia", "egs_world_get_mass",
    "egs_problem_set_restitution", "egs_world_set_restitution",
    "egs_problem_set_motors", "egs_world_set_joints_kinds", "egs_world_set_joint_motors", "egs_world_get_blocks",
    "egs_problem_set_hinge_limits", "egs_world_set_joint_limits",
    "egs_problem_set_slider_limits", "egs_world_set_slider_limits",
    "egs_cast_rays", "egs_world_set_rays", "egs_world_cast_rays",
]


class SolveParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("max_iters", C.c_int32), ("check_every", C.c_int32),
                ("reserved", C.c_int32), ("omega", C.c_double), ("cfm", C.c_double),
                ("tol", C.c_double)]


class SolveStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("residual", C.c_double),
                ("n_islands", C.c_int32), ("n_tiles", C.c_int32), ("n_global", C.c_int32),
                ("reserved", C.c_int32), ("schedule", C.c_int32), ("tile_constraints", C.c_int32)]


class EgsError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("eggshell_amd status %d: %s" % (status, msg))
        self.status = status


_lib = None


def load():
    """Load the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                LIB_PATH + " is missing: run __graft_entry__.build() (there is no CPU fallback)")
        _lib = C.CDLL(LIB_PATH)
        _lib.egs_last_error.restype = C.c_char_p
        if hasattr(_lib, "egs_mixed_constraints_solve_batch"):      # (a timing tool may load an older build with --lib)
            # ctx, count, n, A, b, C, lo, hi, use_bounds, max_pivots, x, w, ok, pivots
            _lib.egs_mixed_constraints_solve_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] * 2 + [C.c_void_p] * 4
            _lib.egs_mixed_constraints_solve_batch.restype = C.c_int
        if hasattr(_lib, "egs_mixed_friction_solve_batch"):
            # ctx, count, n, A, b, C, lo, hi, normal_row, mu, max_pivots, max_outer, tol, x, w, beta, ok, pivots, outer, change
            _lib.egs_mixed_friction_solve_batch.argtypes = ([C.c_void_p, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32] * 2 + [C.c_double]
                                                            + [C.c_void_p] * 7)
            _lib.egs_mixed_friction_solve_batch.restype = C.c_int
            for name in ("egs_problem_set_dense_friction", "egs_world_set_dense_friction"):
                getattr(_lib, name).argtypes = [C.c_void_p, C.c_int32, C.c_double]
        if hasattr(_lib, "egs_problem_set_restitution"):
            _lib.egs_problem_set_restitution.argtypes = [C.c_void_p, C.c_void_p, C.c_double]   # problem, rest, vth
            _lib.egs_world_set_restitution.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double]   # world, E, rest, vth
        if hasattr(_lib, "egs_problem_set_motors"):
            _lib.egs_problem_set_motors.argtypes = [C.c_void_p, C.c_void_p]   # problem, motor
            _lib.egs_world_set_joints_kinds.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4   # world, m, kind, b0, b1, data
            _lib.egs_world_set_joint_motors.argtypes = [C.c_void_p, C.c_void_p]   # world, motor
            _lib.egs_world_get_blocks.argtypes = [C.c_void_p] * 8   # world, J0, J1, is_eq, lo, hi, rhs, err
            for name in ("egs_problem_set_motors", "egs_world_set_joints_kinds", "egs_world_set_joint_motors", "egs_world_get_blocks"):
                getattr(_lib, name).restype = C.c_int
        if hasattr(_lib, "egs_problem_set_hinge_limits"):
            for name in ("egs_problem_set_hinge_limits", "egs_world_set_joint_limits"):
                getattr(_lib, name).argtypes = [C.c_void_p, C.c_void_p]   # problem / world, lim
                getattr(_lib, name).restype = C.c_int
        if hasattr(_lib, "egs_problem_set_slider_limits"):
            for name in ("egs_problem_set_slider_limits", "egs_world_set_slider_limits"):
                getattr(_lib, name).argtypes = [C.c_void_p, C.c_void_p]   # problem / world, lim
                getattr(_lib, name).restype = C.c_int
        if hasattr(_lib, "egs_problem_set_live_inertia"):
            # handle, inertia_body, torque / handle, Minv, f_ext
            for name in ("egs_problem_set_live_inertia", "egs_problem_get_mass", "egs_world_set_live_inertia", "egs_world_get_mass"):
                getattr(_lib, name).argtypes = [C.c_void_p] * 3
                getattr(_lib, name).restype = C.c_int
        if hasattr(_lib, "egs_cast_rays"):
            # ctx, n, pos, R, side, shape, n_rays, ray_body, origin, dir, tmax, hit, t, normal
            _lib.egs_cast_rays.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 7
            _lib.egs_world_set_rays.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5   # world, n_rays, ens, body, o, d, tmax
            _lib.egs_world_cast_rays.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4   # world, max_rays, n_out, hit, t, normal
            for name in ("egs_cast_rays", "egs_world_set_rays", "egs_world_cast_rays"):
                getattr(_lib, name).restype = C.c_int
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


def _ray_arrays(origin, dir, tmax, ray_body):
    """(origin, dir, n_rays, tmax, ray_body) of the ray entries: contiguous, tmax None = +inf, shapes checked."""
    origin, dir = _f64(origin).reshape(-1, 3), _f64(dir).reshape(-1, 3)
    nr = origin.shape[0]
    tmax = np.full(nr, np.inf) if tmax is None else _f64(tmax).reshape(-1)
    ray_body = _i32(ray_body)
    if dir.shape[0] != nr or tmax.shape[0] != nr or (ray_body is not None and ray_body.shape != (nr,)):
        raise ValueError("origin, dir, tmax and ray_body must describe the same %d rays" % nr)
    return origin, dir, nr, tmax, ray_body


def _live_arrays(n, inertia_body, torque):
    """The two pointers of the set_live_inertia entries, shapes checked: [n][9] (or [n][3][3]) and [n][3]."""
    Ib, tq = _f64(inertia_body), _f64(torque)
    if Ib is not None and Ib.size != 9 * n:
        raise ValueError("inertia_body has %d entries for %d bodies" % (Ib.size, n))
    if tq is not None and (Ib is None or tq.size != 3 * n):
        raise ValueError("torque needs inertia_body and 3 entries for each of the %d bodies" % n)
    return _p(Ib), _p(tq)


def debug_plan_patches(n_bodies, body0, body1):
    """Host only: the body patches of an oversize island -- n_patches, patch / lane per constraint, remote flags per side."""
    b0, b1 = _i32(body0), _i32(body1)
    m = b0.shape[0]
    npat = C.c_int32(0)
    cp, cl, r0, r1 = (np.zeros(m, np.int32) for _ in range(4))
    st = load().egs_debug_plan_patches(C.c_int32(n_bodies), C.c_int32(m), _p(b0), _p(b1), C.byref(npat), _p(cp), _p(cl), _p(r0), _p(r1))
    if st != OK:
        raise RuntimeError("egs_debug_plan_patches failed: %d" % st)
    return npat.value, cp, cl, r0, r1


def lcp_batch_offsets(ns):
    """Offsets of the packed batch layout of egs_box_lcp_batch / egs_box_lcp_schur_batch: problem k's vectors start at
    vo[k] = sum_{j<k} n_j, its row-major matrix at ao[k] = sum_{j<k} n_j^2 (both int64, count + 1 entries)."""
    ns = np.asarray(ns, np.int64)
    return np.concatenate([[0], np.cumsum(ns)]).astype(np.int64), np.concatenate([[0], np.cumsum(ns * ns)]).astype(np.int64)


def pack_lcp_batch(As, bs, los, his):
    """Lists of matrices and vectors -> ns, A, b, lo, hi in the packed batch layout (host only)."""
    ns = np.array([np.shape(b)[0] for b in bs], np.int32)
    if len(As) != len(bs):
        raise ValueError("%d matrices for %d right-hand sides" % (len(As), len(bs)))
    for k, a in enumerate(As):
        if np.shape(a) != (ns[k], ns[k]):
            raise ValueError("problem %d: matrix %s for %d rows" % (k, np.shape(a), ns[k]))
    cat = lambda vs: np.concatenate([_f64(v).reshape(-1) for v in vs]) if len(vs) else np.zeros(0)
    return ns, cat(As), cat(bs), cat(los), cat(his)


def pack_batch_vectors(ns, vs, dtype=np.float64, what="vector"):
    """A list of per-problem vectors -> one packed array in the batch layout; every vector must have its problem's size."""
    if len(vs) != len(ns):
        raise ValueError("%d %ss for %d problems" % (len(vs), what, len(ns)))
    for k, v in enumerate(vs):
        if np.shape(v) != (ns[k],):
            raise ValueError("problem %d: %s %s for %d rows" % (k, what, np.shape(v), ns[k]))
    return np.concatenate([np.ascontiguousarray(v, dtype=dtype) for v in vs]) if len(vs) else np.zeros(0, dtype)


def unpack_lcp_batch(ns, A=None, *vectors):
    """The inverse of pack_lcp_batch: a list of n_k x n_k views of A (if given), then a list of n_k views per vector."""
    vo, ao = lcp_batch_offsets(ns)
    cnt = len(ns)
    out = []
    if A is not None:
        out.append([A[ao[k]:ao[k + 1]].reshape(ns[k], ns[k]) for k in range(cnt)])
    for v in vectors:
        out.append([v[vo[k]:vo[k + 1]] for k in range(cnt)])
    return out


def check_dense_iterate_batch(ns, A, b, C=None, lo=None, hi=None):
    """The size checks of Context.dense_iterate_batch_packed (host only): the packed arrays must hold exactly what the
    sizes ask for, and C, lo and hi come together.  Returns ns, A, b, C, lo, hi as the C ABI takes them.  (A size outside
    0..1024 is the library's to refuse; it counts as no rows here.)"""
    ns = np.asarray(ns)
    if ns.ndim != 1 or (ns.size and not np.issubdtype(ns.dtype, np.integer)):
        raise ValueError("ns: a list of integer sizes")
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    rows = np.maximum(ns, 0).astype(np.int64)
    tot = int(rows.sum())
    A, b, lo, hi = map(_f64, (A, b, lo, hi))
    C = _u8(C)
    if A.size != int((rows ** 2).sum()) or b.size != tot:
        raise ValueError("packed arrays do not match the sizes")
    given = [v is not None for v in (C, lo, hi)]
    if any(given) and not all(given):
        raise ValueError("C, lo and hi come together (or all None: every row an equality)")
    if all(given) and any(v.size != tot for v in (C, lo, hi)):
        raise ValueError("packed arrays do not match the sizes")
    return ns, A.reshape(-1), b.reshape(-1), C, lo, hi


def check_mixed_batch(ns, A, b, C, lo, hi):
    """The size checks of Context.mixed_constraints_solve_batch_packed (host only): the packed arrays must hold exactly
    what the sizes ask for.  Returns ns, A, b, C, lo, hi as the C ABI takes them.  (A negative size is the library's to
    refuse; it counts as no rows here.)"""
    ns = np.asarray(ns)
    if ns.ndim != 1 or (ns.size and not np.issubdtype(ns.dtype, np.integer)):
        raise ValueError("ns: a list of integer sizes")
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    rows = np.maximum(ns, 0).astype(np.int64)
    tot = int(rows.sum())
    if any(v is None for v in (A, b, C, lo, hi)):
        raise ValueError("A, b, C, lo and hi are all required")
    A, b, lo, hi = map(_f64, (A, b, lo, hi))
    C = _u8(C)
    if A.size != int((rows ** 2).sum()) or any(v.size != tot for v in (b, C, lo, hi)):
        raise ValueError("packed arrays do not match the sizes")
    return ns, A.reshape(-1), b.reshape(-1), C.reshape(-1), lo.reshape(-1), hi.reshape(-1)


def check_mixed_friction_batch(ns, A, b, C, lo, hi, normal_row, mu, max_outer=32, tol=1e-10):
    """The checks of Context.mixed_friction_solve_batch_packed that need no device: check_mixed_batch's, normal_row (integers)
    and mu packed like the vectors, max_outer an integer >= 0 and tol >= 0 (not NaN).  Returns ns, A, b, C, lo, hi,
    normal_row, mu as the C ABI takes them.  (What a normal_row may point at and the sign of mu are the library's to
    refuse.)"""
    ns, A, b, C, lo, hi = check_mixed_batch(ns, A, b, C, lo, hi)
    if normal_row is None or mu is None:
        raise ValueError("normal_row and mu are required")
    nr = np.asarray(normal_row)
    if nr.size and not np.issubdtype(nr.dtype, np.integer):
        raise ValueError("normal_row: integer row indices (-1: a plain row)")
    nr, mu = _i32(nr).reshape(-1), _f64(mu).reshape(-1)
    if nr.size != b.size or mu.size != b.size:
        raise ValueError("packed arrays do not match the sizes")
    if int(max_outer) != max_outer or max_outer < 0:
        raise ValueError("max_outer: an integer >= 0 (0: the default, 32)")
    if not tol >= 0:
        raise ValueError("tol must be >= 0")
    return ns, A, b, C, lo, hi, nr, mu


def params(method=GAUSS_SEIDEL, max_iters=500, tol=1e-9, cfm=0.0, omega=1.5, check_every=1):
    return SolveParams(method, max_iters, check_every, 0, omega, cfm, tol)


class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        self._children = weakref.WeakSet()   # problems / worlds must be destroyed before their context
        st = load().egs_context_create(C.c_int(device), C.byref(self.h))
        if st != OK:
            self.h = C.c_void_p()
            raise EgsError(st, "egs_context_create failed (no usable gfx950 device?)")

    def check(self, st):
        if st != OK:
            raise EgsError(st, load().egs_last_error(self.h).decode())

    def close(self):
        if self.h:
            for child in list(self._children):
                child.close()
            load().egs_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self.check(load().egs_context_synchronize(self.h))

    def cu_count(self):
        n = C.c_int32(0)
        self.check(load().egs_context_cu_count(self.h, C.byref(n)))
        return n.value

    def timer_start(self):
        self.check(load().egs_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float(0)
        self.check(load().egs_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def kernel_time(self, reset=True):
        s = C.c_double(0); n = C.c_int64(0)
        self.check(load().egs_kernel_time(self.h, C.byref(s), C.byref(n), C.c_int(1 if reset else 0)))
        return s.value, n.value

    def solve_blocks(self, Minv, body0, body1, J0, J1, is_eq, lo, hi, rhs, prm, precision=F64):
        """sparse::{Jacobi,GaussSeidel,SOR}Iteration on flat arrays (entry 1)."""
        Minv, J0, J1, lo, hi, rhs = map(_f64, (Minv, J0, J1, lo, hi, rhs))
        body0, body1, is_eq = _i32(body0), _i32(body1), _u8(is_eq)
        n = Minv.reshape(-1, 36).shape[0]
        m = body0.shape[0]
        x = np.zeros(3 * m)
        st = SolveStats()
        self.check(load().egs_solve_blocks(self.h, C.c_int32(n), _p(Minv), C.c_int32(m), _p(body0),
                                           _p(body1), _p(J0), _p(J1), _p(is_eq), _p(lo), _p(hi), _p(rhs),
                                           C.byref(prm), C.c_int32(precision), _p(x), C.byref(st)))
        return x, st

    def matvec_blocks(self, Minv, body0, body1, J0, J1, x, parts=MV_FULL, eps=0.0, scale=1.0, precision=F64):
        """sparse::CalculateSparse{JMJtX,Lx,Ux,Dx,...} on flat arrays (one-shot form)."""
        Minv, J0, J1, x = map(_f64, (Minv, J0, J1, x))
        body0, body1 = _i32(body0), _i32(body1)
        n, m = Minv.reshape(-1, 36).shape[0], body0.shape[0]
        y = np.zeros(3 * m)
        self.check(load().egs_matvec_blocks(self.h, C.c_int32(n), _p(Minv), C.c_int32(m), _p(body0), _p(body1),
                                            _p(J0), _p(J1), C.c_int32(parts), C.c_double(eps), C.c_double(scale),
                                            C.c_int32(precision), _p(x), _p(y)))
        return y

    def update_contacts(self, pos, R, side=None, max_contacts=None, joints=None):
        """Ensemble::UpdateContacts + contact pruning on the GPU (reference order).
        joints = (body0, body1, data[m][7]) adds the joint-vs-contact pruning."""
        pos, R = _f64(pos), _f64(R)
        if joints is not None:
            jb0, jb1, jd = _i32(joints[0]), _i32(joints[1]), _f64(joints[2])
            n = pos.reshape(-1, 3).shape[0]
            side = _f64(np.tile([0.3, 0.3, 0.3], (n, 1)) if side is None else side)
            cap = int(max_contacts if max_contacts is not None else 64 * n + 64)
            b0 = np.zeros(cap, np.int32); b1 = np.zeros(cap, np.int32); data = np.zeros((cap, 7))
            m = C.c_int32(0)
            self.check(load().egs_update_contacts_joints(self.h, C.c_int32(n), _p(pos), _p(R), _p(side),
                                                         C.c_int32(jb0.shape[0]), _p(jb0), _p(jb1), _p(jd), C.c_int32(cap),
                                                         C.byref(m), _p(b0), _p(b1), _p(data)))
            return b0[:m.value].copy(), b1[:m.value].copy(), data[:m.value].copy()
        n = pos.reshape(-1, 3).shape[0]
        side = _f64(np.tile([0.3, 0.3, 0.3], (n, 1)) if side is None else side)
        cap = int(max_contacts if max_contacts is not None else 64 * n + 64)
        b0 = np.zeros(cap, np.int32); b1 = np.zeros(cap, np.int32); data = np.zeros((cap, 7))
        m = C.c_int32(0)
        self.check(load().egs_update_contacts(self.h, C.c_int32(n), _p(pos), _p(R), _p(side), C.c_int32(cap),
                                              C.byref(m), _p(b0), _p(b1), _p(data)))
        return b0[:m.value].copy(), b1[:m.value].copy(), data[:m.value].copy()

    def update_contacts_shapes(self, pos, R, side, shape=None, max_contacts=None, joints=None):
        """update_contacts with a shape per body (egs_update_contacts_shapes): SHAPE_BOX / SHAPE_SPHERE /
        SHAPE_CAPSULE [n], a sphere's side row being (d, d, d) and a capsule's (d, d, l) with l > d, its axis column 2 of
        R; shape None = all boxes.  joints as in update_contacts."""
        pos, R, side, shape = _f64(pos), _f64(R), _f64(side), _i32(shape)
        n = pos.reshape(-1, 3).shape[0]
        jb0, jb1, jd = (_i32(joints[0]), _i32(joints[1]), _f64(joints[2])) if joints is not None else (None, None, None)
        mj = 0 if jb0 is None else jb0.shape[0]
        cap = int(max_contacts if max_contacts is not None else 64 * n + 64)
        b0 = np.zeros(cap, np.int32); b1 = np.zeros(cap, np.int32); data = np.zeros((cap, 7))
        m = C.c_int32(0)
        self.check(load().egs_update_contacts_shapes(self.h, C.c_int32(n), _p(pos), _p(R), _p(side), C.c_int32(mj),
                                                     _p(jb0), _p(jb1), _p(jd), _p(shape), C.c_int32(cap), C.byref(m),
                                                     _p(b0), _p(b1), _p(data)))
        return b0[:m.value].copy(), b1[:m.value].copy(), data[:m.value].copy()

    def cast_rays(self, pos, R, side, shape, origin, dir, tmax=None, ray_body=None, out=None):
        """Rays against the ground and one ensemble's bodies (egs_cast_rays; the rules are in eggshell_amd.h): origin,
        dir [n_rays][3] (dir is not normalised: t is in its units), tmax [n_rays] (None = +inf), ray_body [n_rays] (-1 =
        world frame; otherwise origin and dir are in that body's frame and it is not tested) or None.  Returns (hit_body
        [n_rays] int32: -2 none, -1 the ground, else the body; t [n_rays]; normal [n_rays][3]).  out = (hit_body, t,
        normal): arrays to write into."""
        pos, R, side, shape = _f64(pos), _f64(R), _f64(side), _i32(shape)
        n = pos.reshape(-1, 3).shape[0]
        origin, dir, nr, tmax, ray_body = _ray_arrays(origin, dir, tmax, ray_body)
        hit, t, normal = out if out is not None else (np.full(nr, -2, np.int32), np.zeros(nr), np.zeros((nr, 3)))
        self.check(load().egs_cast_rays(self.h, C.c_int32(n), _p(pos), _p(R), _p(side), _p(shape), C.c_int32(nr),
                                        _p(ray_body), _p(origin), _p(dir), _p(tmax), _p(hit), _p(t), _p(normal)))
        return hit, t, normal

    def match_contacts(self, old_b0, old_b1, old_pos, old_lambda, old_off, valid, new_b0, new_b1, new_pos, new_rhs,
                       new_off, radius):
        """The start of a solve from the previous contact list's lambda (egs_match_contacts): x0 [3 m_new] and the old
        index each new contact took its rows from (-1: none within the radius, x0 = 0; -2: its ensemble has no
        history, x0 = rhs)."""
        ob0, ob1, ooff, nb0, nb1, noff = map(_i32, (old_b0, old_b1, old_off, new_b0, new_b1, new_off))
        opos, olam, npos, nrhs = map(_f64, (old_pos, old_lambda, new_pos, new_rhs))
        valid = _u8(valid)
        mo, mn = ob0.shape[0], nb0.shape[0]
        if opos.size != 3 * mo or olam.size != 3 * mo or npos.size != 3 * mn or nrhs.size != 3 * mn or \
                ooff.shape[0] != valid.shape[0] + 1 or noff.shape[0] != valid.shape[0] + 1:
            raise ValueError("arrays do not match the list sizes")
        x0 = np.zeros(3 * mn); src = np.zeros(mn, np.int32)
        self.check(load().egs_match_contacts(self.h, C.c_int32(valid.shape[0]), C.c_int32(mo), _p(ob0), _p(ob1), _p(opos),
                                             _p(olam), _p(ooff), _p(valid), C.c_int32(mn), _p(nb0), _p(nb1), _p(npos),
                                             _p(nrhs), _p(noff), C.c_double(radius), _p(x0), _p(src)))
        return x0, src

    def relax_blocks_direct(self, n_bodies, body0, body1, J0, J1, err, rank_tol=0.0):
        """(J J^T) y = err by the rank-revealing LDL^T of the direct relaxation route (egs_relax_blocks_direct):
        y [3m] (0 on the rows the truncation left) and the rank."""
        body0, body1 = _i32(body0), _i32(body1)
        J0, J1, err = _f64(J0), _f64(J1), _f64(err)
        m = body0.shape[0]
        y = np.zeros(3 * m); rank = C.c_int32(0)
        self.check(load().egs_relax_blocks_direct(self.h, C.c_int32(n_bodies), C.c_int32(m), _p(body0), _p(body1), _p(J0),
                                                  _p(J1), _p(err), C.c_double(rank_tol), _p(y), C.byref(rank)))
        return y, rank.value

    def mixed_constraints_solve(self, A, b, Ceq, lo, hi, use_bounds=0, max_pivots=0, max_seconds=0.0):
        A, b, lo, hi = map(_f64, (A, b, lo, hi))
        Ceq = _u8(Ceq)
        N = b.shape[0]
        x = np.zeros(N); w = np.zeros(N); ok = C.c_int32(0); piv = C.c_int32(0)
        st = load().egs_mixed_constraints_solve_limits(self.h, C.c_int32(N), _p(A), _p(b), _p(Ceq), _p(lo), _p(hi),
                                                       C.c_int32(use_bounds), C.c_int32(max_pivots), C.c_double(max_seconds),
                                                       _p(x), _p(w), C.byref(ok), C.byref(piv))
        if st not in (OK, ERR_LCP_FAILED):
            self.check(st)
        return bool(ok.value), x, w, piv.value


    def mixed_constraints_solve_batch_packed(self, ns, A, b, C, lo, hi, use_bounds=0, max_pivots=0):
        """egs_mixed_constraints_solve_batch on packed arrays (see lcp_batch_offsets): ok [count] (bool), x, w (packed),
        pivots [count].  A failed problem shows in ok[k], not as an exception."""
        ns, A, b, c8, lo, hi = check_mixed_batch(ns, A, b, C, lo, hi)
        cnt = len(ns)
        tot = int(np.maximum(ns, 0).sum())
        x = np.zeros(tot); w = np.zeros(tot); ok = np.zeros(cnt, np.int32); piv = np.zeros(cnt, np.int32)
        self.check(load().egs_mixed_constraints_solve_batch(self.h, cnt, _p(ns), _p(A), _p(b), _p(c8), _p(lo), _p(hi), int(use_bounds),
                                                            int(max_pivots), _p(x), _p(w), _p(ok), _p(piv)))
        return ok.astype(bool), x, w, piv

    def mixed_constraints_solve_batch(self, As, bs, Cs, los, his, use_bounds=0, max_pivots=0):
        """Lcp::MixedConstraintsSolver(A, b, C, x_lo, x_hi, x, w) on `len(As)` independent problems in one call: lists ok, x,
        w, pivots -- problem k's entries are those of mixed_constraints_solve on it."""
        ns, A, b, _, _ = pack_lcp_batch(As, bs, [], [])
        Cp = pack_batch_vectors(ns, Cs, np.uint8, "C")
        lo, hi = pack_batch_vectors(ns, los, what="lo"), pack_batch_vectors(ns, his, what="hi")
        ok, x, w, piv = self.mixed_constraints_solve_batch_packed(ns, A, b, Cp, lo, hi, use_bounds, max_pivots)
        xl, wl = unpack_lcp_batch(ns, None, x, w)
        return [bool(v) for v in ok], xl, wl, [int(v) for v in piv]

    def mixed_friction_solve_batch_packed(self, ns, A, b, C, lo, hi, normal_row, mu, max_pivots=0, max_outer=32, tol=1e-10):
        """egs_mixed_friction_solve_batch on packed arrays: a dict of ok [count] (bool), x, w, beta (packed), pivots, outer
        [count], change [count] and converged = change <= tol.  A failed problem shows in ok[k], not as an exception."""
        ns, A, b, c8, lo, hi, nr, mu = check_mixed_friction_batch(ns, A, b, C, lo, hi, normal_row, mu, max_outer, tol)
        cnt = len(ns)
        tot = int(np.maximum(ns, 0).sum())
        x = np.zeros(tot); w = np.zeros(tot); beta = np.zeros(tot)
        ok = np.zeros(cnt, np.int32); piv = np.zeros(cnt, np.int32); outer = np.zeros(cnt, np.int32); change = np.zeros(cnt)
        self.check(load().egs_mixed_friction_solve_batch(self.h, cnt, _p(ns), _p(A), _p(b), _p(c8), _p(lo), _p(hi), _p(nr), _p(mu),
                                                         int(max_pivots), int(max_outer), float(tol), _p(x), _p(w), _p(beta), _p(ok),
                                                         _p(piv), _p(outer), _p(change)))
        return dict(ok=ok.astype(bool), x=x, w=w, beta=beta, pivots=piv, outer=outer, change=change, converged=change <= tol)

    def dense_iterate(self, A, b, prm, Ceq=None, lo=None, hi=None):
        """sparse::{Jacobi,GaussSeidel,SOR}Iteration(A, b[, C, x_lo, x_hi]) on an explicit matrix: x, stats."""
        A, b = _f64(A), _f64(b)
        n = b.shape[0]
        x = np.zeros(n)
        st = SolveStats()
        args = (None, None, None) if Ceq is None else (_p(_u8(Ceq)), _p(_f64(lo)), _p(_f64(hi)))
        keep = (Ceq, lo, hi)
        if Ceq is not None:
            c8, l8, h8 = _u8(Ceq), _f64(lo), _f64(hi)
            args = (_p(c8), _p(l8), _p(h8))
        self.check(load().egs_dense_iterate(self.h, C.c_int32(n), _p(A), _p(b), args[0], args[1], args[2], C.byref(prm), _p(x), C.byref(st)))
        return x, st

    def dense_iterate_batch_packed(self, ns, A, b, prm, C=None, lo=None, hi=None, history=False):
        """egs_dense_iterate_batch on packed arrays (see lcp_batch_offsets): x (packed), iterations [count], residual
        [count] and, with history=True, the residual after every sweep, [count][max_iters + 1] (NaN beyond iterations)."""
        ns, A, b, c8, lo, hi = check_dense_iterate_batch(ns, A, b, C, lo, hi)
        cnt = len(ns)
        x = np.zeros(int(np.maximum(ns, 0).sum())); it = np.zeros(cnt, np.int32); res = np.zeros(cnt)
        hist = np.zeros((cnt, max(int(prm.max_iters), 0) + 1)) if history else None
        self.check(load().egs_dense_iterate_batch(self.h, _ct.c_int32(cnt), _p(ns), _p(A), _p(b), _p(c8), _p(lo), _p(hi), _ct.byref(prm),
                                                  _p(x), _p(it), _p(res), _p(hist)))
        return (x, it, res, hist) if history else (x, it, res)

    def dense_iterate_batch(self, As, bs, prm, Cs=None, los=None, his=None, history=False):
        """sparse::{Jacobi,GaussSeidel,SOR}Iteration(A, b[, C, x_lo, x_hi]) on `len(As)` independent systems in one call:
        lists x, iterations, residual[, history] -- problem k's entries are those of dense_iterate on it."""
        given = [v is not None for v in (Cs, los, his)]
        if any(given) and not all(given):
            raise ValueError("Cs, los and his come together (or all None: every row an equality)")
        ns, A, b, _, _ = pack_lcp_batch(As, bs, [], [])
        Cp = lo = hi = None
        if all(given):
            Cp = pack_batch_vectors(ns, Cs, np.uint8, "C")
            lo, hi = pack_batch_vectors(ns, los, what="lo"), pack_batch_vectors(ns, his, what="hi")
        out = self.dense_iterate_batch_packed(ns, A, b, prm, Cp, lo, hi, history)
        xl, = unpack_lcp_batch(ns, None, out[0])
        res = (xl, [int(v) for v in out[1]], [float(v) for v in out[2]])
        return res + ([out[3][k] for k in range(len(ns))],) if history else res

    def dense_condition(self, A):
        """GetConditionNumber of a symmetric positive definite matrix (utils.cc:256-261) on the device: (estimate, pivot bound)."""
        A = _f64(A)
        est, pb = C.c_double(0), C.c_double(0)
        self.check(load().egs_dense_condition(self.h, C.c_int32(A.shape[0]), _p(A), C.byref(est), C.byref(pb)))
        return est.value, pb.value

    def box_lcp_murty(self, A, b, lo, hi, max_iterations=0):
        """lcp::SolveLCP_BoxMurty on a LinearReducer (toolkit/lcp.cc:213-328, 380-442), n <= 1024."""
        return self.box_lcp_dantzig(A, b, lo, hi, max_iterations, _entry="egs_box_lcp_murty")

    def box_lcp_dantzig(self, A, b, lo, hi, max_steps=0, _entry="egs_box_lcp_dantzig"):
        """lcp::SolveLCP_BoxDantzig with the incremental factor (toolkit/lcp.cc:444-619), n <= 1024.
        Returns ok, x, w, A permuted in place (lower triangle), perm, pivot steps."""
        A = _f64(A).copy()
        b, lo, hi = map(_f64, (b, lo, hi))
        n = b.shape[0]
        x = np.zeros(n); w = np.zeros(n); perm = np.zeros(n, np.int32); ok = C.c_int32(0); piv = C.c_int32(0)
        st = getattr(load(), _entry)(self.h, C.c_int32(n), _p(A), _p(b), _p(lo), _p(hi), C.c_int32(max_steps),
                                        _p(x), _p(w), _p(perm), C.byref(ok), C.byref(piv))
        if st not in (OK, ERR_LCP_FAILED):
            self.check(st)
        return bool(ok.value), x, w, A, perm, piv.value

    def box_lcp_batch_packed(self, algorithm, ns, A, b, lo, hi, max_steps=0, max_seconds=0.0):
        """egs_box_lcp_batch on packed arrays (problem k's matrix at sum_{j<k} n_j^2, its vectors at sum_{j<k} n_j):
        returns ok, x, w, A (permuted in place, a copy), perm, pivots -- packed the same way."""
        ns = _i32(ns)
        A = _f64(A).copy()
        b, lo, hi = map(_f64, (b, lo, hi))
        tot, cnt = int(ns.sum()), len(ns)
        x = np.zeros(tot); w = np.zeros(tot); perm = np.zeros(tot, np.int32)
        ok = np.zeros(cnt, np.int32); piv = np.zeros(cnt, np.int32)
        self.check(load().egs_box_lcp_batch(self.h, C.c_int32(algorithm), C.c_int32(cnt), _p(ns), _p(A), _p(b), _p(lo), _p(hi),
                                            C.c_int32(max_steps), C.c_double(max_seconds), _p(x), _p(w), _p(perm), _p(ok), _p(piv)))
        return ok, x, w, A, perm, piv

    def box_lcp_batch(self, algorithm, As, bs, los, his, max_steps=0, max_seconds=0.0):
        """`len(As)` independent box LCPs in one launch (egs_box_lcp_batch); algorithm 0 = BoxMurty, 1 = BoxDantzig.
        Returns lists ok, x, w, A (permuted in place), perm, pivots -- problem k's entries equal its single call's."""
        ns = np.array([len(b) for b in bs], np.int32)
        A = np.concatenate([_f64(a).reshape(-1) for a in As])
        b, lo, hi = (np.concatenate([_f64(v) for v in vs]) for vs in (bs, los, his))
        cnt = len(ns)
        ok, x, w, A, perm, piv = self.box_lcp_batch_packed(algorithm, ns, A, b, lo, hi, max_steps, max_seconds)
        vo = np.concatenate([[0], np.cumsum(ns)]); ao = np.concatenate([[0], np.cumsum(ns.astype(np.int64) ** 2)])
        return ([bool(v) for v in ok], [x[vo[k]:vo[k + 1]] for k in range(cnt)], [w[vo[k]:vo[k + 1]] for k in range(cnt)],
                [A[ao[k]:ao[k + 1]].reshape(ns[k], ns[k]) for k in range(cnt)], [perm[vo[k]:vo[k + 1]] for k in range(cnt)],
                [int(v) for v in piv])

    def box_lcp_schur(self, A, b, lo, hi, algorithm=0, nub=-1, reference_quirks=True, max_iterations=0, max_seconds=0.0):
        """lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747).  Returns ok, x, w, A permuted in place (lower triangle),
        perm of the partition, nub, inner pivots."""
        A = _f64(A).copy()
        b, lo, hi = map(_f64, (b, lo, hi))
        n = b.shape[0]
        x = np.zeros(n); w = np.zeros(n); perm = np.zeros(n, np.int32)
        ok = C.c_int32(0); piv = C.c_int32(0); nub_out = C.c_int32(0)
        st = load().egs_box_lcp_schur(self.h, C.c_int32(n), _p(A), _p(b), _p(lo), _p(hi), C.c_int32(algorithm), C.c_int32(nub),
                                      C.c_int32(1 if reference_quirks else 0), C.c_int32(max_iterations), C.c_double(max_seconds),
                                      _p(x), _p(w), _p(perm), C.byref(ok), C.byref(nub_out), C.byref(piv))
        if st not in (OK, ERR_LCP_FAILED):
            self.check(st)
        return bool(ok.value), x, w, A, perm, nub_out.value, piv.value


    def box_lcp_schur_batch_packed(self, ns, A, b, lo, hi, algorithm=0, nubs=None, reference_quirks=True, max_iterations=0,
                                   max_seconds=0.0):
        """egs_box_lcp_schur_batch on packed arrays (see lcp_batch_offsets): returns ok, x, w, A (permuted in place, a
        copy), perm of the partitions, nub, inner pivots -- packed the same way."""
        ns = _i32(ns)
        A = _f64(A).copy()
        b, lo, hi = map(_f64, (b, lo, hi))
        nubs = _i32(nubs)
        tot, cnt = int(ns.sum()), len(ns)
        if A.size != int((ns.astype(np.int64) ** 2).sum()) or any(v.size != tot for v in (b, lo, hi)) or (nubs is not None and nubs.size != cnt):
            raise ValueError("packed arrays do not match the sizes")
        x = np.zeros(tot); w = np.zeros(tot); perm = np.zeros(tot, np.int32)
        ok = np.zeros(cnt, np.int32); nub_out = np.zeros(cnt, np.int32); piv = np.zeros(cnt, np.int32)
        self.check(load().egs_box_lcp_schur_batch(self.h, C.c_int32(algorithm), C.c_int32(cnt), _p(ns), _p(A), _p(b), _p(lo), _p(hi),
                                                  _p(nubs), C.c_int32(1 if reference_quirks else 0), C.c_int32(max_iterations),
                                                  C.c_double(max_seconds), _p(x), _p(w), _p(perm), _p(ok), _p(nub_out), _p(piv)))
        return ok, x, w, A, perm, nub_out, piv

    def box_lcp_schur_batch(self, As, bs, los, his, algorithm=0, nubs=None, reference_quirks=True, max_iterations=0, max_seconds=0.0):
        """lcp::SolveLCP under its default Settings (SolveLCP_BoxSchur) on `len(As)` independent problems in one call:
        those of n <= 96 rows in one fused launch, larger ones one after another.  Returns lists ok, x, w, A (permuted in
        place), perm, nub, pivots -- problem k's entries are those of box_lcp_schur on it."""
        ns, A, b, lo, hi = pack_lcp_batch(As, bs, los, his)
        ok, x, w, A, perm, nub, piv = self.box_lcp_schur_batch_packed(ns, A, b, lo, hi, algorithm, nubs, reference_quirks,
                                                                      max_iterations, max_seconds)
        Al, xl, wl, pl = unpack_lcp_batch(ns, A, x, w, perm)
        return [bool(v) for v in ok], xl, wl, Al, pl, [int(v) for v in nub], [int(v) for v in piv]


class Problem:
    """Device-resident ensemble (or batch of ensembles)."""

    def __init__(self, ctx, n_bodies, body0, body1, precision=F64):
        self.ctx = ctx
        self.body0, self.body1 = _i32(body0), _i32(body1)
        self.n, self.m = int(n_bodies), int(self.body0.shape[0])
        self.h = C.c_void_p()
        ctx.check(load().egs_problem_create(ctx.h, C.c_int32(self.n), C.c_int32(self.m), _p(self.body0),
                                            _p(self.body1), C.c_int32(precision), C.byref(self.h)))
        ctx._children.add(self)

    def set_mass(self, inv_mass, inv_inertia):
        """Compact M^-1: 1/m [n] and the inverse global-frame inertia [n][9]."""
        self.ctx.check(load().egs_problem_set_mass(self.h, _p(_f64(inv_mass)), _p(_f64(inv_inertia))))

    @classmethod
    def batch(cls, ctx, n_bodies, n_constraints, body0, body1, precision=F64):
        """E independent ensembles in one problem (egs_problem_create_batch): per-ensemble
        sizes and ensemble-LOCAL body indices; returns (problem, body_offset, constraint_offset)."""
        nb, nc = _i32(n_bodies), _i32(n_constraints)
        self = cls.__new__(cls)
        self.ctx = ctx
        self.body0, self.body1 = _i32(body0), _i32(body1)     # local indices, as passed
        self.n, self.m = int(nb.sum()), int(nc.sum())
        boff = np.zeros(nb.shape[0] + 1, np.int32); coff = np.zeros(nb.shape[0] + 1, np.int32)
        self.h = C.c_void_p()
        ctx.check(load().egs_problem_create_batch(ctx.h, C.c_int32(nb.shape[0]), _p(nb), _p(nc), _p(self.body0),
                                                  _p(self.body1), C.c_int32(precision), C.byref(self.h),
                                                  _p(boff), _p(coff)))
        ctx._children.add(self)
        return self, boff, coff

    def close(self):
        if self.h:
            load().egs_problem_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_blocks(self, Minv=None, J0=None, J1=None, is_eq=None, lo=None, hi=None, rhs=None):
        a = [_f64(Minv), _f64(J0), _f64(J1), _u8(is_eq), _f64(lo), _f64(hi), _f64(rhs)]
        self.ctx.check(load().egs_problem_set_blocks(self.h, *[_p(v) for v in a]))

    def set_state(self, pos=None, R=None, v=None, w=None, Minv=None, f_ext=None):
        a = [_f64(pos), _f64(R), _f64(v), _f64(w), _f64(Minv), _f64(f_ext)]
        self.ctx.check(load().egs_problem_set_state(self.h, *[_p(v_) for v_ in a]))

    def set_live_inertia(self, inertia_body=None, torque=None):
        """Live inertia (egs_problem_set_live_inertia): body-frame inertias [n][3][3] and an optional applied torque
        [n][3]; every stepping entry then recomputes M^-1 and the gyroscopic torque of the bodies whose inertia is not
        a multiple of the identity from the R and w the device holds.  None turns it off."""
        self.ctx.check(load().egs_problem_set_live_inertia(self.h, *_live_arrays(self.n, inertia_body, torque)))

    def mass(self):
        """Minv [n][36] and f_ext [n][6] as the device holds them (egs_problem_get_mass)."""
        Minv = np.zeros((self.n, 36)); f_ext = np.zeros((self.n, 6))
        self.ctx.check(load().egs_problem_get_mass(self.h, _p(Minv), _p(f_ext)))
        return Minv, f_ext

    def set_constraints(self, kind, data):
        kind, data = _i32(kind), _f64(data)
        self.ctx.check(load().egs_problem_set_constraints(self.h, _p(kind), _p(data)))

    def assemble(self, dt, erp=0.2):
        self.ctx.check(load().egs_problem_assemble(self.h, C.c_double(dt), C.c_double(erp)))

    def solve(self, prm, want_stats=True):
        st = SolveStats()
        self.ctx.check(load().egs_problem_solve(self.h, C.byref(prm), C.byref(st) if want_stats else None))
        return st

    def step(self, dt, erp, prm, want_stats=False):
        st = SolveStats()
        self.ctx.check(load().egs_problem_step(self.h, C.c_double(dt), C.c_double(erp), C.byref(prm),
                                               C.byref(st) if want_stats else None))
        return st

    def stats(self):
        st = SolveStats()
        self.ctx.check(load().egs_problem_get_stats(self.h, C.byref(st)))
        return st

    def schedule(self):
        """The schedule bits of the last solve, SCHED_CHAIN among them (see egs_problem_get_schedule)."""
        out = C.c_int32(0)
        self.ctx.check(load().egs_problem_get_schedule(self.h, C.byref(out)))
        return int(out.value)

    def schedule_full(self):
        """... and SCHED_SHARE with them (see egs_problem_get_schedule_full)."""
        out = C.c_int32(0)
        self.ctx.check(load().egs_problem_get_schedule_full(self.h, C.byref(out)))
        return int(out.value)

    def schedule_forms(self):
        """... and SCHED_FACE with them (see egs_problem_get_schedule_forms)."""
        out = C.c_int32(0)
        self.ctx.check(load().egs_problem_get_schedule_forms(self.h, C.byref(out)))
        return int(out.value)

    def lambda_(self):
        x = np.zeros(3 * self.m)
        self.ctx.check(load().egs_problem_get_lambda(self.h, _p(x)))
        return x

    def debug_trace(self, max_sweeps=1000):
        """EGS_TRACE_UPDATES=1: completion stamps [sweeps][m] (100 MHz ticks) of the last 4-lane patch launch."""
        buf = np.zeros(max_sweeps * self.m, np.uint64)
        sw = C.c_int32(0)
        self.ctx.check(load().egs_problem_debug_trace(self.h, _p(buf), C.c_int64(buf.shape[0]), C.byref(sw)))
        return buf[:sw.value * self.m].reshape(sw.value, self.m)

    def set_start(self, mode, x0=None):
        """Where the following solves start (egs_problem_set_start): START_RHS (the reference, the default),
        START_GIVEN with the 3m rows of x0, START_PREVIOUS (the last solve's lambda).  Sticky until changed."""
        x0 = _f64(x0)
        if x0 is not None and x0.size != 3 * self.m:
            raise ValueError("x0: %d rows for %d constraints" % (x0.size, self.m))
        self.ctx.check(load().egs_problem_set_start(self.h, C.c_int32(mode), _p(x0)))

    def set_friction(self, mu=None):
        """The Coulomb pyramid (egs_problem_set_friction): one coefficient per constraint, >= 0: the tangential rows are
        bounded by +-mu x_n, < 0: the stored bounds.  None, or no coefficient >= 0, turns friction off."""
        mu = _f64(mu)
        if mu is not None and mu.size != self.m:
            raise ValueError("mu: %d coefficients for %d constraints" % (mu.size, self.m))
        self.ctx.check(load().egs_problem_set_friction(self.h, _p(mu)))

    def set_restitution(self, rest=None, vth=0.0):
        """Restitution (egs_problem_set_restitution): one coefficient per constraint, >= 0: a contact approaching faster
        than vth bounces with it, < 0: assembled as stored.  None, or no coefficient >= 0, turns it off."""
        rest = _f64(rest)
        if rest is not None and rest.size != self.m:
            raise ValueError("rest: %d coefficients for %d constraints" % (rest.size, self.m))
        self.ctx.check(load().egs_problem_set_restitution(self.h, _p(rest), float(vth)))

    def set_motors(self, motor=None):
        """Hinge motors (egs_problem_set_motors): [m][2] = (speed, tau) per constraint; a HINGE_AXIS constraint with
        tau >= 0 is driven towards speed within +-tau, everything else is assembled as stored.  None turns it off."""
        motor = _f64(motor)
        if motor is not None and motor.size != 2 * self.m:
            raise ValueError("motor: %d values for %d constraints" % (motor.size, self.m))
        self.ctx.check(load().egs_problem_set_motors(self.h, _p(motor)))

    def set_hinge_limits(self, lim=None):
        """Hinge angle limits (egs_problem_set_hinge_limits): [m][8] = (qw, qx, qy, qz, sin lo, cos lo, sin hi, cos hi)
        per constraint, q the quaternion of R0(0)^T R1(0); a (sin, cos) pair of (0, 0): no stop on that side.  A
        HINGE_AXIS constraint past a stop gets the one-sided axis row of that stop.  None turns it off."""
        lim = _f64(lim)
        if lim is not None and lim.size != 8 * self.m:
            raise ValueError("lim: %d values for %d constraints" % (lim.size, self.m))
        self.ctx.check(load().egs_problem_set_hinge_limits(self.h, _p(lim)))

    def set_slider_limits(self, lim=None):
        """Slider travel stops (egs_problem_set_slider_limits): [m][2] = (xlo, xhi) per constraint, -inf / +inf: no stop
        on that side.  A SLIDER_AXIS constraint past a stop gets the one-sided rail row of that stop.  None turns it off."""
        lim = _f64(lim)
        if lim is not None and lim.size != 2 * self.m:
            raise ValueError("lim: %d values for %d constraints" % (lim.size, self.m))
        self.ctx.check(load().egs_problem_set_slider_limits(self.h, _p(lim)))

    def wres(self):
        """w = A lambda - rhs of the last solve (the solve kernels' epilogue)."""
        w = np.zeros(3 * self.m)
        self.ctx.check(load().egs_problem_get_wres(self.h, _p(w)))
        return w

    def matvec(self, x=None, parts=MV_FULL, eps=0.0, scale=1.0, fetch=True):
        """y = part(J M^-1 J^T) x (egs_problem_matvec).  x=None: the device-resident lambda;
        fetch=False leaves y on the device (asynchronous; matvec_result() reads it)."""
        xx = _f64(x) if x is not None else None
        y = np.zeros(3 * self.m) if fetch else None
        self.ctx.check(load().egs_problem_matvec(self.h, C.c_int32(parts), C.c_double(eps), C.c_double(scale),
                                                 _p(xx), _p(y)))
        return y

    def matvec_result(self):
        y = np.zeros(3 * self.m)
        self.ctx.check(load().egs_problem_get_matvec(self.h, _p(y)))
        return y

    def dense_system(self, cfm=0.0):
        """A = J M^-1 J^T + cfm I (ensembles.cc:510, 513-521), built on the device."""
        A = np.zeros((3 * self.m, 3 * self.m))
        self.ctx.check(load().egs_problem_dense_system(self.h, C.c_double(cfm), _p(A)))
        return A

    def dense_condition(self, cfm=0.0):
        est = C.c_double(0)
        self.ctx.check(load().egs_problem_dense_condition(self.h, C.c_double(cfm), C.byref(est)))
        return est.value

    def set_dense_friction(self, max_outer=32, tol=1e-10):
        """egs_problem_set_dense_friction: max_outer > 0 lets step_dense solve the friction pyramid (0: it refuses)."""
        self.ctx.check(load().egs_problem_set_dense_friction(self.h, int(max_outer), float(tol)))

    def dense_friction_info(self):
        """(outer, converged, change) of the last step_dense that solved the pyramid."""
        outer, conv, change = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        self.ctx.check(load().egs_problem_dense_friction_info(self.h, C.byref(outer), C.byref(conv), C.byref(change)))
        return outer.value, bool(conv.value), change.value

    def step_dense(self, dt, erp=0.2, cfm=0.0, use_bounds=0):
        """StepVelocities_ODE through the dense path: returns (ok, pivots)."""
        ok = C.c_int32(0); piv = C.c_int32(0)
        st = load().egs_problem_step_dense(self.h, C.c_double(dt), C.c_double(erp), C.c_double(cfm), C.c_int32(use_bounds),
                                           C.byref(ok), C.byref(piv))
        if st not in (OK, ERR_LCP_FAILED):
            self.ctx.check(st)
        return bool(ok.value), piv.value

    def accumulators(self):
        a = np.zeros((self.n, 6))
        self.ctx.check(load().egs_problem_get_accumulators(self.h, _p(a)))
        return a

    def velocity(self):
        v = np.zeros((self.n, 6))
        self.ctx.check(load().egs_problem_get_velocity(self.h, _p(v)))
        return v

    def advance(self, dt):
        self.ctx.check(load().egs_problem_advance(self.h, C.c_double(dt)))

    def state(self):
        pos = np.zeros((self.n, 3)); R = np.zeros((self.n, 9)); v = np.zeros((self.n, 3)); w = np.zeros((self.n, 3))
        self.ctx.check(load().egs_problem_get_state(self.h, _p(pos), _p(R), _p(v), _p(w)))
        return pos, R, v, w

    def blocks(self):
        m = self.m
        J0 = np.zeros((m, 18)); J1 = np.zeros((m, 18)); is_eq = np.zeros(3 * m, np.uint8)
        lo = np.zeros(3 * m); hi = np.zeros(3 * m); rhs = np.zeros(3 * m); err = np.zeros(3 * m)
        self.ctx.check(load().egs_problem_get_blocks(self.h, _p(J0), _p(J1), _p(is_eq), _p(lo), _p(hi),
                                                     _p(rhs), _p(err)))
        return J0, J1, is_eq, lo, hi, rhs, err


def debug_plan(n_bodies, body0, body1, tile_size=256):
    """Host-only view of the schedule (islands, tiles, tickets); needs no GPU."""
    body0, body1 = _i32(body0), _i32(body1)
    m = body0.shape[0]
    ni, nt, ng = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    out = [np.zeros(m, np.int32) for _ in range(5)]
    st = load().egs_debug_plan(C.c_int32(n_bodies), C.c_int32(m), _p(body0), _p(body1), C.c_int32(tile_size),
                               C.byref(ni), C.byref(nt), C.byref(ng), *[_p(o) for o in out])
    if st != OK:
        raise EgsError(st, "egs_debug_plan failed")
    return dict(n_islands=ni.value, n_tiles=nt.value, n_global=ng.value, cons_tile=out[0],
                pos0=out[1], cnt0=out[2], pos1=out[3], cnt1=out[4])


def debug_choose_oversize_schedule(n_patch_tiles, quad_per_cu, patch_per_cu, cu_count=256, patches=True, quad_patches=True):
    """0 = 4-lane patches, 1 = 1-lane patches, 2 = all-global kernel (host only)."""
    return int(load().egs_debug_choose_oversize_schedule(C.c_int32(n_patch_tiles), C.c_int32(quad_per_cu),
                                                         C.c_int32(patch_per_cu), C.c_int32(cu_count),
                                                         C.c_int32(1 if patches else 0), C.c_int32(1 if quad_patches else 0)))


def debug_matvec_plan(n_bodies, body0, body1, tile_size=256):
    """Host-only view of the mat-vec schedule (tiles, shared bodies, boundary list); needs no GPU."""
    body0, body1 = _i32(body0), _i32(body1)
    m = body0.shape[0]
    vals = [C.c_int32(0) for _ in range(4)]
    ct = np.full(m, -1, np.int32); cl = np.full(m, -1, np.int32)
    st = load().egs_debug_matvec_plan(C.c_int32(n_bodies), C.c_int32(m), _p(body0), _p(body1), C.c_int32(tile_size),
                                      *[C.byref(v) for v in vals], _p(ct), _p(cl))
    if st != OK:
        raise EgsError(st, "egs_debug_matvec_plan failed")
    return dict(n_tiles=vals[0].value, n_islands=vals[1].value, n_shared_bodies=vals[2].value,
                n_boundary=vals[3].value, cons_tile=ct, cons_lane=cl)


def debug_plan_slots(n_bodies, body0, body1, tile_size=256):
    """Host-only: per constraint its lane in the tile, the LDS slots of its two sides and
    the slot count of its tile (see egs_debug_plan_slots)."""
    body0, body1 = _i32(body0), _i32(body1)
    m = body0.shape[0]
    out = [np.zeros(m, np.int32) for _ in range(4)]
    st = load().egs_debug_plan_slots(C.c_int32(n_bodies), C.c_int32(m), _p(body0), _p(body1), C.c_int32(tile_size),
                                     *[_p(o) for o in out])
    if st != OK:
        raise EgsError(st, "egs_debug_plan_slots failed")
    return dict(lane=out[0], slot0=out[1], slot1=out[2], tile_nslots=out[3])


def debug_plan_timetable(n_bodies, body0, body1, tile_size=256):
    """Host-only: per constraint its level in the list-order dependency DAG and the period / depth of
    its tile's static timetable (see egs_debug_plan_timetable)."""
    body0, body1 = _i32(body0), _i32(body1)
    m = body0.shape[0]
    out = [np.zeros(m, np.int32) for _ in range(3)]
    runs = C.c_int32(0)
    st = load().egs_debug_plan_timetable(C.c_int32(n_bodies), C.c_int32(m), _p(body0), _p(body1), C.c_int32(tile_size),
                                         *[_p(o) for o in out], C.byref(runs))
    if st != OK:
        raise EgsError(st, "egs_debug_plan_timetable failed")
    return dict(level=out[0], period=out[1], depth=out[2], runs=bool(runs.value))


def debug_plan_pairable(n_bodies, body0, body1):
    """Host-only: does the 256-lane tile plan keep one timetable phase per half-wavefront (see egs_debug_plan_pairable)?"""
    body0, body1 = _i32(body0), _i32(body1)
    out = C.c_int32(0)
    st = load().egs_debug_plan_pairable(C.c_int32(n_bodies), C.c_int32(body0.shape[0]), _p(body0), _p(body1), C.byref(out))
    if st != OK:
        raise EgsError(st, "egs_debug_plan_pairable failed")
    return bool(out.value)


def debug_plan_chained(n_bodies, body0, body1):
    """Host-only: do the thread pairs of the lane-pair form hold consecutive updates of the same two bodies (see
    egs_debug_plan_chained)?"""
    body0, body1 = _i32(body0), _i32(body1)
    out = C.c_int32(0)
    st = load().egs_debug_plan_chained(C.c_int32(n_bodies), C.c_int32(body0.shape[0]), _p(body0), _p(body1), C.byref(out))
    if st != OK:
        raise EgsError(st, "egs_debug_plan_chained failed")
    return bool(out.value)


def debug_plan_share(n_bodies, body0, body1, data):
    """Host-only: is the plan chained, and do the two contacts of every thread pair carry the same normal bit for bit
    (see egs_debug_plan_share)?  data: the constraint descriptors [m][7]."""
    body0, body1 = _i32(body0), _i32(body1)
    data = np.ascontiguousarray(data, dtype=np.float64).reshape(body0.shape[0], 7)
    out = C.c_int32(0)
    st = load().egs_debug_plan_share(C.c_int32(n_bodies), C.c_int32(body0.shape[0]), _p(body0), _p(body1), _p(data),
                                     C.byref(out))
    if st != OK:
        raise EgsError(st, "egs_debug_plan_share failed")
    return bool(out.value)


def debug_plan_faced(n_bodies, body0, body1):
    """Host-only: do the thread pairs of the face form hold four consecutive updates of the same two bodies, alone on
    those bodies within a block of four time steps (see egs_debug_plan_faced)?"""
    body0, body1 = _i32(body0), _i32(body1)
    out = C.c_int32(0)
    st = load().egs_debug_plan_faced(C.c_int32(n_bodies), C.c_int32(body0.shape[0]), _p(body0), _p(body1), C.byref(out))
    if st != OK:
        raise EgsError(st, "egs_debug_plan_faced failed")
    return bool(out.value)


def debug_face_split(n_tiles, slots, depth, period, sweeps, force=None):
    """Host-only: the split of the FACE launch in time (see egs_debug_face_split) for n_tiles tiles on `slots` resident
    slots.  force: None, the policy decides; (h, s1), the last h tiles after s1 sweeps.  Returns (split tiles, s1, pieces):
    pieces int32 [n][4] in ticket order, per piece tile, resume, sweeps, kind (0 whole, 1 first part, 2 second part)."""
    h, s1 = (-1, 0) if force is None else force
    tiles, cut, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    pieces = np.zeros((2 * max(int(n_tiles), 0) + 1, 4), dtype=np.int32)
    st = load().egs_debug_face_split(C.c_int32(n_tiles), C.c_int32(slots), C.c_int32(depth), C.c_int32(period),
                                     C.c_int32(sweeps), C.c_int32(h), C.c_int32(s1), C.byref(tiles), C.byref(cut),
                                     _p(pieces), C.byref(n))
    if st != OK:
        raise EgsError(st, "egs_debug_face_split failed")
    return tiles.value, cut.value, pieces[:n.value].copy()


def debug_face_form(n_tiles, cus, depth, period, sweeps, max_slots=0):
    """Host-only: the form of the FACE launch (see egs_debug_face_form) for n_tiles tiles on `cus` CUs.  Returns a dict:
    lean (bool), us (the predicted launch of the present and of the lean form, microseconds), split (per form: split
    tiles, s1) and lds_bytes (a lean tile's LDS request at six tiles per CU for max_slots body slots; 0: it does not fit,
    or max_slots was not given)."""
    lean, lds = C.c_int32(0), C.c_int64(0)
    us, split = np.zeros(2, dtype=np.float64), np.zeros((2, 2), dtype=np.int32)
    lib = load()
    lib.egs_debug_face_form.argtypes = [C.c_int32] * 6 + [C.c_void_p] * 4
    st = lib.egs_debug_face_form(n_tiles, cus, depth, period, sweeps, max_slots, C.addressof(lean), us.ctypes.data,
                                 split.ctypes.data, C.addressof(lds))
    if st != OK:
        raise EgsError(st, "egs_debug_face_form failed")
    return {"lean": bool(lean.value), "us": (float(us[0]), float(us[1])),
            "split": (tuple(int(v) for v in split[0]), tuple(int(v) for v in split[1])), "lds_bytes": int(lds.value)}


def debug_plan_face_normals(n_bodies, body0, body1, data):
    """Host-only: is the plan faced, and do the contacts of every group of four carry one normal bit for bit (see
    egs_debug_plan_face_normals)?  data: the constraint descriptors [m][7]."""
    body0, body1 = _i32(body0), _i32(body1)
    data = np.ascontiguousarray(data, dtype=np.float64).reshape(body0.shape[0], 7)
    out = C.c_int32(0)
    st = load().egs_debug_plan_face_normals(C.c_int32(n_bodies), C.c_int32(body0.shape[0]), _p(body0), _p(body1), _p(data),
                                            C.byref(out))
    if st != OK:
        raise EgsError(st, "egs_debug_plan_face_normals failed")
    return bool(out.value)


class World:
    """Ensemble::Step resident on the device (collide -> solve -> integrate)."""

    def __init__(self, ctx, n_bodies, precision=F64, _handle=None):
        self.ctx, self.n = ctx, int(n_bodies)
        self.n_ensembles = 1
        if _handle is None:
            self.h = C.c_void_p()
            ctx.check(load().egs_world_create(ctx.h, C.c_int32(self.n), C.c_int32(precision), C.byref(self.h)))
        else:
            self.h = _handle
        ctx._children.add(self)

    @classmethod
    def batch(cls, ctx, n_bodies, precision=F64):
        """E independent ensembles in one world (egs_world_create_batch): n_bodies [E].
        Returns (world, body_offset [E+1]); body arrays are the ensembles' concatenated."""
        nb = _i32(n_bodies)
        off = np.zeros(nb.shape[0] + 1, np.int32)
        h = C.c_void_p()
        ctx.check(load().egs_world_create_batch(ctx.h, C.c_int32(nb.shape[0]), _p(nb), C.c_int32(precision),
                                                C.byref(h), _p(off)))
        w = cls(ctx, int(off[-1]), precision, _handle=h)
        w.n_ensembles = int(nb.shape[0])
        return w, off

    def batch_info(self):
        """Per-ensemble figures: joint_offset / contact_offset [E+1], iterations / residual [E] of the last solve."""
        E = self.n_ensembles
        jo = np.zeros(E + 1, np.int32); co = np.zeros(E + 1, np.int32)
        it = np.zeros(E, np.int32); res = np.zeros(E)
        self.ctx.check(load().egs_world_batch_info(self.h, C.c_int32(E), _p(jo), _p(co), _p(it), _p(res)))
        return dict(joint_offset=jo, contact_offset=co, iterations=it, residual=res)

    def close(self):
        if self.h:
            load().egs_world_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_bodies(self, pos, R, v, w, Minv, f_ext, side=None):
        side = _f64(np.tile([0.3, 0.3, 0.3], (self.n, 1)) if side is None else side)
        a = [_f64(pos), _f64(R), _f64(v), _f64(w), _f64(Minv), _f64(f_ext), side]
        self.ctx.check(load().egs_world_set_bodies(self.h, *[_p(x) for x in a]))

    def set_live_inertia(self, inertia_body=None, torque=None):
        """Live inertia (egs_world_set_live_inertia): as Problem.set_live_inertia, global body indices in a batched
        world.  None turns it off."""
        self.ctx.check(load().egs_world_set_live_inertia(self.h, *_live_arrays(self.n, inertia_body, torque)))

    def mass(self):
        """Minv [n][36] and f_ext [n][6] as the device holds them (egs_world_get_mass)."""
        Minv = np.zeros((self.n, 36)); f_ext = np.zeros((self.n, 6))
        self.ctx.check(load().egs_world_get_mass(self.h, _p(Minv), _p(f_ext)))
        return Minv, f_ext

    def set_shapes(self, shape):
        """A shape per body, SHAPE_BOX / SHAPE_SPHERE / SHAPE_CAPSULE [n] (egs_world_set_shapes); None switches back to
        boxes.  A sphere's side row is (d, d, d), a capsule's (d, d, l) with l > d (diameter, tip-to-tip length; the axis
        is column 2 of R); the inertia is the caller's Minv."""
        shape = _i32(shape)
        if shape is not None and shape.shape != (self.n,):
            raise ValueError("shape has shape %s: the world has %d bodies" % (shape.shape, self.n))
        self.ctx.check(load().egs_world_set_shapes(self.h, _p(shape)))

    def set_rays(self, origin, dir, tmax=None, ray_body=None, ray_ens=None):
        """The world's ray table (egs_world_set_rays), kept on the device until the next call: arrays as
        Context.cast_rays takes them, ray_body in global body indices, ray_ens [n_rays] non-decreasing in a batched
        world.  No rays (an empty origin) drops the table."""
        origin, dir, nr, tmax, ray_body = _ray_arrays(origin, dir, tmax, ray_body)
        ray_ens = _i32(ray_ens)
        if ray_ens is not None and ray_ens.shape != (nr,):
            raise ValueError("ray_ens has shape %s for %d rays" % (ray_ens.shape, nr))
        self.ctx.check(load().egs_world_set_rays(self.h, C.c_int32(nr), _p(ray_ens), _p(ray_body), _p(origin), _p(dir),
                                                 _p(tmax)))
        self.n_rays = nr

    def cast_rays(self, out=None):
        """The table's rays against the state the device holds now (egs_world_cast_rays): (hit_body, t, normal) as
        Context.cast_rays returns them, hit_body in global body indices."""
        nr = getattr(self, "n_rays", 0)
        hit, t, normal = out if out is not None else (np.full(nr, -2, np.int32), np.zeros(nr), np.zeros((nr, 3)))
        got = C.c_int32(0)
        self.ctx.check(load().egs_world_cast_rays(self.h, C.c_int32(hit.shape[0]), C.byref(got), _p(hit), _p(t), _p(normal)))
        return hit, t, normal

    def set_joints(self, body0, body1, data):
        body0, body1, data = _i32(body0), _i32(body1), _f64(data)
        self.m_joints = int(body0.shape[0])
        self.ctx.check(load().egs_world_set_joints(self.h, C.c_int32(body0.shape[0]), _p(body0), _p(body1), _p(data)))

    def set_joints_kinds(self, kind, body0, body1, data):
        """Joints of any kind (egs_world_set_joints_kinds): JOINT_BALL, JOINT_LOCK, JOINT_HINGE_AXIS, JOINT_SLIDER_AXIS; kind None: all ball."""
        kind, body0, body1, data = _i32(kind), _i32(body0), _i32(body1), _f64(data)
        if kind is not None and kind.shape[0] != body0.shape[0]:
            raise ValueError("kind: %d entries for %d joints" % (kind.shape[0], body0.shape[0]))
        self.m_joints = int(body0.shape[0])
        self.ctx.check(load().egs_world_set_joints_kinds(self.h, C.c_int32(body0.shape[0]), _p(kind), _p(body0), _p(body1), _p(data)))

    def blocks(self):
        """(J0, J1, is_eq, lo, hi, rhs, err) of the list the last step assembled (egs_world_get_blocks), joints first."""
        m = self.info()["n_constraints"]
        J0 = np.zeros((m, 18)); J1 = np.zeros((m, 18)); is_eq = np.zeros(3 * m, np.uint8)
        lo = np.zeros(3 * m); hi = np.zeros(3 * m); rhs = np.zeros(3 * m); err = np.zeros(3 * m)
        self.ctx.check(load().egs_world_get_blocks(self.h, _p(J0), _p(J1), _p(is_eq), _p(lo), _p(hi), _p(rhs), _p(err)))
        return J0, J1, is_eq, lo, hi, rhs, err

    def set_joint_motors(self, motor=None):
        """Hinge motors of the world's joints (egs_world_set_joint_motors): [m_joints][2] = (speed, tau); None: off."""
        motor = _f64(motor)
        self.ctx.check(load().egs_world_set_joint_motors(self.h, _p(motor)))

    def set_joint_limits(self, lim=None):
        """Hinge limits of the world's joints (egs_world_set_joint_limits): [m_joints][8] as Problem.set_hinge_limits;
        None: off."""
        lim = _f64(lim)
        mj = getattr(self, "m_joints", None)
        if lim is not None and mj is not None and lim.size != 8 * mj:
            raise ValueError("lim: %d values for %d joints" % (lim.size, mj))
        self.ctx.check(load().egs_world_set_joint_limits(self.h, _p(lim)))

    def set_slider_limits(self, lim=None):
        """Travel stops of the world's sliders (egs_world_set_slider_limits): [m_joints][2] as
        Problem.set_slider_limits; None: off."""
        lim = _f64(lim)
        mj = getattr(self, "m_joints", None)
        if lim is not None and mj is not None and lim.size != 2 * mj:
            raise ValueError("lim: %d values for %d joints" % (lim.size, mj))
        self.ctx.check(load().egs_world_set_slider_limits(self.h, _p(lim)))

    def step(self, dt, erp, prm, detect_contacts=True, want_stats=False):
        st = SolveStats()
        self.ctx.check(load().egs_world_step(self.h, C.c_double(dt), C.c_double(erp), C.byref(prm),
                                             C.c_int32(1 if detect_contacts else 0),
                                             C.byref(st) if want_stats else None))
        return st

    def step_dense(self, dt, erp=0.2, cfm=0.01, use_bounds=0, detect_contacts=True):
        """Ensemble::Step through the reference's dense path for every ensemble (egs_world_step_dense): cfm is
        kCfmCoeff, added where cond(J M^-1 J^T) >= 1e7.  Returns how many ensembles failed to solve (then no body
        moved; dense_info() tells which); any other error raises."""
        nf = C.c_int32(0)
        st = load().egs_world_step_dense(self.h, C.c_double(dt), C.c_double(erp), C.c_double(cfm), C.c_int32(use_bounds),
                                         C.c_int32(1 if detect_contacts else 0), C.byref(nf))
        if st not in (OK, ERR_LCP_FAILED):
            self.ctx.check(st)
        return nf.value

    def _rates(self, dt, erp):
        """dt [E] and erp (a scalar broadcasts) as two fp64 arrays of the world's length; ValueError otherwise."""
        E = self.n_ensembles
        dt = np.ascontiguousarray(np.atleast_1d(np.asarray(dt, np.float64)))
        erp = np.asarray(erp, np.float64)
        erp = np.ascontiguousarray(np.full(E, float(erp)) if erp.ndim == 0 else erp)
        for name, a in (("dt", dt), ("erp", erp)):
            if a.shape != (E,):
                raise ValueError("%s has shape %s: the world has %d ensemble(s)" % (name, a.shape, E))
        return dt, erp

    def step_each(self, dt, erp, prm, detect_contacts=True, want_stats=False):
        """step() with ensemble e stepped by dt[e] with erp[e] (egs_world_step_each): array-likes of length E, a scalar
        erp broadcasts; dt[e] = 0 lets ensemble e sit the step out."""
        dt, erp = self._rates(dt, erp)
        st = SolveStats()
        self.ctx.check(load().egs_world_step_each(self.h, C.c_int32(self.n_ensembles), _p(dt), _p(erp), C.byref(prm),
                                                  C.c_int32(1 if detect_contacts else 0),
                                                  C.byref(st) if want_stats else None))
        return st

    def step_dense_each(self, dt, erp, cfm=0.01, use_bounds=0, detect_contacts=True):
        """step_dense() with ensemble e stepped by dt[e] with erp[e] (egs_world_step_dense_each); returns how many
        ensembles failed to solve, as step_dense() does."""
        dt, erp = self._rates(dt, erp)
        nf = C.c_int32(0)
        st = load().egs_world_step_dense_each(self.h, C.c_int32(self.n_ensembles), _p(dt), _p(erp), C.c_double(cfm),
                                              C.c_int32(use_bounds), C.c_int32(1 if detect_contacts else 0), C.byref(nf))
        if st not in (OK, ERR_LCP_FAILED):
            self.ctx.check(st)
        return nf.value

    def set_dense_friction(self, max_outer=32, tol=1e-10):
        """egs_world_set_dense_friction: max_outer > 0 lets the dense steps solve the friction pyramid (0: they refuse)."""
        self.ctx.check(load().egs_world_set_dense_friction(self.h, int(max_outer), float(tol)))

    def dense_friction_info(self):
        """Per-ensemble outcomes of the pyramid in the last dense step: outer, converged (bool), change [E]."""
        E = self.n_ensembles
        outer = np.zeros(E, np.int32); conv = np.zeros(E, np.int32); change = np.zeros(E)
        self.ctx.check(load().egs_world_dense_friction_info(self.h, C.c_int32(E), _p(outer), _p(conv), _p(change)))
        return outer, conv.astype(bool), change

    def dense_info(self):
        """Per-ensemble figures of the last step_dense: condition estimate, cfm added, pivots, ok [E]."""
        E = self.n_ensembles
        cond = np.zeros(E); cfm = np.zeros(E); piv = np.zeros(E, np.int32); ok = np.zeros(E, np.int32)
        self.ctx.check(load().egs_world_dense_info(self.h, C.c_int32(E), _p(cond), _p(cfm), _p(piv), _p(ok)))
        return dict(condition=cond, cfm=cfm, pivots=piv, ok=ok.astype(bool))

    def stabilize(self, mode, max_steps=0, detect_contacts=True, params=None):
        """Ensemble::InitStabilize (mode STABILIZE_INIT) or PostStabilize(max_steps) (STABILIZE_POST) for every
        ensemble (egs_world_stabilize); max_steps = 0 is the reference's 100 / 500, params None the adapter's
        relaxation solve.  Returns how many ensembles ended with err_sq > 1e-9; stabilize_info() has the figures."""
        nu = C.c_int32(0)
        self.ctx.check(load().egs_world_stabilize(self.h, C.c_int32(mode), C.c_int32(max_steps),
                                                  C.c_int32(1 if detect_contacts else 0),
                                                  C.byref(params) if params is not None else None, C.byref(nu)))
        return nu.value

    def stabilize_direct(self, mode, max_steps=0, detect_contacts=True, rank_tol=0.0):
        """stabilize() with the relaxation system solved directly on the device, a workgroup per ensemble
        (egs_world_stabilize_direct): a pivoted LDL^T truncated at the first pivot <= rank_tol * |first pivot|
        (0: 1e-10).  Returns how many ensembles ended with err_sq > 1e-9; stabilize_info() / stabilize_rank()."""
        nu = C.c_int32(0)
        self.ctx.check(load().egs_world_stabilize_direct(self.h, C.c_int32(mode), C.c_int32(max_steps),
                                                         C.c_int32(1 if detect_contacts else 0), C.c_double(rank_tol),
                                                         C.byref(nu)))
        return nu.value

    def stabilize_rank(self):
        """Per-ensemble figures of the last stabilize_direct: rows of the system and the rank of the last pass solved [E]."""
        E = self.n_ensembles
        rows = np.zeros(E, np.int32); rank = np.zeros(E, np.int32)
        self.ctx.check(load().egs_world_stabilize_rank(self.h, C.c_int32(E), _p(rows), _p(rank)))
        return dict(rows=rows, rank=rank)

    def stabilize_info(self):
        """Per-ensemble figures of the last stabilize: relaxation steps and the final err_sq [E]."""
        E = self.n_ensembles
        steps = np.zeros(E, np.int32); err_sq = np.zeros(E)
        self.ctx.check(load().egs_world_stabilize_info(self.h, C.c_int32(E), _p(steps), _p(err_sq)))
        return dict(steps=steps, err_sq=err_sq)

    def bodies(self):
        pos = np.zeros((self.n, 3)); R = np.zeros((self.n, 9)); v = np.zeros((self.n, 3)); w = np.zeros((self.n, 3))
        self.ctx.check(load().egs_world_get_bodies(self.h, _p(pos), _p(R), _p(v), _p(w)))
        return pos, R, v, w

    def info(self):
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.ctx.check(load().egs_world_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_constraints=a.value, n_contacts=b.value, replans=c.value)

    def contacts(self):
        m = self.info()["n_contacts"]
        b0 = np.zeros(m, np.int32); b1 = np.zeros(m, np.int32); data = np.zeros((m, 7)); mo = C.c_int32(0)
        self.ctx.check(load().egs_world_get_contacts(self.h, C.c_int32(m), C.byref(mo), _p(b0), _p(b1), _p(data)))
        return b0, b1, data

    def set_friction(self, mu):
        """The Coulomb pyramid per ensemble (egs_world_set_friction): every contact of ensemble e takes mu[e] (a scalar
        for a plain world), joints none; mu[e] < 0 keeps the reference's friction box."""
        mu = np.atleast_1d(_f64(mu))
        self.ctx.check(load().egs_world_set_friction(self.h, C.c_int32(mu.shape[0]), _p(mu)))

    def set_restitution(self, rest, vth=0.0):
        """Restitution per ensemble (egs_world_set_restitution): every contact of ensemble e takes rest[e] (a scalar for a
        plain world), joints none; rest[e] < 0: that ensemble's contacts do not bounce."""
        rest = None if rest is None else np.atleast_1d(_f64(rest))
        self.ctx.check(load().egs_world_set_restitution(self.h, C.c_int32(0 if rest is None else rest.shape[0]), _p(rest), float(vth)))

    def set_warm_start(self, enable, match_radius=0.01):
        """Sweep steps start from the previous step's lambda (egs_world_set_warm_start): a contact takes the rows of the
        nearest previous contact of its body pair within match_radius (metres, world frame), a joint its own."""
        self.ctx.check(load().egs_world_set_warm_start(self.h, C.c_int32(1 if enable else 0), C.c_double(match_radius)))

    def start(self):
        """x0 [3m] and source [m] of the last warm-started step (egs_world_get_start): per constraint the previous
        contact (joint) index its rows came from, -1: none within the radius (x0 = 0), -2: no history (x0 = rhs)."""
        m = self.info()["n_constraints"]
        x0 = np.zeros(3 * m); src = np.zeros(m, np.int32); ro = C.c_int32(0)
        self.ctx.check(load().egs_world_get_start(self.h, C.c_int32(3 * m), C.byref(ro), _p(x0), _p(src)))
        return x0, src

    def lambda_(self):
        rows = 3 * self.info()["n_constraints"]
        x = np.zeros(rows); ro = C.c_int32(0)
        self.ctx.check(load().egs_world_get_lambda(self.h, C.c_int32(rows), C.byref(ro), _p(x)))
        return x
