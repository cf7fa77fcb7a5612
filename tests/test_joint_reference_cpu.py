"""CPU: the angular joint blocks as mathematics (tests/joint_reference.py).  The reference checks itself against the
exact rigid motion; the fp64 twin lies within its bounds of the reference; the library, the header and the adapter
carry the new entries."""
import ctypes
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import joint_reference as jr
import model_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = mp.mpf("1e-12")


def _rot(rng):
    return mr._m3(mr.random_rotations(rng, 1)[0])


def _orth(R):
    """The mpf matrix, re-orthonormalised at 50 digits (Gram-Schmidt): the fp64 entries are orthonormal only to 1e-16."""
    a, b = R[0], R[1]
    na = mp.sqrt(sum(x * x for x in a)); a = [x / na for x in a]
    d = sum(x * y for x, y in zip(a, b)); b = [y - d * x for x, y in zip(a, b)]
    nb = mp.sqrt(sum(x * x for x in b)); b = [x / nb for x in b]
    return [a, b, mr._cross(a, b)]


def _moved(R, w, h):
    return mr._mul(mr.rodrigues_exp([h * x for x in w]), R)


@pytest.mark.parametrize("world", [False, True], ids=["two-body", "world"])
@pytest.mark.parametrize("kind", [jr.LOCK, jr.HINGE], ids=["lock", "hinge"])
def test_error_rate_is_the_jacobian(kind, world):
    """err exactly 0; both bodies move by exp(h [w]x): the central difference of err is J0 s0 + J1 s1 to O(h^2).  The
    third derivative of a product of two such motions is below (|w0| + |w1|)^3 times the O(1) entries it multiplies (at
    most four unit-vector factors for the hinge), so the truncation h^2 / 6 of it is bounded by h^2 (|w0| + |w1|)^3."""
    rng = np.random.default_rng(11 + kind + 7 * world)
    with mp.workdps(mr.DPS):
        for _ in range(8):
            R0 = _orth(_rot(rng))
            R1 = None if world else _orth(_rot(rng))
            w0 = mr._v(rng.uniform(-3, 3, 3))
            w1 = [mp.mpf(0)] * 3 if world else mr._v(rng.uniform(-3, 3, 3))
            if kind == jr.LOCK:
                # E = R0 Rq R1^T = I: Rq = R0^T R1, handed over as a matrix through a patched quat_matrix-free path
                Rq = mr._mul(mr._T(R0), R1 if R1 is not None else mr._eye())

                def err_at(h):
                    A = _moved(R0, w0, h)
                    B = _moved(R1, w1, h) if R1 is not None else mr._eye()
                    E = mr._mul(mr._mul(A, Rq), mr._T(B))
                    return [(E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2]
                J = mr._eye()
            else:
                s = mr._v(rng.normal(size=3)); n = mp.sqrt(sum(x * x for x in s)); s = [x / n for x in s]
                a0 = mr._mv(mr._T(R0), s)
                a1 = mr._mv(mr._T(R1), s) if R1 is not None else s
                J = jr.hinge_reference(R0, R1, a0, a1)[2]

                def err_at(h):
                    # the frame (p, q, s^) is held at its value at h = 0, as the Jacobian is: d err = Rn d(c)
                    A = _moved(R0, w0, h)
                    B = _moved(R1, w1, h) if R1 is not None else None
                    sa = mr._mv(A, a0)
                    ta = mr._mv(B, a1) if B is not None else a1
                    c = mr._cross(ta, sa)
                    return [sum(J[r][k] * c[k] for k in range(3)) for r in range(2)] + [mp.mpf(0)]
            e0 = err_at(mp.mpf(0))
            assert max(abs(x) for x in e0) < mp.mpf("1e-45")
            fd = [(a - b) / (2 * H) for a, b in zip(err_at(H), err_at(-H))]
            rel = [a - b for a, b in zip(w0, w1)]
            want = mr._mv(J, rel)
            if kind == jr.HINGE:
                want[2] = mp.mpf(0)      # the axis row carries no error: its Jacobian row is the motor's
            bound = H * H * (sum(abs(x) for x in w0) + sum(abs(x) for x in w1)) ** 3
            assert max(abs(a - b) for a, b in zip(fd, want)) <= bound


def test_hinge_frame_moves_at_second_order():
    """... and with the frame recomputed at the moved pose, as the assembly does, err still starts at the same rate: the
    frame's own motion multiplies c, which is 0 at err = 0."""
    rng = np.random.default_rng(5)
    with mp.workdps(mr.DPS):
        R0, R1 = _orth(_rot(rng)), _orth(_rot(rng))
        s = [mp.mpf(0), mp.mpf(3) / 5, mp.mpf(4) / 5]
        a0, a1 = mr._mv(mr._T(R0), s), mr._mv(mr._T(R1), s)
        w0, w1 = mr._v(rng.uniform(-3, 3, 3)), mr._v(rng.uniform(-3, 3, 3))
        Rn = jr.hinge_reference(R0, R1, a0, a1)[2]
        ep = jr.hinge_reference(_moved(R0, w0, H), _moved(R1, w1, H), a0, a1)[0]
        en = jr.hinge_reference(_moved(R0, w0, -H), _moved(R1, w1, -H), a0, a1)[0]
        fd = [(a - b) / (2 * H) for a, b in zip(ep, en)]
        want = mr._mv(Rn, [a - b for a, b in zip(w0, w1)])
        bound = H * H * (sum(abs(x) for x in w0) + sum(abs(x) for x in w1)) ** 3
        assert abs(fd[0] - want[0]) <= bound and abs(fd[1] - want[1]) <= bound and fd[2] == 0


def test_known_error_is_sin_theta_n():
    """Body 0 turned by 0.05 rad about a known axis n from the locked pose: err = sin(theta) n; a hinge whose body 0 is
    turned about an n across its axis: err0 p + err1 q = sin(theta) n."""
    rng = np.random.default_rng(3)
    with mp.workdps(mr.DPS):
        th = mp.mpf("0.05")
        R0, R1 = _orth(_rot(rng)), _orth(_rot(rng))
        n = [mp.mpf(2) / 7, mp.mpf(3) / 7, mp.mpf(6) / 7]
        bent = mr._mul(mr.rodrigues_exp([th * x for x in n]), R0)
        Rq = mr._mul(mr._T(R0), R1)
        E = mr._mul(mr._mul(bent, Rq), mr._T(R1))
        err = [(E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2]
        assert max(abs(e - mp.sin(th) * x) for e, x in zip(err, n)) < mp.mpf("1e-45")
        # the same through the quaternion the library is given (rounded to fp64: within its bound of the exact value)
        q = mr._v(jr.lock_data(np.array([[float(x) for x in row] for row in R0]), np.array([[float(x) for x in row] for row in R1]))[:4])
        e2, tol = jr.lock_reference(bent, R1, q)
        assert max(abs(e - mp.sin(th) * x) for e, x in zip(e2, n)) < mp.mpf("1e-14")
        # hinge: s across n
        s = mr._cross(n, [mp.mpf(1), mp.mpf(0), mp.mpf(0)]); ln = mp.sqrt(sum(x * x for x in s)); s = [x / ln for x in s]
        a0, a1 = mr._mv(mr._T(R0), s), mr._mv(mr._T(R1), s)
        e, _, Rn, _, _ = jr.hinge_reference(bent, R1, a0, a1)
        back = [e[0] * Rn[0][k] + e[1] * Rn[1][k] for k in range(3)]
        # Rn is the frame of the turned axis, which still lies across n
        assert max(abs(b - mp.sin(th) * x) for b, x in zip(back, n)) < mp.mpf("1e-45")
        assert e[2] == 0


@pytest.mark.parametrize("cid", jr.IDS)
def test_twin_within_bounds(cid):
    case, motor, asm, plain, driven = jr.generated(cid)
    r0 = jr.check_twin(case, asm, plain)
    r1 = jr.check_twin(case, asm, driven, motor)
    print(cid, "worst error / tolerance without the motor", r0, "with it", r1)
    for r in (r0, r1):
        for k, x in r.items():
            assert x <= 1.0, (cid, k, x)
    kinds = set(int(k) for k in case["kind"])
    assert kinds == {0, 1, 2, 3}
    ang = case["kind"] >= 2
    assert (case["body1"][ang] < 0).any() and (case["body1"][ang] >= 0).any()
    # the linear columns of the angular blocks are exactly +0, the lock's J is +-I to the bit
    for i in np.nonzero(ang)[0]:
        for J in (plain["J0"], plain["J1"]):
            assert jr.bits_equal(J[i].reshape(3, 6)[:, :3], np.zeros((3, 3)))
        if case["kind"][i] == jr.LOCK:
            assert np.array_equal(plain["J0"][i].reshape(3, 6)[:, 3:], np.eye(3))
            assert np.array_equal(plain["J1"][i].reshape(3, 6)[:, 3:], -np.eye(3) if case["body1"][i] >= 0 else np.zeros((3, 3)))


def test_motor_rows_of_the_twin():
    case, motor, asm, plain, driven = jr.generated("n4m8-a")
    for i in range(case["kind"].shape[0]):
        on = jr.motor_applies(case, motor, i)
        assert (driven["hi"][3 * i + 2] == motor[i][1] and driven["lo"][3 * i + 2] == -motor[i][1]) if on else \
            jr.bits_equal(driven["hi"][3 * i:3 * i + 3], plain["hi"][3 * i:3 * i + 3])
        rows = slice(3 * i, 3 * i + (2 if on else 3))
        assert jr.bits_equal(driven["rhs"][rows], plain["rhs"][rows])


# ---- the library, the header, the adapter ----------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = ctypes.CDLL(os.path.join(ROOT, "eggshell_amd", "libeggshell_amd.so"))
    for name in ("egs_problem_set_motors", "egs_world_set_joints_kinds", "egs_world_set_joint_motors"):
        assert hasattr(lib, name), name
    from eggshell_amd import capi
    assert {"egs_problem_set_motors", "egs_world_set_joints_kinds", "egs_world_set_joint_motors"} <= set(capi.EXPORTS)
    assert (capi.JOINT_LOCK, capi.JOINT_HINGE_AXIS) == (2, 3)


def test_header_enum_values():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} egs_constraint_kind;", text).group(1)
    values = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in body.split(",")))
    assert values == {"EGS_JOINT_BALL": 0, "EGS_CONTACT_BOX": 1, "EGS_JOINT_LOCK": 2, "EGS_JOINT_HINGE_AXIS": 3}


def test_adapter_and_hinge_demo_compile(tmp_path):
    """The adapter with the two joint classes and host/hinge_demo.cpp compile."""
    host = os.path.join(ROOT, "eggshell_amd", "host")
    for src in ("hinge_demo.cpp", "eggshell_api.cpp"):
        cmd = ["g++", "-std=c++17", "-O0", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + host, "-c",
               os.path.join(host, src), "-o", str(tmp_path / (src + ".o"))]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
    text = open(os.path.join(host, "eggshell_api.h")).read()
    for name in ("class AngularLockJoint", "class HingeAxisJoint", "HasPosition", "AddWeld", "AddHinge", "SetHingeMotor"):
        assert name in text, name


def test_host_side_of_the_joints_under_sanitizers(tmp_path):
    """host/joint_host_check.cpp: ComputeError, ComputeJ and Describe of the two joint classes, AddWeld, AddHinge and
    SetHingeMotor, as a stand-alone program built with -fsanitize=address,undefined and run on the CPU (it creates no
    device context)."""
    host = os.path.join(ROOT, "eggshell_amd", "host")
    out = str(tmp_path / "joint_host_check")
    res = subprocess.run(["make", "-B", "-C", host, "joint_host_check", "CHECK_OUT=" + out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "eggshell_amd") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime the library links keeps its start-up allocations)
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and "joint_host_check: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])
