"""CPU: the hinge angle limits as mathematics (tests/limit_reference.py).  The angle's rate against the exact rigid
motion; the half-angle comparison against atan2; the fp64 twin within its bounds of the reference and agreeing with it
on which stop is active; the library, the header and the adapter carry the new entries."""
import ctypes
import math
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import joint_reference as jr
import limit_reference as lr
import model_reference as mr
from test_joint_reference_cpu import H, _moved, _orth, _rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [False, True], ids=["two-body", "world"])
def test_angle_rate_is_the_axis_row(world):
    """Both bodies move by exp(h [w]x) from a pose at angle theta0 about the common axis: the central difference of
    theta = atan2(sn, cs) is s^ . (w0 - w1), the axis row's J0 s0 + J1 s1, to O(h^2).  theta is a smooth function of the
    two rotations built from products of at most four O(1) factors, so, as for the blocks of test_joint_reference_cpu,
    the truncation h^2 / 6 of its third derivative is bounded by h^2 (|w0| + |w1|)^3."""
    rng = np.random.default_rng(23 + world)
    with mp.workdps(mr.DPS):
        for th0 in (0.0, 0.3, -1.2, 2.5):
            R1 = None if world else _orth(_rot(rng))
            R00 = _orth(_rot(rng))
            s = mr._v(rng.normal(size=3)); n = mp.sqrt(sum(x * x for x in s)); s = [x / n for x in s]
            R0 = mr._mul(mr.rodrigues_exp([mp.mpf(th0) * x for x in s]), R00)
            a0 = mr._mv(mr._T(R0), s)
            Rq = mr._mul(mr._T(R00), R1 if R1 is not None else mr._eye())
            w0 = mr._v(rng.uniform(-3, 3, 3))
            w1 = [mp.mpf(0)] * 3 if world else mr._v(rng.uniform(-3, 3, 3))

            def theta_at(h):
                A = _moved(R0, w0, h)
                B = _moved(R1, w1, h) if R1 is not None else mr._eye()
                E = mr._mul(mr._mul(A, Rq), mr._T(B))
                ax = [(E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2]
                sa = mr._mv(A, a0)
                return mp.atan2(sum(x * y for x, y in zip(sa, ax)), ((E[0][0] + E[1][1] + E[2][2]) - 1) / 2)
            assert abs(theta_at(mp.mpf(0)) - th0) < mp.mpf("1e-45")
            fd = (theta_at(H) - theta_at(-H)) / (2 * H)
            want = sum(x * (a - b) for x, a, b in zip(s, w0, w1))
            bound = H * H * (sum(abs(x) for x in w0) + sum(abs(x) for x in w1)) ** 3
            assert abs(fd - want) <= bound, (th0, float(fd - want), float(bound))


def test_half_angle_comparison_is_the_atan2_comparison():
    """sn (1 + cl) > sl (1 + cs) in fp64 against theta > limit, on seeded angles over (-pi, pi) with |theta| > 3 among them
    and both at least MARGIN apart in tan(x / 2): the same answer every time, for either stop."""
    rng = np.random.default_rng(41)
    thetas = np.concatenate([rng.uniform(-math.pi, math.pi, 300), rng.uniform(3.0, 3.14, 50), rng.uniform(-3.14, -3.0, 50)])
    limits = np.concatenate([rng.uniform(-3.13, 3.13, 350), rng.uniform(3.0, 3.13, 25), rng.uniform(-3.13, -3.0, 25)])
    rng.shuffle(limits)
    beyond, used = 0, 0
    for th, lm in zip(thetas, limits):
        if abs(math.tan(th / 2) - math.tan(lm / 2)) < lr.MARGIN:      # (never with this seed: asserted below)
            continue
        used += 1
        sn, cs, sl, cl = math.sin(th), math.cos(th), math.sin(lm), math.cos(lm)
        assert (sn * (1.0 + cl) > sl * (1.0 + cs)) == (th > lm), (th, lm)
        assert (sn * (1.0 + cl) < sl * (1.0 + cs)) == (th < lm), (th, lm)
        beyond += abs(th) > 3
    assert used == thetas.size and beyond >= 100


CIDS = ["n4m8-a", "n4m8-b", "m259"]


@pytest.mark.parametrize("cid", CIDS)
def test_twin_within_bounds_and_agrees_on_activity(cid):
    """err[2] of the twin within the product-sum bound of the reference (limit_reference's docstring has the terms), and
    the twin's half-angle decision equal to the reference's atan2 decision on every hinge of every family."""
    case, motor, _, _, _ = jr.generated(cid)
    seen = set()
    for fam, off in lr.FAMILIES.items():
        lim = lr.make_limits(case, off)
        tw = lr.twin_assemble(case, motor, lim)
        ref = lr.case_reference(case, lim)
        worst = 0.0
        with mp.workdps(mr.DPS):
            for i, r in enumerate(ref):
                if r is None:
                    assert tw["active"][i] == 0
                    continue
                act, err, tol, dist, theta = r
                assert dist > lr.MARGIN
                assert tw["active"][i] == act, (cid, fam, i, float(theta))
                seen.add(act)
                if act:
                    d = abs(mp.mpf(float(tw["err"][3 * i + 2])) - err)
                    worst = max(worst, float(d / tol))
                    assert d <= tol, (cid, fam, i, float(d), float(tol))
                    # sin(theta - limit), with the sign the bounds go with
                    L = lim[i]
                    lm = math.atan2(L[6], L[7]) if act > 0 else math.atan2(L[4], L[5])
                    assert abs(float(err) - math.sin(float(theta) - lm)) < 1e-14 and (float(err) > 0) == (act > 0)
                    assert (tw["lo"][3 * i + 2], tw["hi"][3 * i + 2]) == ((-math.inf, 0.0) if act > 0 else (0.0, math.inf))
                assert tw["is_eq"][3 * i + 2] == 0
        print(cid, fam, "worst err[2] error / tolerance %.3g" % worst)
    assert seen == {-1, 0, 1}


def test_limit_rows_of_the_twin():
    """What the table may touch: row 2 of a hinge with an active stop, nothing else; a motor's row under an active stop
    is the limit's, inside the range the motor's."""
    case, motor, _, plain, driven = jr.generated("m259")
    lim = lr.make_limits(case, 0)
    tw = lr.twin_assemble(case, motor, lim)
    both = 0
    for i in range(case["kind"].shape[0]):
        rows = slice(3 * i, 3 * i + 3) if not tw["active"][i] else slice(3 * i, 3 * i + 2)
        for name in ("err", "lo", "hi", "rhs"):
            assert jr.bits_equal(tw[name][rows], driven[name][rows]), (i, name)
        assert jr.bits_equal(tw["J0"][i], driven["J0"][i]) and jr.bits_equal(tw["J1"][i], driven["J1"][i])
        if tw["active"][i] and jr.motor_applies(case, motor, i):
            both += 1
            assert (tw["lo"][3 * i + 2], tw["hi"][3 * i + 2]) in ((-math.inf, 0.0), (0.0, math.inf))
            assert tw["err"][3 * i + 2] != 0.0 and tw["rhs"][3 * i + 2] != driven["rhs"][3 * i + 2]
    assert both > 0
    off = lr.twin_assemble(case, motor, np.zeros((case["kind"].shape[0], 8)))
    for name in ("err", "lo", "hi", "rhs"):
        assert jr.bits_equal(off[name], driven[name])


# ---- the library, the header, the adapter ----------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = ctypes.CDLL(os.path.join(ROOT, "eggshell_amd", "libeggshell_amd.so"))
    for name in ("egs_problem_set_hinge_limits", "egs_world_set_joint_limits"):
        assert hasattr(lib, name), name
    from eggshell_amd import capi
    assert {"egs_problem_set_hinge_limits", "egs_world_set_joint_limits"} <= set(capi.EXPORTS)
    assert hasattr(capi.Problem, "set_hinge_limits") and hasattr(capi.World, "set_joint_limits")


def test_header_keeps_its_four_kinds_and_declares_the_limits():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} egs_constraint_kind;", text).group(1)
    values = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in body.split(",")))
    assert values == {"EGS_JOINT_BALL": 0, "EGS_CONTACT_BOX": 1, "EGS_JOINT_LOCK": 2, "EGS_JOINT_HINGE_AXIS": 3}
    for name in ("egs_problem_set_hinge_limits", "egs_world_set_joint_limits"):
        assert re.search(r"egs_status %s\(" % name, text), name


def test_adapter_and_hinge_limit_demo_compile(tmp_path):
    host = os.path.join(ROOT, "eggshell_amd", "host")
    for src in ("hinge_limit_demo.cpp", "eggshell_api.cpp"):
        cmd = ["g++", "-std=c++17", "-O0", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + host, "-c",
               os.path.join(host, src), "-o", str(tmp_path / (src + ".o"))]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
    text = open(os.path.join(host, "eggshell_api.h")).read()
    for name in ("SetLimits", "SetHingeLimits", "HingeAngle"):
        assert name in text, name


def test_host_side_of_the_limits_under_sanitizers(tmp_path):
    """host/limit_host_check.cpp: HingeAxisJoint's captured q, SetLimits, ComputeError in the device's order, and
    Ensemble::SetHingeLimits / HingeAngle with their refusals, as a stand-alone program built with
    -fsanitize=address,undefined and run on the CPU (it creates no device context)."""
    host = os.path.join(ROOT, "eggshell_amd", "host")
    out = str(tmp_path / "limit_host_check")
    res = subprocess.run(["make", "-B", "-C", host, "limit_host_check", "LIMIT_CHECK_OUT=" + out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "eggshell_amd") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime the library links keeps its start-up allocations)
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and "limit_host_check: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])
