"""CPU: the slider block as mathematics (tests/slider_reference.py).  The rates of err and of the travel against the
exact rigid motion; the block's net force and torque; the fp64 twin within its bounds of the reference and agreeing
with it on which stop is active; the library, the header and the adapter carry the new entries."""
import ctypes
import math
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import joint_reference as jr
import model_reference as mr
import slider_reference as sr
from test_joint_reference_cpu import H, _moved, _orth, _rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose(rng, world, x, across):
    """A slider pose in mpf: (p0, R0, p1 or None, a0, c, s), D = x s + across * (a unit vector across s).  The rail
    direction is kept with s_z >= -1/2, so 1 + c >= 1/2 in align_to_z (the bound below uses it)."""
    R0 = _orth(_rot(rng))
    while True:
        s = rng.normal(size=3)
        s /= np.linalg.norm(s)
        if s[2] >= -0.5:
            break
    s = mr._v(s); n = mp.sqrt(sum(v * v for v in s)); s = [v / n for v in s]
    t = mr._cross(s, mr._v(rng.normal(size=3))); n = mp.sqrt(sum(v * v for v in t)); t = [v / n for v in t]
    D = [mp.mpf(x) * a + mp.mpf(across) * b for a, b in zip(s, t)]
    p0 = mr._v(rng.uniform(-2, 2, 3))
    a0 = mr._mv(mr._T(R0), s)
    if world:
        return p0, R0, None, a0, [a - b for a, b in zip(p0, D)], s
    p1 = mr._v(rng.uniform(-2, 2, 3))
    return p0, R0, p1, a0, mr._mv(mr._T(R0), [d - a + b for d, a, b in zip(D, p0, p1)]), s


def _rate_and_bound(rng, world, x, across, rows):
    """The central difference of the rows named (0, 1: err; 2: the travel x) of a slider under the exact rigid motion of
    both bodies, what J0 s0 + J1 s1 says, and the truncation bound.

    The bound.  Row r is f(h) = sum_k Rn_rk(h) D_k(h), the frame recomputed at the moved pose as the assembly does.
    s(h) = exp(h [w0]x) s has |s^(n)| <= W^n, W = |w0|.  With s^ = (x, y, z), k = 1 + z >= 1/2 an entry of Rn is one of
    x, y, z, or 1 - g / k, -g / k with g a product of two of x, y: |g| <= 1, |g'| <= 2W, |g''| <= 4W^2, |g'''| <= 8W^3;
    |(1/k)| <= 2, |(1/k)'| <= 4W, |(1/k)''| <= 4W^2 + 16W^2 = 20W^2, |(1/k)'''| <= 4W^3 + 48W^3 + 96W^3 = 148W^3.
    By the product rule an entry e has |e| <= 1 (a rotation matrix), |e'| <= 2*2W + 4W = 8W, |e''| <= 8 + 16 + 20 = 44W^2,
    |e'''| <= 16 + 48 + 120 + 148 = 332W^3.  D(h) = p0 + h v0 + exp(h [w0]x) R0 c - p1 - h v1 has |D'| <= V = |v0| + |v1| +
    W |c|, |D''| <= W^2 |c|, |D'''| <= W^3 |c|, and |D| <= |D(0)| + h V.  So
        |f'''| <= 3 (332 W^3 Dmax + 3 * 44 W^2 V + 3 * 8 W W^2 |c| + W^3 |c|)
    and the central difference is off by at most h^2 / 6 of it.  Norms are taken as 1-norms (no smaller than these)."""
    p0, R0, p1, a0, c, s = _pose(rng, world, x, across)
    v0, w0 = mr._v(rng.uniform(-2, 2, 3)), mr._v(rng.uniform(-3, 3, 3))
    v1 = mr._v(rng.uniform(-2, 2, 3)) if not world else [mp.mpf(0)] * 3
    ref = sr.slider_reference(p0, R0, p1, a0, c)

    def at(h):
        r = sr.slider_reference([a + h * b for a, b in zip(p0, v0)], _moved(R0, w0, h),
                                None if world else [a + h * b for a, b in zip(p1, v1)], a0, c)
        return [r["err"][0], r["err"][1], r["x"]]
    fd = [(a - b) / (2 * H) for a, b in zip(at(H), at(-H))]
    # body 1 enters through its centre only: its turning rate meets the zero angular columns of J1
    s0, s1 = v0 + w0, v1 + [mp.mpf(0)] * 3
    want = [sum(ref["J0"][6 * r + k][0] * s0[k] + ref["J1"][6 * r + k][0] * s1[k] for k in range(6)) for r in range(3)]
    n1 = lambda v: sum(abs(t) for t in v)
    W, cn = n1(w0), (n1(c) if not world else mp.mpf(0))
    V = n1(v0) + n1(v1) + W * cn
    Dmax = n1(ref["D"]) + H * V
    bound = H * H / 6 * 3 * (332 * W ** 3 * Dmax + 132 * W ** 2 * V + 24 * W ** 3 * cn + W ** 3 * cn)
    return ref, [(r, fd[r], want[r], bound) for r in rows]


@pytest.mark.parametrize("world", [False, True], ids=["two-body", "world"])
def test_error_rate_is_the_jacobian(world):
    """err = 0 (D along the rail, any travel x, any c, v and w): the central difference of err[0..1] under the exact
    rigid motion of both bodies is rows 0 and 1 of J0 s0 + J1 s1, within the bound of _rate_and_bound."""
    rng = np.random.default_rng(71 + world)
    with mp.workdps(mr.DPS):
        for x in (0.0, 0.7, -1.9, 3.2):
            ref, out = _rate_and_bound(rng, world, x, 0.0, (0, 1))
            assert max(abs(e) for e in ref["err"]) < mp.mpf("1e-45")
            for r, fd, want, bound in out:
                assert abs(fd - want) <= bound, (x, r, float(fd - want), float(bound))
                assert abs(want) > 1e-3      # (the rows are not trivially zero)


@pytest.mark.parametrize("world", [False, True], ids=["two-body", "world"])
def test_travel_rate_is_the_rail_row_at_every_pose(world):
    """... and the travel x = s^ . D moves at row 2 of J0 s0 + J1 s1 at poses with err != 0 as well (0.3 across the rail)."""
    rng = np.random.default_rng(81 + world)
    with mp.workdps(mr.DPS):
        for x, across in ((0.0, 0.3), (0.7, -0.3), (-1.9, 0.0), (3.2, 0.25)):
            ref, out = _rate_and_bound(rng, world, x, across, (2,))
            assert abs(mp.sqrt(ref["err"][0] ** 2 + ref["err"][1] ** 2) - abs(mp.mpf(across))) < mp.mpf("1e-45")
            assert abs(ref["x"] - x) < mp.mpf("1e-45")
            for r, fd, want, bound in out:
                assert abs(fd - want) <= bound, (x, r, float(fd - want), float(bound))


def test_block_carries_no_net_force_or_torque():
    """For any lambda the wrenches J0^T lambda on body 0 and J1^T lambda on body 1 sum to zero force and to zero torque
    about the origin: the lever arm (P1 - p0) on body 0 alone is the right one."""
    rng = np.random.default_rng(91)
    with mp.workdps(mr.DPS):
        for x, across in ((0.4, 0.0), (-1.1, 0.2), (2.0, -0.4)):
            p0, R0, p1, a0, c, _ = _pose(rng, False, x, across)
            ref = sr.slider_reference(p0, R0, p1, a0, c)
            lam = mr._v(rng.uniform(-5, 5, 3))
            w0 = [sum(ref["J0"][6 * r + k][0] * lam[r] for r in range(3)) for k in range(6)]
            w1 = [sum(ref["J1"][6 * r + k][0] * lam[r] for r in range(3)) for k in range(6)]
            force = [a + b for a, b in zip(w0[:3], w1[:3])]
            torque = [a + b + c0 + c1 for a, b, c0, c1 in zip(w0[3:], w1[3:], mr._cross(p0, w0[:3]), mr._cross(p1, w1[:3]))]
            assert max(abs(v) for v in force) == 0
            assert max(abs(v) for v in torque) < mp.mpf("1e-45")
            assert max(abs(v) for v in w0[:3]) > 1e-2


CHECKS = [(cid, fam) for cid in ("n4m8-a", "n4m8-b", "n4m8-c") for fam in sr.FAMILIES] + [("m259", "mixed")]


def test_twin_within_bounds_and_agrees_on_activity():
    """J, err and rhs of the twin within the product-sum bounds of the reference (slider_reference's docstring has the
    terms), with and without the motor, on every family; the twin's stop decision equal to the reference's on every
    slider; the bounds and the sign of err[2] as specified; all of {upper, none, lower} seen."""
    seen, worst = set(), {"J": 0.0, "err": 0.0, "rhs": 0.0}
    for cid, fam in CHECKS:
        case, motor = sr.generated(cid)
        kinds = set(int(k) for k in case["kind"])
        assert kinds == {0, 1, 2, 3, 5}
        sl = case["kind"] == sr.SLIDER
        assert (case["body1"][sl] < 0).any() and (case["body1"][sl] >= 0).any() and np.abs(case["data"][sl][:, 3:6]).min() > 0
        travel = sr.make_travel(case, fam)
        asm = sr.assemble_reference(case, travel)
        for i in np.nonzero(sl)[0]:
            assert asm["dist"][i] > sr.MARGIN > float(asm["x"][i][1])      # the stop is further off than x is uncertain
        for mot in (None, motor):
            tw = sr.twin_assemble(case, mot, travel)
            r = sr.check_twin(case, asm, tw, mot)
            for k, v in r.items():
                assert v <= 1.0, (cid, fam, k, v)
                worst[k] = max(worst[k], v)
            for i in np.nonzero(sl)[0]:
                act, k = int(tw["active"][i]), 3 * i + 2
                seen.add(act)
                assert tw["is_eq"][k] == 0
                if act:
                    assert (tw["lo"][k], tw["hi"][k]) == ((-math.inf, 0.0) if act > 0 else (0.0, math.inf))
                    assert (tw["err"][k] > 0) == (act > 0) and abs(tw["err"][k]) > 0.09
                elif sr.slider_motor_applies(case, mot, i):
                    assert tw["err"][k] == 0.0 and (tw["lo"][k], tw["hi"][k]) == (-mot[i][1], mot[i][1])
                else:
                    assert tw["err"][k] == 0.0 and (tw["lo"][k], tw["hi"][k]) == (0.0, 0.0)
    print("worst twin error / tolerance", worst)
    assert seen == {-1, 0, 1}


def test_tables_touch_the_rail_row_only():
    """What the tables may touch: row 2 of a slider; an all-infinite table and the rows of other kinds change nothing; a
    motor's row under an active stop is the stop's."""
    case, motor = sr.generated("m259")
    plain, driven = sr.twin_assemble(case), sr.twin_assemble(case, motor)
    off = sr.twin_assemble(case, motor, sr.make_travel(case, "all-infinite"))
    tw = sr.twin_assemble(case, motor, sr.make_travel(case, "mixed"))
    both = 0
    for name in ("J0", "J1", "err", "lo", "hi", "rhs", "is_eq"):
        assert jr.bits_equal(off[name], driven[name]), name
    for i in range(case["kind"].shape[0]):
        rows = slice(3 * i, 3 * i + 3) if not tw["active"][i] else slice(3 * i, 3 * i + 2)
        for name in ("err", "lo", "hi", "rhs"):
            assert jr.bits_equal(tw[name][rows], driven[name][rows]), (i, name)
            assert jr.bits_equal(driven[name][3 * i:3 * i + 2], plain[name][3 * i:3 * i + 2])
        assert jr.bits_equal(tw["J0"][i], plain["J0"][i]) and jr.bits_equal(tw["J1"][i], plain["J1"][i])
        assert not tw["active"][i] or case["kind"][i] == sr.SLIDER
        if tw["active"][i] and sr.slider_motor_applies(case, motor, i):
            both += 1
            assert tw["rhs"][3 * i + 2] != driven["rhs"][3 * i + 2]
    assert both > 0


# ---- the library, the header, the adapter ----------------------------------------------------------------------------------
NEW = ("egs_problem_set_slider_limits", "egs_world_set_slider_limits")


def test_library_exports_the_entries():
    lib = ctypes.CDLL(os.path.join(ROOT, "eggshell_amd", "libeggshell_amd.so"))
    for name in NEW:
        assert hasattr(lib, name), name
    from eggshell_amd import capi
    assert set(NEW) <= set(capi.EXPORTS)
    assert capi.JOINT_SLIDER_AXIS == 5
    assert hasattr(capi.Problem, "set_slider_limits") and hasattr(capi.World, "set_slider_limits")


def test_header_declares_the_kind_and_the_entries():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    assert re.search(r"EGS_JOINT_SLIDER_AXIS\s*=\s*5\b", text)
    assert not re.search(r"\bEGS_(JOINT|CONTACT)_\w+\s*=\s*4\b", text)      # 4 stays no kind, and the header says so
    assert "4 is no kind" in text
    for name in NEW:
        assert re.search(r"egs_status %s\(" % name, text), name


def test_adapter_and_slider_demo_compile(tmp_path):
    host = os.path.join(ROOT, "eggshell_amd", "host")
    for src in ("slider_demo.cpp", "eggshell_api.cpp"):
        cmd = ["g++", "-std=c++17", "-O0", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), "-I" + host, "-c",
               os.path.join(host, src), "-o", str(tmp_path / (src + ".o"))]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
    text = open(os.path.join(host, "eggshell_api.h")).read()
    for name in ("class SliderAxisJoint", "AddSlider", "SetSliderMotor", "SetSliderLimits", "SliderPosition"):
        assert name in text, name


def test_host_side_of_the_sliders_under_sanitizers(tmp_path):
    """host/slider_host_check.cpp: SliderAxisJoint's ComputeError, ComputeJ and Describe in the device's order, AddSlider
    (x = 0 at creation), SetSliderMotor, SetSliderLimits and SliderPosition with their refusals, as a stand-alone program
    built with -fsanitize=address,undefined and run on the CPU (it creates no device context)."""
    host = os.path.join(ROOT, "eggshell_amd", "host")
    out = str(tmp_path / "slider_host_check")
    res = subprocess.run(["make", "-B", "-C", host, "slider_host_check", "SLIDER_CHECK_OUT=" + out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "eggshell_amd") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime the library links keeps its start-up allocations)
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and "slider_host_check: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])
