"""GPU (-m gpu): the ray cast of raycast.hip through egs_cast_rays -- bit for bit the fp64 twin (ray_twin.py), within
the families' bounds of the 50-digit reference (ray_reference.py), the same bytes with the bounding-sphere cull off."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ray_reference as ref
import ray_twin as twin
from eggshell_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "eggshell_amd", "csrc", "raycast.h")) as _h:
    CHUNK = int(re.search(r"kRayChunk\s*=\s*(\d+)", _h.read()).group(1))     # bodies staged into LDS per round


def cast(ctx, f, **kw):
    return ctx.cast_rays(f["pos"], f["R"], f["side"], f["shape"], f["origin"], f["dir"], f["tmax"], **kw)


def same_bits(got, want):
    """hit_body, t and normal as bytes: -0.0 and 0.0 are different bits."""
    return all(a.tobytes() == np.ascontiguousarray(b, a.dtype).tobytes() for a, b in zip(got, want))


@pytest.fixture(scope="module")
def twins():
    return {name: twin.cast(*(ref.family(name)[k] for k in ("pos", "R", "side", "shape", "origin", "dir", "tmax")))
            for name in ref.FAMILIES}


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_family_is_the_twin_bit_for_bit_and_the_reference_within_its_bound(ctx, twins, name):
    got = cast(ctx, ref.family(name))
    assert same_bits(got, twins[name])
    worst, left_out = ref.check_family(name, *got)
    print("%s: largest error %.3g (bound %.3g), left out %d" % (name, worst, ref.BOUND[name], left_out))
    assert worst <= ref.BOUND[name]


@pytest.mark.parametrize("cull", ["0", "1"])
@pytest.mark.parametrize("name", ref.FAMILIES)
def test_cull_off_and_on_give_the_same_bytes(ctx, twins, monkeypatch, name, cull):
    """EGS_RAY_CULL=0: no bounding-sphere rejection; 1: forced on (the default takes it from the bodies per ensemble)."""
    monkeypatch.setenv("EGS_RAY_CULL", cull)
    assert same_bits(cast(ctx, ref.family(name)), twins[name])


def test_two_full_workgroups_and_one_lane(ctx, twins):
    """2 x 256 + 1 rays: the heap's fan twice and its first ray once more."""
    f = ref.family("heap")
    idx = np.concatenate([np.arange(256), np.arange(256), [0]])
    got = ctx.cast_rays(f["pos"], f["R"], f["side"], f["shape"], f["origin"][idx], f["dir"][idx], f["tmax"][idx])
    assert len(got[0]) == 513 and same_bits(got, tuple(a[idx] for a in twins["heap"]))


@pytest.mark.parametrize("swap", [False, True])
def test_one_lds_chunk_and_one_body(ctx, swap):
    """CHUNK + 1 balls, all but two of them beside the ray's path: the nearest hit on the last body (the second chunk's
    only one) and a farther one on body 0, then the two swapped."""
    n = CHUNK + 1
    pos = np.array([[10.0 + 0.5 * k, 5.0, 1.0] for k in range(n)])
    near, far = (0, n - 1) if swap else (n - 1, 0)
    pos[near], pos[far] = [3.0, 0.0, 1.0], [6.0, 0.0, 1.0]
    side, shape = np.full((n, 3), 0.4), np.full(n, capi.SHAPE_SPHERE, np.int32)
    R = np.tile(np.eye(3).reshape(9), (n, 1))
    o, d = np.array([[0.0, 0.0, 1.0], [9.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0], [-2.0, 0.0, 0.0]])
    got = ctx.cast_rays(pos, R, side, shape, o, d)          # more than a chunk of bodies: the cull is on by default
    assert list(got[0]) == [near, far] and abs(got[1][0] - 2.8) < 1e-12 and abs(got[1][1] - 1.4) < 1e-12
    assert same_bits(got, twin.cast(pos, R, side, shape, o, d, [np.inf, np.inf]))


def test_attached_rays_follow_the_carrier_and_never_see_it(ctx):
    """Rays given in a body's frame, from its centre: the device's result is the twin's on the world-frame rays the
    twin forms (o_w = c + R o, d_w = R d), and the carrier, which holds every origin, is never reported."""
    f = ref.family("heap")
    rng = np.random.default_rng(7)
    body = np.repeat(np.arange(12, dtype=np.int32), 8)
    body[::8] = -1                                          # a world-frame ray among them
    o = rng.uniform(-0.02, 0.02, (96, 3))
    o[body < 0] += [0.45, 0.24, 1.0]
    d = rng.normal(size=(96, 3))
    tmax = np.full(96, np.inf)
    got = ctx.cast_rays(f["pos"], f["R"], f["side"], f["shape"], o, d, tmax, ray_body=body)
    assert same_bits(got, twin.cast(f["pos"], f["R"], f["side"], f["shape"], o, d, tmax, ray_body=body))
    assert (got[0][body >= 0] != body[body >= 0]).all() and (got[0] >= 0).any()
    plain = ctx.cast_rays(f["pos"], f["R"], f["side"], f["shape"], *zip(*[twin.world_frame(f["pos"][b], f["R"][b], o[i], d[i])
                                                                          for i, b in enumerate(body) if b >= 0]))
    assert (plain[0] >= 0).all() and (plain[1] == 0.0).all()         # without the frame's rule a solid holds every origin


def _bad_calls():
    f = ref.family("heap")
    n = 4
    base = dict(pos=f["pos"], R=f["R"], side=f["side"], shape=f["shape"], origin=f["origin"][:n].copy(), dir=f["dir"][:n].copy(),
                tmax=np.full(n, 5.0), ray_body=np.full(n, -1, np.int32))

    def edit(key, at, value):
        a = dict(base)
        a[key] = np.array(base[key], copy=True)
        a[key][at] = value
        return a

    none = lambda key: {**base, key: None}
    side_bad = edit("side", 2, [0.2, 0.3, 0.2])             # body 2 is a sphere
    return {"nan_origin": edit("origin", (1, 0), np.nan), "inf_origin": edit("origin", (2, 2), np.inf),
            "nan_dir": edit("dir", (0, 1), np.nan), "inf_dir": edit("dir", (3, 0), -np.inf), "zero_dir": edit("dir", 2, 0.0),
            "negative_tmax": edit("tmax", 1, -1e-300), "nan_tmax": edit("tmax", 3, np.nan),
            "ray_body_high": edit("ray_body", 0, 12), "ray_body_low": edit("ray_body", 3, -2),
            "null_origin": none("origin"), "null_dir": none("dir"), "null_tmax": none("tmax"), "null_pos": none("pos"),
            "null_hit": {**base, "drop": 0}, "null_t": {**base, "drop": 1},
            "bad_shape": edit("shape", 5, 7), "bad_sphere_side": side_bad}


BAD = _bad_calls()


@pytest.mark.parametrize("what", sorted(BAD))
def test_refusals_leave_the_outputs_untouched(ctx, what):
    a = BAD[what]
    n = 4
    hit, t, normal = np.full(n, 77, np.int32), np.full(n, 7.5), np.full((n, 3), -3.25)
    outs = [hit, t, normal]
    keep = {k: np.ascontiguousarray(a[k], np.int32 if k in ("shape", "ray_body") else np.float64) if a[k] is not None else None
            for k in ("pos", "R", "side", "shape", "origin", "dir", "tmax", "ray_body")}
    p = {k: (None if v is None else v.ctypes.data_as(C.c_void_p)) for k, v in keep.items()}
    op = [x.ctypes.data_as(C.c_void_p) for x in outs]
    if "drop" in a:
        op[a["drop"]] = None
    st = capi.load().egs_cast_rays(ctx.h, C.c_int32(12), p["pos"], p["R"], p["side"], p["shape"], C.c_int32(n), p["ray_body"],
                                   p["origin"], p["dir"], p["tmax"], *op)
    assert st == capi.ERR_INVALID
    assert (hit == 77).all() and (t == 7.5).all() and (normal == -3.25).all()


def test_no_rays_is_ok_and_no_bodies_is_the_ground_alone(ctx):
    f = ref.family("heap")
    hit, t, normal = ctx.cast_rays(f["pos"], f["R"], f["side"], f["shape"], np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(hit) == 0 and len(t) == 0 and normal.shape == (0, 3)
    g = ref.family("ground")
    hit, t, normal = ctx.cast_rays(np.zeros((0, 3)), np.zeros((0, 9)), np.zeros((0, 3)), None, g["origin"], g["dir"])
    assert set(hit) == {-2, -1} and (t[hit == -2] == np.inf).all()
