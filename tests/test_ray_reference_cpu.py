"""CPU: the fp64 twin of the ray cast (ray_twin.py) against the 50-digit reference (ray_reference.py) on the seeded
families, and the three ray entries declared, exported and reachable.  No GPU."""
import os
import re

import numpy as np
import pytest

import ray_reference as ref
import ray_twin as twin
from collision_reference import TOL
from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("egs_cast_rays", "egs_world_set_rays", "egs_world_cast_rays")


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_reference_decides_the_family(name):
    """The cap on cases left out, on the reference alone: before any twin or device result is compared."""
    f = ref.family(name)
    assert len(f["origin"]) == (256 if name == "heap" else 64)
    assert ref.left_out(name) <= ref.MAX_LEFT_OUT[name]
    kinds = {r[0] for r in ref.family_reference(name)}
    assert "hit" in kinds and (name in ("heap",) or len(kinds - {None}) >= 2)


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_twin_agrees_with_the_reference(name):
    f = ref.family(name)
    got = twin.cast(f["pos"], f["R"], f["side"], f["shape"], f["origin"], f["dir"], f["tmax"])
    worst, left_out = ref.check_family(name, *got)
    print("%s: twin worst error %.3g (recorded %.3g, bound %.3g), left out %d" % (name, worst, ref.MEASURED[name],
                                                                               ref.BOUND[name], left_out))
    assert worst <= ref.BOUND[name]
    # the bound's own rule: TOL where the recorded worst is at most a quarter of it, else 4 x the recorded worst
    assert ref.BOUND[name] == (TOL if ref.MEASURED[name] <= TOL / 4 else 4 * ref.MEASURED[name])
    assert worst <= 1.5 * ref.MEASURED[name]          # the record is the measurement, not a guess


def test_families_hold_what_they_are_meant_to():
    g = ref.family("ground")
    assert (g["dir"][16:32, 2] == 0.0).all() and (g["origin"][48:, 2] < 0).all()
    b = ref.family("box")
    zero = (b["dir"][36:52] == 0.0).sum(axis=1)
    assert (zero[:8] == 1).all() and (zero[8:] == 2).all()
    c = ref.family("capsule")
    assert (c["dir"][40:48, :2] == 0.0).all()
    refs = ref.family_reference("ties")
    assert all(r[:2] == ("hit", 0) for r in refs[:16])                  # the lowest index of the twin spheres
    assert all(r[:2] == ("hit", -1) and r[2] == 0 for r in refs[16:32])  # the ground at the touching point
    assert all(refs[k][0] == ("hit" if k % 2 else "miss") for k in range(32, 64))
    s = ref.family_reference("sphere")
    assert {r[0] for r in s[48:]} == {"hit"} and {r[1] >= 0 for r in s[48:]} == {True, False}   # grazing: both sides


def test_attached_rays_and_ensembles_in_the_twin():
    f = ref.family("heap")
    k = 4
    o, d = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]]), np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    hit, t, n = twin.cast(f["pos"], f["R"], f["side"], f["shape"], o, d, [np.inf, np.inf], ray_body=[k, k])
    assert (hit != k).all()
    for i in range(2):
        ow, dw = twin.world_frame(f["pos"][k], f["R"][k], o[i], d[i])
        assert twin.cast_one(f["pos"], f["R"], f["side"], f["shape"], ow, dw, np.inf, skip=k) == (hit[i], t[i], list(n[i]))
    # two ensembles: a ray sees its own bodies only
    off = [0, 6, 12]
    a = twin.cast(f["pos"], f["R"], f["side"], f["shape"], f["origin"][:8], f["dir"][:8], f["tmax"][:8], ray_ens=[1] * 8, body_off=off)
    b = twin.cast(f["pos"][6:], f["R"][6:], f["side"][6:], f["shape"][6:], f["origin"][:8], f["dir"][:8], f["tmax"][:8])
    assert np.array_equal(np.where(a[0] >= 0, a[0] - 6, a[0]), b[0]) and a[1].tobytes() == b[1].tobytes()


def test_entries_are_declared_exported_and_reachable():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared in eggshell_amd.h"
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name + " is not exported by libeggshell_amd.so"
    assert callable(capi.Context.cast_rays) and callable(capi.World.set_rays) and callable(capi.World.cast_rays)
