"""GPU (-m gpu): EnsembleGroup of the reference-shaped C++ API (eggshell_amd/host): the reference's frame (model.cc:37-70,
the chain stepped with kSimTimeStep and the cairn with kSimTimeStep * 5) through ONE batched world, driven by
`frame_demo`: three frames of group.Step({1e-3, 5e-3}) + 4 x group.Step({1e-3, 0}) against chain.Step(1e-3) x 5 and
cairn.Step(5e-3) on an identically seeded second copy.  The two runs must agree bit for bit."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "frame_demo")
FRAMES = 3
SEED = 24   # a cairn whose rocks touch after InitStabilize: 7 contacts in every frame (seed 1 has none: the rocks start apart)


def run(*args):
    if not os.path.exists(DEMO):
        pytest.fail("frame_demo is not built: run __graft_entry__.build()")
    p = subprocess.run([DEMO, *args], check=True, capture_output=True, text=True, timeout=600)
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def out():
    return run(str(FRAMES), str(SEED))


def test_group_frame_equals_separate_steps_bit_for_bit(out):
    print(out)
    assert out["frames"] == FRAMES
    assert out["max_abs_diff"] == 0.0
    assert out["chain_contacts_group"] == out["chain_contacts_separate"]
    assert out["cairn_contacts_group"] == out["cairn_contacts_separate"]
    assert len(out["cairn_contacts_group"]) == FRAMES


def test_the_cairn_has_contacts(out):
    assert max(out["cairn_contacts_group"]) > 0, out["cairn_contacts_group"]


def test_the_group_made_one_batched_world(out):
    assert out["worlds_created"] == 1
    assert out["world_ensembles"] == 2


def test_members_that_differ_are_refused():
    res = run("--mismatch")          # exit status 0: the refusal is EGS_ERR_INVALID
    assert res["refused"] == 1       # EGS_ERR_INVALID
    assert "member 1" in res["message"] and "cfm_coeff" in res["message"]
