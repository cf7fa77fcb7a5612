"""GPU (-m gpu): Ensemble::SetWarmStart / EnsembleGroup of the reference-shaped C++ API (eggshell_amd/host), driven by
`frame_demo --warm`: the frame of tests/test_gpu_adapter_group.py with warm start on every Ensemble -- the group's
batched world against the separate Ensembles' worlds, bit for bit -- and a cold copy that the warm run must leave."""
import pytest

from test_gpu_adapter_group import FRAMES, SEED, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def out():
    return run("--warm", str(FRAMES + 3), str(SEED))


def test_warm_group_equals_warm_separate_steps_bit_for_bit(out):
    print(out)
    assert out["frames"] == FRAMES + 3
    assert out["max_abs_diff"] == 0.0
    assert out["cairn_contacts_group"] == out["cairn_contacts_separate"]
    assert out["worlds_created"] == 1 and out["world_ensembles"] == 2


def test_the_history_is_in_use(out):
    """The adapter does not push an untouched state again, so the world keeps its history: from the second frame with
    contacts on, the cairn's solve starts from the previous lambda and leaves the cold run."""
    assert max(out["cairn_contacts_group"]) > 0
    assert out["differs_from_cold"] > 0


def test_members_that_differ_in_warm_start_are_refused():
    res = run("--warm-mismatch")
    assert res["refused"] == 1       # EGS_ERR_INVALID
    assert "member 1" in res["message"] and "SetWarmStart" in res["message"]
