"""CPU: which form takes the FACE launch (policy.h: face_form_policy, face_lds_bytes), read through the host-only entry
egs_debug_face_form.  The present kernels hold 252 .. 256 VGPRs and run four tiles per CU; the lean ones hold 168 and
run six, at a longer block.  The policy predicts both launches, each with the split of face_split_policy applied to its
own slot count (4 x CUs, 6 x CUs), and takes the shorter; at and below 4 x CUs tiles the present form stays.

  * the headline (24 C3 piles: 1 536 tiles, depth 64, period 8, 100 sweeps, 256 CUs) runs lean, unsplit, in one round;
  * tile counts at and below 4 x CUs keep the present form, whatever the sweeps;
  * for every tile count the decision is the smaller of the policy's own two predictions;
  * each form's split is face_split_policy's on that form's slots (egs_debug_face_split);
  * a lean tile asks for at most 26 KiB of LDS at six tiles per CU, and is refused (0) beyond that."""
import pytest

from eggshell_amd import capi

CUS, DEPTH, PERIOD = 256, 64, 8
LDS_MAX = 26 * 1024


def test_the_headline_runs_lean_in_one_round():
    f = capi.debug_face_form(1536, CUS, DEPTH, PERIOD, 100)
    assert f["lean"]
    assert f["split"][1] == (0, 0)                  # 1 536 tiles on 6 x 256 slots: nothing to split
    assert f["split"][0] == (512, 50)               # the present form would have split its half round
    assert 1536 <= 6 * CUS                          # one round
    assert f["us"][1] < f["us"][0]


@pytest.mark.parametrize("sweeps", [1, 2, 20, 50, 100, 400])
def test_up_to_four_tiles_per_cu_keep_the_present_form(sweeps):
    for n in (0, 1, 3, 255, 256, 512, 768, 1000, 1023, 1024):
        f = capi.debug_face_form(n, CUS, DEPTH, PERIOD, sweeps)
        assert not f["lean"], (n, sweeps)
    for cus, n in ((8, 32), (64, 256), (304, 1216)):
        assert not capi.debug_face_form(n, cus, DEPTH, PERIOD, sweeps)["lean"], (cus, n)


@pytest.mark.parametrize("sweeps", [1, 10, 50, 81, 100, 250])
def test_the_decision_is_the_smaller_prediction(sweeps):
    for cus in (8, 256):
        for n in list(range(0, 12 * cus + 2, max(cus // 8, 1))) + [4 * cus + 1, 6 * cus, 6 * cus + 1, 12 * cus + 1]:
            f = capi.debug_face_form(n, cus, DEPTH, PERIOD, sweeps)
            present, lean = f["us"]
            assert present >= 0 and lean >= 0
            assert f["lean"] == (lean < present), (cus, n, sweeps, f)
            for k, per_cu in enumerate((4, 6)):
                tiles, s1, _ = capi.debug_face_split(n, per_cu * cus, DEPTH, PERIOD, sweeps)
                assert f["split"][k] == (tiles, s1), (cus, n, sweeps, k)


def test_more_tiles_cost_no_less():
    """each form's prediction does not fall as tiles are added within a round, and a second round costs more"""
    for k, per_cu in enumerate((4, 6)):
        slots = per_cu * CUS
        one = capi.debug_face_form(slots, CUS, DEPTH, PERIOD, 100)["us"][k]
        assert capi.debug_face_form(1, CUS, DEPTH, PERIOD, 100)["us"][k] == one
        assert capi.debug_face_form(slots + 1, CUS, DEPTH, PERIOD, 100)["us"][k] > one
        assert capi.debug_face_form(2 * slots, CUS, DEPTH, PERIOD, 100)["us"][k] == pytest.approx(2 * one)


def test_a_lean_tile_asks_for_at_most_26_kib():
    seen_fit = seen_refused = False
    for slots in list(range(1, 700)):
        lds = capi.debug_face_form(1536, CUS, DEPTH, PERIOD, 100, max_slots=slots)["lds_bytes"]
        assert 0 <= lds <= LDS_MAX, slots
        if lds:
            # the accumulators and the parked values fit the request
            assert lds >= slots * 48 and not seen_refused, slots
            assert 6 * lds <= 160 * 1024
            seen_fit = True
        else:
            seen_refused = True
    assert seen_fit and seen_refused
    # a C3 pile's tile: four columns of sixteen boxes and the world
    assert capi.debug_face_form(1536, CUS, DEPTH, PERIOD, 100, max_slots=65)["lds_bytes"] > 0


def test_bad_arguments_are_refused():
    with pytest.raises(capi.EgsError):
        capi.debug_face_form(-1, CUS, DEPTH, PERIOD, 100)
    with pytest.raises(capi.EgsError):
        capi.debug_face_form(10, 0, DEPTH, PERIOD, 100)
