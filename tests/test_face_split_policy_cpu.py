"""CPU: the policy that splits the FACE launch in time (policy.h: face_split_policy, face_piece_list), through the host
entry egs_debug_face_split.  With n_tiles = k x slots + R, 0 < R <= slots / 2, R tiles run as two workgroups, sweeps
1 .. s1 and s1 + 1 .. S, so that a resident slot runs either a first part and then a whole tile or a whole tile and then
a second part; s1 balances the two.  The work list is taken in order (by ticket), so a first part stands before its
second part."""
import numpy as np
import pytest

from eggshell_amd import capi

DEPTH, P = 64, 8   # the timetable of a C3 pile's tile
WHOLE, FIRST, SECOND = 0, 1, 2


def steps_fresh(depth, period, sweeps):
    """timetable_end of a fresh launch: the accumulation and `sweeps` sweeps"""
    return depth + period * sweeps


def steps_resumed(depth, period, sweeps):
    return depth + period * (sweeps - 1)


def check_list(pieces, n_tiles, H, s1, S):
    assert pieces.shape == (n_tiles + H, 4)
    tile, resume, sweeps, kind = pieces.T
    seen_whole = np.bincount(tile[kind == WHOLE], minlength=n_tiles)
    seen_first = np.bincount(tile[kind == FIRST], minlength=n_tiles)
    seen_second = np.bincount(tile[kind == SECOND], minlength=n_tiles)
    # every tile once whole or once as a (first, second) pair
    assert ((seen_whole == 1) & (seen_first == 0) & (seen_second == 0) |
            (seen_whole == 0) & (seen_first == 1) & (seen_second == 1)).all()
    assert seen_first.sum() == H and (tile >= 0).all() and (tile < n_tiles).all()
    # the split tiles are the last H
    assert set(tile[kind == FIRST]) == set(range(n_tiles - H, n_tiles))
    assert (resume == (kind == SECOND)).all()
    assert (sweeps[kind == WHOLE] == S).all() and (sweeps[kind == FIRST] == s1).all() and (sweeps[kind == SECOND] == S - s1).all()
    if H:
        assert 1 <= s1 <= S - 1
    where = {(int(t), int(k)): i for i, (t, k) in enumerate(zip(tile, kind))}
    for t in range(n_tiles - H, n_tiles):
        assert where[(t, FIRST)] < where[(t, SECOND)]
        assert sweeps[where[(t, FIRST)]] + sweeps[where[(t, SECOND)]] == S


def test_the_headline_splits_a_third_of_its_tiles_in_the_middle():
    H, s1, pieces = capi.debug_face_split(1536, 1024, DEPTH, P, 100)
    assert H == 512 and s1 in (49, 50)
    check_list(pieces, 1536, H, s1, 100)
    first_then_whole = steps_fresh(DEPTH, P, s1) + steps_fresh(DEPTH, P, 100)
    whole_then_second = steps_fresh(DEPTH, P, 100) + steps_resumed(DEPTH, P, 100 - s1)
    assert abs(first_then_whole - whole_then_second) <= P
    # the first 1 024 pieces fill the slots: the 512 first parts and 512 whole tiles, evenly mixed; the remaining whole
    # tiles follow, the second parts come last
    kind = pieces[:, 3]
    assert (kind[:1024] == FIRST).sum() == 512 and (kind[:1024] == WHOLE).sum() == 512
    assert np.abs(np.cumsum(kind[:1024] == FIRST) - np.arange(1, 1025) / 2).max() <= 1
    assert (kind[1024:1536] == WHOLE).all() and (kind[1536:] == SECOND).all()


@pytest.mark.parametrize("n_tiles,sweeps", [(1024, 100), (768, 100), (1600, 100), (1536, 1), (1536, 2), (2048, 100), (512, 100),
                                            (0, 100), (1, 100)])
def test_no_split(n_tiles, sweeps):
    """exact multiples of the slots, fewer tiles than slots, a remainder above half of the slots, low sweep counts"""
    H, s1, pieces = capi.debug_face_split(n_tiles, 1024, DEPTH, P, sweeps)
    assert (H, s1) == (0, 0)
    check_list(pieces, n_tiles, 0, 0, sweeps)
    assert (pieces[:, 0] == np.arange(n_tiles)).all()


def test_a_small_remainder():
    H, s1, pieces = capi.debug_face_split(1100, 1024, DEPTH, P, 100)
    assert H == 76 and s1 in (49, 50)
    check_list(pieces, 1100, H, s1, 100)
    kind = pieces[:, 3]
    assert (kind[:1024] == FIRST).sum() == 76 and (kind[1024:1100] == WHOLE).all() and (kind[1100:] == SECOND).all()


def test_a_full_round_comes_first():
    H, s1, pieces = capi.debug_face_split(2560, 1024, DEPTH, P, 100)
    assert H == 512 and s1 in (49, 50)
    check_list(pieces, 2560, H, s1, 100)
    assert (pieces[:1024, 3] == WHOLE).all() and (pieces[:1024, 0] == np.arange(1024)).all()
    assert (pieces[1024:2048, 3] == FIRST).sum() == 512 and (pieces[2560:, 3] == SECOND).all()


def test_the_saving_must_pay_for_the_second_fill_and_prologue():
    """The split saves P (S - s1) steps per slot and adds the fill (depth) and a prologue: it starts where the former
    exceeds the latter, and stays from there on."""
    answers = [capi.debug_face_split(1536, 1024, DEPTH, P, S)[0] for S in range(1, 201)]
    first = answers.index(512)
    assert answers[:first] == [0] * first and answers[first:] == [512] * (200 - first)
    S = first + 1
    assert P * (S - S // 2) > DEPTH                              # more than the fill alone
    assert 20 <= S <= 100                                        # ... and on well before the headline's 100 sweeps
    # a deeper timetable needs more sweeps
    assert capi.debug_face_split(1536, 1024, 4 * DEPTH, P, S)[0] == 0


@pytest.mark.parametrize("n_tiles,h,S,s1", [(3, 3, 9, 4), (3, 1, 9, 1), (3, 2, 10, 9), (3, 50, 2, 1), (1, 1, 3, 2), (2048, 100, 100, 30)])
def test_force(n_tiles, h, S, s1):
    H, cut, pieces = capi.debug_face_split(n_tiles, 1024, DEPTH, P, S, force=(h, s1))
    assert H == min(h, n_tiles) and cut == s1
    check_list(pieces, n_tiles, H, s1, S)


@pytest.mark.parametrize("S,s1", [(1, 1), (1, 0), (9, 0), (9, 9), (9, 12), (9, -1)])
def test_force_without_a_cut_inside_the_sweeps_is_no_split(S, s1):
    H, cut, pieces = capi.debug_face_split(3, 1024, DEPTH, P, S, force=(3, s1))
    assert (H, cut) == (0, 0)
    check_list(pieces, 3, 0, 0, S)
    H, _, _ = capi.debug_face_split(3, 1024, DEPTH, P, 9, force=(0, 4))
    assert H == 0
