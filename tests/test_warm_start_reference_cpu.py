"""CPU: what a start taken from the previous step's lambda buys on a resting stack, with the project's own pieces
(oracle assembly, rhs and integration, the oracle's collision, a dense numpy PGS): tests/warm_start_reference.py.
Three 0.3 cubes, dt 0.005, erp 0.2, cfm 0.01, 16 steps, 12 contacts; the reference's stopping rule (tol 1e-9) never
fires on the stack, so a cold solve pays its sweep cap on every step."""
import numpy as np

import warm_start_reference as wsr
from oracle import oracle as orc
from test_gpu_collide import reference_contacts

STEPS = 16


def run(warm, method, sweeps, tol):
    p, R = wsr.stack_scene()
    return wsr.step_loop(reference_contacts, p, R, STEPS, warm, method, sweeps, tol=tol)


def test_matcher_rule_on_a_hand_made_list():
    b0 = np.array([-1, -1, 0, 0], np.int32); b1 = np.array([0, 0, 1, 1], np.int32)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], np.float64)
    lam = np.arange(12, dtype=np.float64) + 1
    nb0 = np.array([-1, 0, 0, 0], np.int32); nb1 = np.array([0, 1, 1, 2], np.int32)
    npos = np.array([[0.9, 0, 0], [0.5, 0, 1], [5, 0, 1], [0, 0, 1]], np.float64)
    rhs = -np.ones(12)
    x0, src = wsr.match_contacts(b0, b1, pos, lam, [0, 4], [1], nb0, nb1, npos, rhs, [0, 4], 0.6)
    assert src.tolist() == [1, 2, -1, -1]          # nearest; a tie goes to the lowest index; too far; no such pair
    assert np.array_equal(x0, np.concatenate([lam[3:6], lam[6:9], np.zeros(6)]))
    x0, src = wsr.match_contacts(b0, b1, pos, lam, [0, 4], [0], nb0, nb1, npos, rhs, [0, 4], 0.6)
    assert src.tolist() == [-2] * 4 and np.array_equal(x0, rhs)


def test_pgs_from_rhs_is_the_default_start():
    from helpers import dense_numpy, numpy_pgs, random_system
    rng = np.random.default_rng(7)
    s, rhs = random_system(rng, 5, 9)
    A, _, _ = dense_numpy(s, 0.05)
    for method in (0, 1, 2):
        x, it = wsr.pgs(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 4)
        assert it == 4 and np.array_equal(x, numpy_pgs(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 4))
        x2, _ = wsr.pgs(A, rhs, s.is_eq, s.lo, s.hi, method, 1.5, 4, x0=rhs)
        assert np.array_equal(x, x2)
    assert abs(wsr.residual(A, rhs, x, s.is_eq, s.lo, s.hi) - orc.lit_residual(s, rhs, x, 0.05)) < 1e-9


def test_warm_sor_ends_far_closer_than_cold_at_the_sweep_cap():
    cold, warm = run(False, orc.SOR, 500, 1e-9), run(True, orc.SOR, 500, 1e-9)
    assert cold[-1][3] == 12 and warm[-1][3] == 12
    assert cold[-1][2] == 500 and warm[-1][2] == 500       # the cap is hit either way
    print("SOR 500, step 16: cold %.3g warm %.3g; residual of x0: cold %.3g warm %.3g" %
          (cold[-1][1], warm[-1][1], cold[-1][0], warm[-1][0]))
    assert warm[-1][1] <= 0.1 * cold[-1][1]


def test_warm_gs_after_twenty_sweeps():
    cold, warm = run(False, orc.GAUSS_SEIDEL, 20, 0.0), run(True, orc.GAUSS_SEIDEL, 20, 0.0)      # exactly 20 sweeps a step
    mc, mw = (np.median([r[1] for r in o[5:STEPS]]) for o in (cold, warm))     # steps 6 .. 16
    print("GS 20, median of steps 6..16: cold %.3g warm %.3g" % (mc, mw))
    assert mw <= 0.5 * mc
