"""CPU: the reference of the dense friction pyramid (dense_friction_reference.py) against the
mathematics, the conditions its seeded cases must meet under the reference alone, the numpy port behind the bounds, and
the argument checks of the capi wrapper that need no device."""
import numpy as np
import pytest

import dense_friction_reference as dfr
import friction_reference as fr
from eggshell_amd import capi


@pytest.mark.parametrize("cid", dfr.CASES)
def test_case_conditions_and_complementarity(cid):
    """Converges within max_outer = 32; delta keeps a factor 4 from tol on both sides of the stopping solve; every
    certification is strict (reference() raises otherwise); the final x satisfies the pyramid's complementarity at beta;
    the port, on the certified sets, makes the same number of solves and stands within the class's bound / 8."""
    c = dfr.case(cid)
    ref = dfr.solved(cid)
    assert ref.converged and ref.outer <= dfr.MAX_OUTER
    K, clear = dfr.gap_ok(ref.deltas)
    assert K == ref.outer - 1 and clear, ref.deltas
    assert len(ref.refs) == ref.outer
    assert dfr.complementarity(c.A, c.b, c.Ceq, c.nrow, c.mu, c.lo, c.hi, ref, dfr.TOL) == []
    # f of every pyramid row is a plain inequality row
    f = c.nrow[c.nrow >= 0]
    assert (c.Ceq[f] == 0).all() and (c.nrow[f] == -1).all()
    p = dfr.port(c.A, c.b, c.Ceq, c.lo, c.hi, c.nrow, c.mu, ref)
    ratio = dfr.x_ratio(ref, p.x)
    print("%s: n %d, %d solves, deltas %s, kappa %.3g, pinned %d, port ratio %.3g (C = %g)" %
          (cid, c.n, ref.outer, " ".join("%.2g" % d for d in ref.deltas), ref.refs[-1].kappa, int(ref.pinned.sum()), ratio, dfr.BOUNDS[c.cls]))
    assert p.outer == ref.outer and p.converged
    assert 8 * ratio <= dfr.BOUNDS[c.cls]


def test_the_cases_cover_every_row_state():
    """At least one case ends with pinned rows (a contact with x_n = 0), and at least one with rows at +beta, at -beta
    and strictly inside; the random sizes stand on both sides of the 32 / 64 / 112 edges."""
    pinned_at_zero_normal, all_three = [], []
    for cid in dfr.CASES:
        c, ref = dfr.case(cid), dfr.solved(cid)
        pyr = c.nrow >= 0
        if (ref.pinned & (ref.x[np.where(pyr, c.nrow, 0)] == 0)).any():
            pinned_at_zero_normal.append(cid)
        live = pyr & (ref.beta > 0)
        if (live & (ref.x == ref.beta)).any() and (live & (ref.x == -ref.beta)).any() and (live & (np.abs(ref.x) < ref.beta)).any():
            all_three.append(cid)
    assert pinned_at_zero_normal and all_three
    assert "joint-contact-mu0.5" in pinned_at_zero_normal          # equality rows and pinned rows together
    assert dfr.case("joint-contact-mu0.5").Ceq.any()
    assert dfr.RANDOM_SIZES == (3, 6, 30, 33, 63, 66, 111, 114)
    assert dfr.case("pile222-mu0.5").n == 96 and dfr.case("pile223-mu0.22").n == 144


@pytest.mark.parametrize("mu", [0.2, 0.8])
def test_cube_velocity_distance(mu):
    """The cube's velocity from the reference's lambda against the analytic Coulomb value: NOT zero, cfm 0.01 softens the
    contact.  Recorded: 2.913e-5 at mu 0.2, 7.260e-5 at mu 0.8; the mu = 0.8 cube is the slower."""
    c = dfr.case("cube-mu%g" % mu)
    ref = dfr.solved(c.id)
    v = dfr.velocity(c, ref.x)[0]
    dist = float(np.abs(v - fr.cube_velocity(mu)).max())
    print("cube mu %.1f: v = %s, distance from the analytic velocity %.4g" % (mu, v, dist))
    assert 0 < dist <= dfr.CUBE_DISTANCE[mu] * (1 + 1e-6)
    assert dist >= dfr.CUBE_DISTANCE[mu] * (1 - 1e-3)


def test_max_outer_two_does_not_converge():
    c = dfr.case(dfr.NOT_CONVERGED)
    ref = dfr.solved(c.id, 2)
    assert not ref.converged and ref.outer == 2 and ref.change > dfr.TOL
    full = dfr.solved(c.id)
    assert ref.deltas == full.deltas[:2]


def test_wrapper_argument_checks():
    c = dfr.case("rnd-n6")
    good = dict(ns=[6], A=c.A, b=c.b, C=c.Ceq, lo=c.lo, hi=c.hi, normal_row=c.nrow, mu=c.mu)
    out = capi.check_mixed_friction_batch(**good)
    assert out[6].dtype == np.int32 and out[7].dtype == np.float64 and out[0].dtype == np.int32
    for bad in (dict(normal_row=None), dict(mu=None), dict(normal_row=c.nrow[:5]), dict(mu=c.mu[:5]),
                dict(normal_row=c.nrow.astype(np.float64)), dict(max_outer=-1), dict(max_outer=1.5), dict(tol=-1.0),
                dict(tol=float("nan")), dict(ns=[5]), dict(A=None)):
        with pytest.raises(ValueError):
            capi.check_mixed_friction_batch(**{**good, **bad})
    assert "egs_mixed_friction_solve_batch" in capi.EXPORTS
