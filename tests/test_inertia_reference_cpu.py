"""CPU: the oracle's minv_blocks / external_force -- the functions the device's live-inertia refresh is bit-equal to --
against the 40-digit statement of tests/inertia_reference.py, on its seeded families: kappa(I_b) from 1 to a thin rod's
1250, diagonal and full symmetric I_b, spins 0, 1e-170, 1, 50 and 1400 rad/s, R up to 1e-6 off orthonormal.

The bounds are in units of kappa(I_b) * u (u = 2^-53).  Measured over the 240 cases: the inverse 3.30, the torque 1.22;
the bounds are four times that, rounded up -- their job is to catch a wrong formula (R^T I R for R I R^T is off by
1e15 units), not a rounding."""
import numpy as np
import pytest

import inertia_reference as ir
from oracle import oracle as orc

INVERSE_BOUND = 14.0
TORQUE_BOUND = 5.0


@pytest.fixture(scope="module")
def measured():
    cases = ir.families()
    R = np.array([c[0] for c in cases]); I = np.array([c[1] for c in cases]); w = np.array([c[2] for c in cases])
    mass = np.ones(len(cases))
    M = orc.minv_blocks(R, mass, I)
    f = orc.external_force(R, w, mass, I)
    return cases, M, f, [ir.errors(*cases[k], M[k], f[k, 3:]) for k in range(len(cases))]


def test_families_cover_the_ground(measured):
    cases = measured[0]
    kappa = [np.linalg.cond(c[1].reshape(3, 3)) for c in cases]
    assert min(kappa) < 1.0 + 1e-9 and max(kappa) > 1250.0
    assert any(c[1][1] != 0 for c in cases) and any(c[1][1] == 0 for c in cases)          # full and diagonal I_b
    big = lambda w: np.abs(w).max()      # (1e-170 squared underflows: the norm through the largest component)
    spins = sorted({float("%.3g" % (big(c[2]) * np.linalg.norm(c[2] / big(c[2])) if big(c[2]) > 0 else 0.0)) for c in cases})
    assert spins == sorted(ir.SPINS)
    ortho = [np.abs(c[0].reshape(3, 3) @ c[0].reshape(3, 3).T - np.eye(3)).max() for c in cases]
    assert min(ortho) < 1e-15 and 1e-7 < max(ortho) < 1e-5


def test_inverse_inertia_against_40_digits(measured):
    worst = max(e[0] for e in measured[3])
    print("inverse: worst %.3f kappa u" % worst)
    assert worst <= INVERSE_BOUND


def test_gyroscopic_torque_against_40_digits(measured):
    worst = max(e[1] for e in measured[3])
    print("torque: worst %.3f kappa u" % worst)
    assert worst <= TORQUE_BOUND


def test_no_spin_no_torque(measured):
    cases, _, f, errs = measured
    for k, c in enumerate(cases):
        if np.linalg.norm(c[2]) < 1e-100:      # 0 and 1e-170: the exact torque is below the smallest subnormal
            assert errs[k][2] and (f[k, 3:] == 0).all()


def test_linear_rows_are_mass_and_gravity(measured):
    _, M, f, _ = measured
    blocks = M.reshape(-1, 6, 6)
    assert (blocks[:, :3, :3] == np.eye(3)).all() and (blocks[:, :3, 3:] == 0).all() and (blocks[:, 3:, :3] == 0).all()
    assert (f[:, :2] == 0).all() and (f[:, 2] == -9.8).all()


def test_the_bound_catches_a_wrong_formula(measured):
    """R^T I_b R instead of R I_b R^T: far outside the bound on every body with a rotated, non-spherical inertia."""
    cases = measured[0]
    pick = [k for k, c in enumerate(cases) if np.linalg.cond(c[1].reshape(3, 3)) > 2][:12]
    Rt = np.array([cases[k][0].reshape(3, 3).T.reshape(9) for k in pick])
    I = np.array([cases[k][1] for k in pick])
    wrong = orc.minv_blocks(Rt, np.ones(len(pick)), I)
    for j, k in enumerate(pick):
        assert ir.errors(*cases[k], wrong[j], np.zeros(3))[0] > 1e6 * INVERSE_BOUND
