"""GPU (-m gpu): Lcp::MixedConstraintsSolverBatch of the reference-shaped C++ API (eggshell_amd/host) against eight
calls of Lcp::MixedConstraintsSolver on the same problems, driven by `mixed_batch_demo`: the same ok for every problem,
x and w within 1e-8 * scale (bits are not required: the single call takes the multi-launch path), and the problems,
rebuilt here, are solved."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "mixed_batch_demo")
SIZES = (1, 6, 12, 20, 33, 48, 64, 96)


@pytest.fixture(scope="module")
def out():
    if not os.path.exists(DEMO):
        pytest.fail("mixed_batch_demo is not built: run __graft_entry__.build()")
    txt = subprocess.run([DEMO], check=True, capture_output=True, text=True, timeout=600).stdout
    res = {}
    for line in txt.splitlines():
        k, *v = line.split()
        res[k] = np.array([float(t) for t in v])
    return res


def test_batch_agrees_with_eight_single_calls(out):
    for k, n in enumerate(SIZES):
        assert out["ok_batch%d" % k][0] == 1 and out["ok_single%d" % k][0] == 1, k
        xb, xs, wb, ws = (out["%s_%s%d" % (v, how, k)] for v in "xw" for how in ("batch", "single"))
        assert xb.shape == (n,) and wb.shape == (n,) and np.all(np.isfinite(xb)) and np.all(np.isfinite(wb)), k
        scale = max(1.0, np.abs(xs).max())
        assert np.abs(xb - xs).max() <= 1e-8 * scale and np.abs(wb - ws).max() <= 1e-8 * scale, k


def test_a_mismatched_argument_is_refused(out):
    assert out["refused"][0] == 1      # EGS_ERR_INVALID


def test_the_problems_are_solved(out):
    """the demo's matrices, rebuilt here: A x = b + w, w = 0 on the equality rows, x >= 0 and w >= 0 on the others"""
    for k, m in enumerate(SIZES):
        i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
        a, c = np.minimum(i, j), np.maximum(i, j)
        A = ((a * 31 + c * 17 + (a * c) % 11 + 7 * k) % 23 - 11) / 11.0
        A[np.diag_indices(m)] = 0.0
        A[np.diag_indices(m)] = 1.5 * np.abs(A).sum(1) + 1.0 + 0.125 * (np.arange(m) % 5)
        b = ((np.arange(m) * 13 + k) % 11 - 5) * 0.3
        eq = (np.arange(m) + k) % 3 != 0
        x, w = out["x_batch%d" % k], out["w_batch%d" % k]
        assert np.linalg.norm(A @ x - b - w) < 1e-9, k
        assert (w[eq] == 0).all() and (x[~eq] >= 0).all() and (w[~eq] >= -1e-9).all(), k
