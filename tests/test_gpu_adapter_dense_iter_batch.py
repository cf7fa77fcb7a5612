"""GPU (-m gpu): sparse::{Jacobi,GaussSeidel,SOR}IterationBatch of the reference-shaped C++ API (eggshell_amd/host)
against eight calls of the single functions on the same systems, driven by `dense_iter_batch_demo`: for every method,
both argument forms and every system the batch returns the bits of the single call, and the systems are solved."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEMO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eggshell_amd", "host", "dense_iter_batch_demo")
SIZES = (1, 6, 12, 20, 33, 48, 64, 96)


@pytest.fixture(scope="module")
def out():
    if not os.path.exists(DEMO):
        pytest.fail("dense_iter_batch_demo is not built: run __graft_entry__.build()")
    txt = subprocess.run([DEMO], check=True, capture_output=True, text=True, timeout=600).stdout
    res = {}
    for line in txt.splitlines():
        k, *v = line.split()
        res[k] = np.array([float(t) for t in v])
    return res


@pytest.mark.parametrize("method", ["jacobi", "gs", "sor"])
@pytest.mark.parametrize("form", ["eq", "mixed"])
def test_batch_equals_eight_single_calls(out, method, form):
    for k, n in enumerate(SIZES):
        xb, xs = out["%s_%s_batch%d" % (method, form, k)], out["%s_%s_single%d" % (method, form, k)]
        assert xb.shape == (n,) and np.all(np.isfinite(xb)), k
        assert np.array_equal(xb, xs), k


def test_the_systems_are_solved(out):
    """the demo's matrices, rebuilt here: the 2-argument results solve A x = b to the reference's tolerance"""
    for k, m in enumerate(SIZES):
        i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
        a, c = np.minimum(i, j), np.maximum(i, j)
        A = ((a * 31 + c * 17 + (a * c) % 11 + 7 * k) % 23 - 11) / 11.0
        A[np.diag_indices(m)] = 0.0
        A[np.diag_indices(m)] = 1.5 * np.abs(A).sum(1) + 1.0 + 0.125 * (np.arange(m) % 5)
        b = ((np.arange(m) * 13 + k) % 11 - 5) * 0.3
        for method in ("jacobi", "gs", "sor"):
            assert np.linalg.norm(A @ out["%s_eq_batch%d" % (method, k)] - b) < 1e-8, (method, k)
