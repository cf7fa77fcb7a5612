"""CPU: the packed layout of the batched LCP entries (egs_box_lcp_batch, egs_box_lcp_schur_batch) as capi builds it --
problem k's matrix at sum_{j<k} n_j^2, its vectors at sum_{j<k} n_j -- round-trips for ragged sizes; no device and
no library needed.  The binding of the batched Schur entry is declared where the header declares it."""
import os
import re

import numpy as np
import pytest

from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_offsets_of_ragged_sizes():
    ns = [3, 1, 96, 7, 1, 20]
    vo, ao = capi.lcp_batch_offsets(ns)
    assert vo.dtype == np.int64 and ao.dtype == np.int64 and len(vo) == len(ns) + 1
    assert list(vo) == [0, 3, 4, 100, 107, 108, 128]
    assert list(ao) == [0, 9, 10, 9226, 9275, 9276, 9676]
    big = capi.lcp_batch_offsets([96] * 300000)[1]              # past 2^31 entries without wrapping
    assert big[-1] == 300000 * 96 * 96


def test_pack_and_unpack_round_trip():
    rng = np.random.default_rng(5)
    ns = [int(v) for v in rng.integers(1, 97, 37)] + [1, 96]
    As = [rng.uniform(-1, 1, (n, n)) for n in ns]
    bs, los, his = ([rng.uniform(-1, 1, n) for n in ns] for _ in range(3))
    pn, A, b, lo, hi = capi.pack_lcp_batch(As, bs, los, his)
    assert pn.dtype == np.int32 and list(pn) == ns
    assert A.dtype == np.float64 and A.size == sum(n * n for n in ns) and b.size == lo.size == hi.size == sum(ns)
    vo, ao = capi.lcp_batch_offsets(pn)
    for k, n in enumerate(ns):
        assert np.array_equal(A[ao[k]:ao[k] + n * n].reshape(n, n), As[k])      # row-major, back to back
        assert np.array_equal(b[vo[k]:vo[k] + n], bs[k]) and np.array_equal(lo[vo[k]:vo[k] + n], los[k])
    A2, b2, lo2, hi2 = capi.unpack_lcp_batch(pn, A, b, lo, hi)
    for k in range(len(ns)):
        assert np.array_equal(A2[k], As[k]) and np.array_equal(b2[k], bs[k]) and np.array_equal(lo2[k], los[k]) and np.array_equal(hi2[k], his[k])
    A2[3][0, 0] = 123.0                                          # views: what the library writes in place is what is returned
    assert A[ao[3]] == 123.0
    (only_b,) = capi.unpack_lcp_batch(pn, None, b)
    assert all(np.array_equal(u, v) for u, v in zip(only_b, bs))


def test_pack_refuses_a_matrix_of_the_wrong_size():
    with pytest.raises(ValueError):
        capi.pack_lcp_batch([np.zeros((3, 3)), np.zeros((2, 3))], [np.zeros(3), np.zeros(2)], [np.zeros(3), np.zeros(2)], [np.zeros(3), np.zeros(2)])


def test_empty_batch_packs():
    ns, A, b, lo, hi = capi.pack_lcp_batch([], [], [], [])
    assert len(ns) == 0 and A.size == b.size == lo.size == hi.size == 0
    assert capi.unpack_lcp_batch(ns, A, b) == [[], []]


def test_batched_schur_entry_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    m = re.search(r"egs_status\s+egs_box_lcp_schur_batch\s*\(([^;]*)\)\s*;", header)
    assert m, "include/eggshell_amd.h does not declare egs_box_lcp_schur_batch"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 18 and args[0].startswith("egs_context") and "nub" in args[8] and args[8].startswith("const int32_t")
    assert "egs_box_lcp_schur_batch" in capi.EXPORTS
    assert callable(getattr(capi.Context, "box_lcp_schur_batch")) and callable(getattr(capi.Context, "box_lcp_schur_batch_packed"))
