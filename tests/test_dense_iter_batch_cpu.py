"""CPU: the host side of the batched dense iteration (egs_dense_iterate_batch) -- packing and unpacking of ragged lists
with empty problems among them, the size checks of the binding, and the symbol in the header and in the built library."""
import os
import re

import numpy as np
import pytest

from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return ([rng.uniform(-1, 1, (n, n)) for n in sizes], [rng.uniform(-1, 1, n) for n in sizes],
            [rng.integers(0, 2, n).astype(bool) for n in sizes], [np.full(n, -0.5) for n in sizes], [np.full(n, 0.25) for n in sizes])


def test_symbol_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "egs_dense_iterate_batch" in re.findall(r"\b(egs_[a-z_0-9]+)\s*\(", text)
    assert "egs_dense_iterate_batch" in capi.EXPORTS
    assert hasattr(capi.load(), "egs_dense_iterate_batch")
    assert hasattr(capi.Context, "dense_iterate_batch") and hasattr(capi.Context, "dense_iterate_batch_packed")


def test_pack_and_unpack_ragged_lists():
    sizes = [0, 3, 1, 0, 5, 2]
    As, bs, Cs, los, his = ragged(sizes)
    ns, A, b, lo, hi = capi.pack_lcp_batch(As, bs, los, his)
    Cp = capi.pack_batch_vectors(ns, Cs, np.uint8, "C")
    assert list(ns) == sizes and ns.dtype == np.int32
    assert A.shape == (sum(n * n for n in sizes),) and b.shape == lo.shape == hi.shape == Cp.shape == (sum(sizes),)
    assert Cp.dtype == np.uint8
    vo, ao = capi.lcp_batch_offsets(ns)
    for k, n in enumerate(sizes):
        assert np.array_equal(A[ao[k]:ao[k + 1]].reshape(n, n), As[k])
        assert np.array_equal(b[vo[k]:vo[k + 1]], bs[k]) and np.array_equal(Cp[vo[k]:vo[k + 1]], Cs[k].astype(np.uint8))
    Al, bl, cl = capi.unpack_lcp_batch(ns, A, b, Cp)
    for k, n in enumerate(sizes):
        assert Al[k].shape == (n, n) and bl[k].shape == (n,) and cl[k].shape == (n,)
        assert np.array_equal(Al[k], As[k]) and np.array_equal(bl[k], bs[k])
    # what the call will hand to the C ABI
    ns2, A2, b2, C2, lo2, hi2 = capi.check_dense_iterate_batch(ns, A, b, Cp, lo, hi)
    assert ns2.dtype == np.int32 and A2.dtype == np.float64 and C2.dtype == np.uint8 and A2.flags.c_contiguous
    ns3, A3, b3, C3, lo3, hi3 = capi.check_dense_iterate_batch(ns, A, b)
    assert C3 is None and lo3 is None and hi3 is None
    # nothing at all, and nothing but empty problems
    ns0, A0, b0, lo0, hi0 = capi.pack_lcp_batch([], [], [], [])
    assert len(ns0) == 0 and A0.size == 0 and b0.size == 0
    capi.check_dense_iterate_batch(ns0, A0, b0)
    nsz, Az, bz, _, _ = capi.pack_lcp_batch([np.zeros((0, 0))] * 3, [np.zeros(0)] * 3, [], [])
    assert list(nsz) == [0, 0, 0] and Az.size == 0
    capi.check_dense_iterate_batch(nsz, Az, bz)


def test_size_checks_raise_value_error():
    sizes = [2, 0, 4]
    As, bs, Cs, los, his = ragged(sizes, 1)
    ns, A, b, lo, hi = capi.pack_lcp_batch(As, bs, los, his)
    Cp = capi.pack_batch_vectors(ns, Cs, np.uint8, "C")
    with pytest.raises(ValueError):
        capi.pack_lcp_batch(As[:2], bs, los, his)                       # a matrix short
    with pytest.raises(ValueError):
        capi.pack_lcp_batch([As[0], As[1], np.zeros((4, 3))], bs, los, his)   # not square
    with pytest.raises(ValueError):
        capi.pack_batch_vectors(ns, [Cs[0], Cs[1], Cs[2][:3]], np.uint8, "C")
    with pytest.raises(ValueError):
        capi.pack_batch_vectors(ns, Cs[:2], np.uint8, "C")
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch(ns, A[:-1], b)
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch(ns, A, b[:-1])
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch(ns, A, b, Cp, lo, None)           # C, lo and hi come together
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch(ns, A, b, Cp[:-1], lo, hi)
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch(ns, A, b, Cp, lo, hi[:-1])
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch([2.0, 0.0, 4.0], A, b)            # sizes are integers
    with pytest.raises(ValueError):
        capi.check_dense_iterate_batch([[2, 0, 4]], A, b)
