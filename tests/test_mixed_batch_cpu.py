"""CPU: the host side of the batched mixed LCP (egs_mixed_constraints_solve_batch) -- the declaration in the header, the
export list, the Python methods, the argument check of the packed layout, and the C++ adapter's declaration.  No GPU."""
import os
import re

import numpy as np
import pytest

from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_with_14_arguments():
    header = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    m = re.search(r"egs_status\s+egs_mixed_constraints_solve_batch\s*\(([^;]*)\)\s*;", header)
    assert m, "include/eggshell_amd.h does not declare egs_mixed_constraints_solve_batch"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14, args
    names = [re.sub(r"/\*.*?\*/", "", a).split()[-1].lstrip("*") for a in args]
    assert names == ["ctx", "count", "n", "A", "b", "C", "lo", "hi", "use_bounds", "max_pivots", "x", "w", "ok", "pivots"]


def test_entry_is_exported_and_bound():
    assert "egs_mixed_constraints_solve_batch" in capi.EXPORTS
    lib = capi.load()
    assert hasattr(lib, "egs_mixed_constraints_solve_batch")
    assert len(lib.egs_mixed_constraints_solve_batch.argtypes) == 14
    assert callable(getattr(capi.Context, "mixed_constraints_solve_batch"))
    assert callable(getattr(capi.Context, "mixed_constraints_solve_batch_packed"))


def packed(sizes, seed=0):
    rng = np.random.default_rng(seed)
    tot = sum(sizes)
    return (np.array(sizes, np.int32), rng.uniform(-1, 1, sum(n * n for n in sizes)), rng.uniform(-1, 1, tot),
            rng.integers(0, 2, tot).astype(np.uint8), np.zeros(tot), np.full(tot, np.inf))


def test_check_mixed_batch_accepts_a_ragged_layout():
    ns, A, b, Cp, lo, hi = packed([2, 0, 4, 1])
    ns2, A2, b2, C2, lo2, hi2 = capi.check_mixed_batch(list(ns), A, b, Cp.astype(bool), lo, hi)
    assert ns2.dtype == np.int32 and C2.dtype == np.uint8 and A2.dtype == np.float64
    assert np.array_equal(ns2, ns) and np.array_equal(A2, A) and np.array_equal(C2, Cp) and np.array_equal(hi2, hi)
    empty = capi.check_mixed_batch([], np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), np.zeros(0), np.zeros(0))
    assert empty[0].size == 0 and empty[1].size == 0
    capi.check_mixed_batch([0, 0], np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), np.zeros(0), np.zeros(0))


def test_check_mixed_batch_refuses_mismatched_arrays():
    ns, A, b, Cp, lo, hi = packed([2, 0, 4, 1])
    for bad in ((ns, A[:-1], b, Cp, lo, hi), (ns, A, b[:-1], Cp, lo, hi), (ns, A, b, Cp[:-1], lo, hi), (ns, A, b, Cp, lo[:-1], hi),
                (ns, A, b, Cp, lo, hi[:-1]), (ns, A, b, None, lo, hi), (ns, A, b, Cp, lo, None), (ns[:-1], A, b, Cp, lo, hi),
                ([2.0, 0.0, 4.0, 1.0], A, b, Cp, lo, hi), ([[2, 0, 4, 1]], A, b, Cp, lo, hi)):
        with pytest.raises(ValueError):
            capi.check_mixed_batch(*bad)


def test_list_form_refuses_ragged_lists_before_any_library_call():
    """Context.mixed_constraints_solve_batch packs before it calls: a context that was never created is enough."""
    ctx = object.__new__(capi.Context)
    As, bs = [np.eye(2), np.eye(3)], [np.ones(2), np.ones(3)]
    Cs, los, his = [np.zeros(2, np.uint8), np.zeros(3, np.uint8)], [np.zeros(2), np.zeros(3)], [np.ones(2), np.ones(3)]
    for bad in ((As[:1], bs, Cs, los, his), (As, bs, Cs[:1], los, his), (As, bs, Cs, los[:1], his), (As, bs, Cs, los, his[:1]),
                ([np.eye(2), np.eye(2)], bs, Cs, los, his), (As, bs, [Cs[0], Cs[0]], los, his), (As, bs, Cs, los, [his[1], his[1]])):
        with pytest.raises(ValueError):
            capi.Context.mixed_constraints_solve_batch(ctx, *bad)


def test_adapter_declares_the_batch_function():
    api = open(os.path.join(ROOT, "eggshell_amd", "host", "eggshell_api.h")).read()
    m = re.search(r"namespace Lcp \{(.*?)\n\}", api, re.S)
    assert m and re.search(r"std::vector<bool>\s+MixedConstraintsSolverBatch\s*\(", m.group(1))
    assert re.search(r"\bMixedConstraintsSolver\s*\(", m.group(1))
    mk = open(os.path.join(ROOT, "eggshell_amd", "host", "Makefile")).read()
    assert "mixed_batch_demo" in mk.split("all:")[1].splitlines()[0]
