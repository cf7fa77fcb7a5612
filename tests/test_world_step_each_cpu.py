"""CPU: the per-ensemble world steps (egs_world_step_each / egs_world_step_dense_each) are part of the C ABI --
declared in the header, exported by the library, listed in capi.EXPORTS and reachable from capi.World -- and what
they refuse without a device: a NULL world, a rate table of the wrong length."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from eggshell_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_world_step_each", "egs_world_step_dense_each")


def test_header_declares_both_entries():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert name in capi.EXPORTS, name
    rates = r"\s*egs_world\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
    # w, n_ensembles, dt, erp, params, detect_contacts, stats
    assert re.search(r"\begs_status\s+egs_world_step_each\s*\(" + rates + r"\s*const\s+egs_solve_params\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s+\w+\s*,\s*egs_solve_stats\s*\*\s*\w+\s*\)", code)
    # w, n_ensembles, dt, erp, cfm_coeff, use_bounds, detect_contacts, n_failed
    assert re.search(r"\begs_status\s+egs_world_step_dense_each\s*\(" + rates + r"\s*double\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*int32_t\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)", code)


def test_library_exports_both_entries():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name


def test_null_world_is_refused_without_a_device():
    lib = capi.load()
    dt, erp = np.array([1e-3, 5e-3]), np.array([0.2, 0.2])
    prm = capi.params()
    assert lib.egs_world_step_each(None, C.c_int32(2), capi._p(dt), capi._p(erp), C.byref(prm), C.c_int32(1),
                                   None) == capi.ERR_INVALID
    nf = C.c_int32(7)
    assert lib.egs_world_step_dense_each(None, C.c_int32(2), capi._p(dt), capi._p(erp), C.c_double(0.01), C.c_int32(0),
                                         C.c_int32(1), C.byref(nf)) == capi.ERR_INVALID


class _NoLibrary:
    """Stands where the world's handle and context would: any use of it is a call that should not have been made."""

    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s)" % name)


def _world_without_a_device(n_ensembles):
    w = object.__new__(capi.World)
    w.ctx, w.h, w.n, w.n_ensembles = _NoLibrary(), None, 0, n_ensembles
    return w


@pytest.mark.parametrize("dt, erp", [([1e-3, 5e-3], 0.2), ([1e-3, 5e-3, 1e-3, 1e-3], 0.2), ([1e-3] * 3, [0.2, 0.2]),
                                     (1e-3, 0.2), ([[1e-3, 5e-3, 1e-3]], 0.2)])
def test_wrapper_refuses_a_wrong_length_before_the_library(dt, erp):
    w = _world_without_a_device(3)
    with pytest.raises(ValueError):
        w.step_each(dt, erp, capi.params())
    with pytest.raises(ValueError):
        w.step_dense_each(dt, erp)
    w.h = None   # (close() of the stub has nothing to destroy)


def test_wrapper_broadcasts_a_scalar_erp():
    w = _world_without_a_device(3)
    dt, erp = w._rates([1e-3, 0.0, 5e-3], 0.2)
    assert dt.dtype == np.float64 and erp.dtype == np.float64
    assert dt.tolist() == [1e-3, 0.0, 5e-3] and erp.tolist() == [0.2, 0.2, 0.2]
    dt, erp = w._rates((1e-3, 2e-3, 3e-3), (0.1, 0.2, 0.3))
    assert erp.tolist() == [0.1, 0.2, 0.3]
