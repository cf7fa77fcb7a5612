"""GPU (-m gpu): object life cycle -- problems, worlds and one-shot solves created and destroyed
many times leave the device memory where it was (grow-only buffers are owned by their object
and go with it); several contexts on one host thread share nothing (each owns its stream and
the dense solvers' scratch, pinned records and side stream)."""
import numpy as np
import pytest
import torch

from eggshell_amd import capi, scenes
from helpers import random_system
from oracle import oracle as orc
from test_oracle_lcp import _spd

pytestmark = pytest.mark.gpu


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def one_cycle(ctx, rng, k):
    s, rhs = random_system(rng, 60, 500 + 40 * (k % 5), connected=bool(k & 1))
    pr = capi.Problem(ctx, s.n, s.body0, s.body1, capi.F32 if k % 3 == 0 else capi.F64)
    pr.set_blocks(s.Minv, s.J0, s.J1, s.is_eq, s.lo, s.hi, rhs)
    pr.solve(capi.params(method=capi.GAUSS_SEIDEL, max_iters=5, tol=0.0 if k % 2 else 1e-9, cfm=0.05))
    pr.close()
    sc = scenes.box_stack(3, 3, 2 + k % 3)
    n = sc["p"].shape[0]
    Minv = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
    f_ext = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
    wd = capi.World(ctx, n)
    wd.set_bodies(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
    for _ in range(3):
        wd.step(0.005, 0.2, capi.params(method=capi.GAUSS_SEIDEL, max_iters=10, tol=0.0, cfm=0.01))
    wd.close()
    ctx.update_contacts(sc["p"], sc["R"])


def test_create_destroy_cycles_do_not_leak_device_memory(ctx):
    rng = np.random.default_rng(70)
    for k in range(6):        # warm up: allocator pools, code objects, the context's pinned arena
        one_cycle(ctx, rng, k)
    before = free_bytes()
    for k in range(60):
        one_cycle(ctx, rng, k)
    after = free_bytes()
    assert before - after < (8 << 20), (before, after)     # nothing proportional to the 60 cycles


def mixed_problem(rng, dim):
    """The recipe of test_gpu_dense.py::test_mixed_no_bounds_vs_oracle."""
    A = _spd(rng, dim)
    b = rng.uniform(-1, 1, dim)
    Ceq = rng.integers(0, 2, dim).astype(np.uint8)
    return A, b, Ceq, np.zeros(dim), np.full(dim, np.inf)


def c5_problem(N, seed=0):
    """The recipe of bench.py's c5_problem beyond 512 rows (GenerateSPDMatrix + 1e-3 I, C ~ Bernoulli(1/2))."""
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (N, N))
    A = M.T @ M + 1e-3 * np.eye(N)
    b = rng.uniform(-1, 1, N)
    C = (rng.uniform(size=N) < 0.5).astype(np.uint8)
    return A, b, C, np.zeros(N), np.full(N, np.inf)


def assert_same(got, want):
    ok, x, w, piv = got
    ok0, x0, w0, piv0 = want
    assert ok == ok0 and piv == piv0
    assert np.array_equal(x, x0) and np.array_equal(w, w0)      # bit for bit: the operation order is fixed


def test_two_contexts_alternate_on_one_thread(ctx):
    """Two contexts on device 0, driven in turn by one host thread with problems of different sizes, each return
    what a context on its own returns, bit for bit (the factorisation and the pivot rule have a fixed operation
    order; a repeated solve on the session context is asserted to be bit-identical first).  N = 320 with 166
    equality rows takes the fused panel factorisation (more than 64 Schur columns: the second array) and the
    multi-launch Murty loop (more than 112 inequality rows: the pinned step record)."""
    rng = np.random.default_rng(322)
    one, two = mixed_problem(rng, 320), mixed_problem(rng, 192)
    assert 160 <= int(one[2].sum()) <= 192
    solo = {}
    for name, pb in (("one", one), ("two", two)):
        for mode in (0, 2):
            solo[name, mode] = ctx.mixed_constraints_solve(*pb, use_bounds=mode)
            assert solo[name, mode][0]
            assert_same(ctx.mixed_constraints_solve(*pb, use_bounds=mode), solo[name, mode])
    a, b = capi.Context(0), capi.Context(0)
    try:
        for _ in range(8):
            for c, name, pb in ((a, "one", one), (b, "two", two), (a, "two", two), (b, "one", one)):
                for mode in (0, 2):
                    assert_same(c.mixed_constraints_solve(*pb, use_bounds=mode), solo[name, mode])
        a.close()
        for mode in (0, 2):
            assert_same(b.mixed_constraints_solve(*one, use_bounds=mode), solo["one", mode])
    finally:
        a.close()
        b.close()


def test_side_stream_belongs_to_the_context(ctx):
    """N = 1024 is the smallest size at which the host entry splits the upload of A across a second stream."""
    pb = c5_problem(1024)
    A, rhs = pb[0], pb[1]
    solo = ctx.mixed_constraints_solve(*pb, use_bounds=2)
    assert solo[0]
    solo_resid = np.abs(A @ solo[1] - rhs - solo[2]).max()
    a, b = capi.Context(0), capi.Context(0)
    try:
        for _ in range(2):
            for c in (a, b, a, b):
                got = c.mixed_constraints_solve(*pb, use_bounds=2)
                assert_same(got, solo)
                assert np.abs(A @ got[1] - rhs - got[2]).max() <= solo_resid
    finally:
        a.close()
        b.close()


def test_context_scratch_goes_with_the_context():
    """One leaked factor array per cycle would be over 80 MB in 20 cycles; the bound is that of the test above."""
    pb = c5_problem(512)

    def cycle():
        c = capi.Context(0)
        try:
            assert c.mixed_constraints_solve(*pb, use_bounds=2)[0]
        finally:
            c.close()

    for _ in range(3):
        cycle()
    before = free_bytes()
    for _ in range(20):
        cycle()
    after = free_bytes()
    assert before - after < (8 << 20), (before, after)
