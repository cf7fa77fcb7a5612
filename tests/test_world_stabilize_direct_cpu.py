"""CPU: the direct relaxation route (egs_world_stabilize_direct, egs_world_stabilize_rank, egs_relax_blocks_direct) is
part of the C ABI -- declared in the header, exported by the library, listed in capi.EXPORTS and reachable from
capi.World / capi.Context -- and the factorisation it runs on the device, restated here in numpy, is the right one:
an LDL^T with symmetric diagonal pivoting that stops at the first pivot <= rank_tol * |first pivot| reproduces the
least-squares correction J^T y on rank-deficient box stacks, does not depend on rank_tol over 1e-14 .. 1e-8, and on
full-rank chains agrees with the oracle's pivoted LDL^T; with its least-squares completion it does so on tilted
cairns too, whose err is not consistent.
No compute calls on the library here."""
import os
import re

import numpy as np
import pytest

from eggshell_amd import capi, scenes
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egs_world_stabilize_direct", "egs_world_stabilize_rank", "egs_relax_blocks_direct")


def truncated_ldlt_solve(A, b, rank_tol=1e-10, complete=True):
    """A y = b by LDL^T with symmetric diagonal pivoting (largest |diagonal|, lowest index on ties), stopped at the
    first pivot <= rank_tol * |first pivot|; y = 0 on the rows left.  Truncated at rank r < n, the rows left of the
    eliminated b hold the residual rho of an inconsistent b, and the leading block is solved for
    L1^-1 b1 + (W^T W)^-1 L2^T rho, W = [L1; L2] the n x r unit lower trapezoid, so that J^T y is the least-squares
    correction (complete = False: without that, the plain truncated solve).  Returns y and the rank."""
    A = np.array(A, dtype=np.float64)
    b = np.array(b, dtype=np.float64)
    n = b.shape[0]
    perm = np.arange(n)
    rank, d0 = n, 0.0
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))      # argmax returns the first of equal maxima
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
            b[[k, p]] = b[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        d = A[k, k]
        if k == 0:
            d0 = abs(d)
        if not abs(d) > rank_tol * d0:
            rank = k
            break
        col = A[k + 1:, k].copy()
        l = col / d
        A[k + 1:, k + 1:] -= np.outer(l, col)
        A[k + 1:, k] = l
        b[k + 1:] -= l * b[k]
    z = b[:rank].copy()
    if complete and 0 < rank < n:
        W = np.tril(A[:, :rank], -1)
        W[:rank] += np.eye(rank)
        z += np.linalg.solve(W.T @ W, W[rank:].T @ b[rank:])
    z = z / np.diag(A)[:rank]
    for k in range(rank - 1, 0, -1):
        z[:k] -= A[k, :k] * z[k]
    y = np.zeros(n)
    y[perm[:rank]] = z
    return y, rank


def dense_J(sc, J0, J1):
    n, m = sc["p"].shape[0], sc["kind"].shape[0]
    J = np.zeros((3 * m, 6 * n))
    for i in range(m):
        for bb, blk in ((sc["body0"][i], J0[i]), (sc["body1"][i], J1[i])):
            if bb >= 0:
                J[3 * i:3 * i + 3, 6 * bb:6 * bb + 6] = blk.reshape(3, 6)
    return J


def system(sc):
    J0, J1, _, _, _, err = orc.assemble(sc["p"], sc["R"], sc["kind"], sc["body0"], sc["body1"], sc["data"])
    J = dense_J(sc, J0, J1)
    return J, J @ J.T, err


def bent_chain(scale):
    sc = scenes.chain(4)
    for i in range(1, 4):
        sc["p"][i] += scale * np.array([0.01 * i, -0.02 * i, 0.015 * i])
    return sc


STACKS = {"2x2x2": lambda: scenes.box_stack(2, 2, 2), "2x2x2 jittered": lambda: scenes.box_stack(2, 2, 2, jitter=1e-3, seed=3),
          "2x2x3": lambda: scenes.box_stack(2, 2, 3), "4x4x4": lambda: scenes.box_stack(4, 4, 4)}


def detect(p, R):
    """The contact list of Ensemble::UpdateContacts with its pruning, from the oracle's collision routines."""
    n = p.shape[0]
    b0, b1, data = [], [], []
    for b in range(n):
        for c in orc.collide_box_ground(p[b], R[b]):
            b0.append(-1); b1.append(b); data.append(c)
    for i in range(n):
        for j in range(i + 1, n):
            if np.linalg.norm(p[i] - p[j]) > 0.53:
                continue
            cs, _ = orc.collide_boxes(p[i], R[i], p[j], R[j])
            for a in range(len(cs)):
                if not any(np.linalg.norm(cs[k][:3] - cs[a][:3]) < 1e-6 for k in range(a)):
                    b0.append(i); b1.append(j); data.append(cs[a])
    return np.array(b0, np.int32), np.array(b1, np.int32), np.array(data).reshape(-1, 7)


def _code():
    text = open(os.path.join(ROOT, "include", "eggshell_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_direct_entries():
    code = _code()
    for name in NEW:
        assert re.search(r"\begs_status\s+" + name + r"\s*\(", code), name
        assert name in capi.EXPORTS, name
    # mode, max_steps, detect_contacts, rank_tol, n_unsettled
    assert re.search(r"egs_world_stabilize_direct\s*\(\s*egs_world\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*int32_t\s+\w+\s*,\s*double\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)", code)
    # n_ensembles, rows, rank
    assert re.search(r"egs_world_stabilize_rank\s*\(\s*egs_world\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*\)", code)
    # ctx, n_bodies, m, body0, body1, J0, J1, err, rank_tol, y, rank
    assert re.search(r"egs_relax_blocks_direct\s*\(\s*egs_context\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s+\w+\s*,\s*double\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*\)", code)


def test_library_exports_the_direct_entries():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_layer_has_the_direct_interface():
    assert callable(getattr(capi.World, "stabilize_direct", None))
    assert callable(getattr(capi.World, "stabilize_rank", None))
    assert callable(getattr(capi.Context, "relax_blocks_direct", None))


@pytest.mark.parametrize("scale", [1.0, -0.7, 1.6])
def test_full_rank_chain_agrees_with_lstsq_and_the_oracle_ldlt(scale):
    J, A, err = system(bent_chain(scale))
    y, rank = truncated_ldlt_solve(A, err)
    assert rank == A.shape[0] == 12
    y_ls = np.linalg.lstsq(A, err, rcond=None)[0]
    assert np.abs(J.T @ y - J.T @ y_ls).max() < 1e-12
    n = err.shape[0]
    # no inequality row: the oracle's MixedConstraintsSolver is ldlt_solve_inplace(A, err)
    ok, y_orc, _, _ = orc.mixed_constraints(A, err, np.ones(n, np.uint8), np.zeros(n), np.zeros(n))
    assert ok
    assert np.abs(y - y_orc).max() < 1e-12


@pytest.mark.parametrize("name", list(STACKS))
def test_rank_deficient_stack_gives_the_least_squares_correction(name):
    J, A, err = system(STACKS[name]())
    n = err.shape[0]
    want = J.T @ np.linalg.lstsq(A, err, rcond=None)[0]
    got = {}
    for tol in (1e-14, 1e-12, 1e-10, 1e-8):
        y, rank = truncated_ldlt_solve(A, err, tol)
        assert rank == n // 2, (tol, rank)                   # four coplanar points per face: half the rows are redundant
        got[tol] = J.T @ y
        assert np.abs(got[tol] - want).max() < 1e-12, tol
    for tol in got:
        assert np.array_equal(got[tol], got[1e-10]), tol     # the result does not move with rank_tol



@pytest.mark.parametrize("n,seed", [(5, 11), (4, 7)])
def test_inconsistent_cairn_needs_and_gets_the_least_squares_completion(n, seed):
    """The contacts of tilted boxes over-determine the bodies: err is not in the range of J J^T, the plain truncated
    solve satisfies only the rows it kept, and the completion restores the least-squares correction."""
    sc = scenes.cairn(n, seed=seed)
    b0, b1, data = detect(sc["p"], sc["R"])
    sc = dict(sc, kind=np.ones(b0.shape[0], np.int32), body0=b0, body1=b1, data=data)
    J, A, err = system(sc)
    want = J.T @ np.linalg.lstsq(A, err, rcond=None)[0]
    y, rank = truncated_ldlt_solve(A, err)
    assert rank == 6 * n < err.shape[0]
    assert np.abs(J.T @ y - want).max() < 1e-12
    y_plain, _ = truncated_ldlt_solve(A, err, complete=False)
    assert np.abs(J.T @ y_plain - want).max() > 1e-3
