"""Preconditioned block CG restated on the host (tests/block_pcg_ref.py) against separate PCG solves with the same M
(block_pcg_cases.pcg, and scipy's direct solve): convergence to the tolerance in float64, the breakdowns, and the two claims the GPU
test (tests/test_gpu_block_pcg.py) leans on -- that the restatement run in the handle's type alone meets the true-residual condition
2 tol |b_j| in every tolerance case, and that in the cases of block_pcg_cases.AHEAD it needs at least 2 iterations fewer than the
slowest column of the separate solves."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import block_pcg_cases as C
import block_pcg_ref as BP
import block_ref as B

_RUN = {}


def run(kind, name, s, dtype):
    """the restatement and the s separate solves of one tolerance case, once: (block result, iterations of every single solve, their x)"""
    key = (kind, name, s, np.dtype(dtype).name)
    if key not in _RUN:
        dtype = np.dtype(dtype)
        A, b, M = C.system(name, dtype), C.rhs(name, s, dtype), C.host_precond(kind, name, dtype)
        nb = np.linalg.norm(b.astype(np.float64), axis=0)
        got = BP.bpcg(A, b, M, tol=C.TOL[dtype] * nb, maxit=400, dtype=dtype)
        single = [C.pcg(A, b[:, j].copy(), M, C.TOL[dtype] * nb[j], 400, dtype) for j in range(s)]
        _RUN[key] = got, [k for k, _ in single], np.array([x for _, x in single]).T
    return _RUN[key]


def residual(name, dtype, b, x):
    b64 = b.astype(np.float64)
    return np.linalg.norm(b64 - C.system(name, dtype) @ x.astype(np.float64), axis=0) / np.linalg.norm(b64, axis=0)


@pytest.mark.parametrize("kind,name,s", C.TOL_CASES, ids=lambda v: str(v))
def test_float64_against_separate_pcg_solves(kind, name, s):
    dtype = np.dtype(np.float64)
    got, its, xs = run(kind, name, s, dtype)
    b = C.rhs(name, s, dtype)
    assert got["status"] == B.RUNNING and got["iterations"] < 400 and max(its) < 400
    res, res_single = residual(name, dtype, b, got["X"]), residual(name, dtype, b, xs)
    exact = spla.spsolve(C.system(name, dtype).tocsc(), b)
    err = np.linalg.norm(got["X"] - exact, axis=0) / np.linalg.norm(exact, axis=0)
    err_single = np.linalg.norm(xs - exact, axis=0) / np.linalg.norm(exact, axis=0)
    print(kind, name, s, "block", got["iterations"], "single", its, "res/tol", float(np.max(res / 1e-8)), "single", float(np.max(res_single / 1e-8)),
          "error", float(err.max()), "single", float(err_single.max()), "min pivot ratio", got["min_ratio"])
    assert np.all(res <= 2e-8)
    # both stopped on the same residual test: the block's solution is as close to the exact one as the separate solves' (their worst
    # column, twice over: the columns of a block stop together, the separate solves each on its own)
    assert err.max() <= 2 * err_single.max()
    assert got["iterations"] <= max(its) and got["min_ratio"] > 1e-3
    # the history is r.r of the recurrence: row k against the true residual of ... the last row, the only X there is
    true_rr = np.linalg.norm(b - C.system(name, dtype) @ got["X"], axis=0) ** 2
    np.testing.assert_allclose(got["history"][-1], true_rr, rtol=1e-3)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind,name,s", C.TOL_CASES, ids=lambda v: str(v))
def test_what_the_gpu_test_leans_on(kind, name, s, dtype):
    dtype = np.dtype(dtype)
    got, its, _ = run(kind, name, s, dtype)
    res = residual(name, dtype, C.rhs(name, s, dtype), got["X"])
    ahead = max(its) - got["iterations"]
    print(kind, name, s, dtype.name, "block", got["iterations"], "slowest single", max(its), "ahead by", ahead, "res/tol", float(np.max(res / C.TOL[dtype])))
    assert got["status"] == B.RUNNING
    assert np.all(res <= 2 * C.TOL[dtype]), "the restatement alone misses the true-residual condition: replace the case"
    if (kind, name, s) in C.AHEAD:
        assert ahead >= 2
    assert {("jacobi", g, 16) for g in C.GRIDS} <= set(C.AHEAD) and any(k == "multigrid" for k, _, _ in C.AHEAD)


def test_the_diagonal_form_is_the_callable_form():
    """a diagonal M given as an array (z never stored as a block) against the same M as a callable: the same bits"""
    for dtype in C.DTYPES:
        A, b, m = C.system("33x29", dtype), C.rhs("33x29", 9, dtype), C.jacobi("33x29", dtype)
        a = BP.bpcg(A, b, m, maxit=6, dtype=dtype)
        c = BP.bpcg(A, b, lambda W: (m[None, :] * W).astype(dtype), maxit=6, dtype=dtype)
        assert a["X"].tobytes() == c["X"].tobytes() and a["history"].tobytes() == c["history"].tobytes()


def test_identity_m_is_block_cg_up_to_the_history():
    """M = I: the recurrence is block_ref.bcg's (Z = W, W^T Z = W^T W); x agrees to rounding, and the history -- formed from W^T W
    and the old xi here, from the new xi there -- to rounding too"""
    A, b = C.system("33x29", np.float64), C.rhs("33x29", 4, np.float64)
    a = BP.bpcg(A, b, np.ones(A.shape[0]), maxit=10, dtype=np.float64)
    c = B.bcg(A, b, maxit=10, dtype=np.float64)
    np.testing.assert_allclose(a["X"], c["X"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(a["history"], c["history"], rtol=1e-10)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_breakdowns(dtype):
    dtype = np.dtype(dtype)
    A, b, m = C.system("33x29", dtype), C.rhs("33x29", 4, dtype), C.jacobi("33x29", dtype)
    b[:, 3] = b[:, 1]
    got = BP.bpcg(A, b, m, maxit=5, dtype=dtype)
    assert (got["status"], got["event"], got["iterations"]) == (B.W_FAILED, 0, 0) and got["min_ratio"] <= 4 * B.EPS[dtype]
    assert not np.any(got["X"])
    np.testing.assert_allclose(got["history"][0].astype(np.float64), np.sum(b.astype(np.float64) ** 2, axis=0), rtol=1e-6)
    # an M that is not positive definite on the block: R0^T M^-1 R0 has a negative pivot
    b = C.rhs("33x29", 4, dtype)
    got = BP.bpcg(A, b, -m, maxit=5, dtype=dtype)
    assert (got["status"], got["event"]) == (B.W_FAILED, 0)
