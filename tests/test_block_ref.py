"""Block CG restated on the host (tests/block_ref.py) against separate CG solves (shift_ref.cg): convergence, the true residual, fewer
iterations than any single solve, healthy pivots, the breakdown of dependent columns, and s = 1 against plain CG."""
import numpy as np
import pytest

import block_ref as B
import shift_ref as R

GRIDS = [(33, 29), (64, 64), (97, 41)]
TOL = {np.float32: 1e-4, np.float64: 1e-8}
_single = {}


def _rhs(n, s):
    return np.random.default_rng(11).standard_normal((n, s))


def _single_iterations(grid, s, dtype):
    """iterations of each of the s single solves to tol |b_j| (history of shift_ref.cg, run once per case)"""
    key = (grid, s, dtype)
    if key not in _single:
        A = R.laplace2d(*grid).astype(dtype)
        b = _rhs(A.shape[0], s).astype(dtype)
        its = []
        for j in range(s):
            _, h = R.cg(A, b[:, j].copy(), 400)
            below = np.nonzero(~(np.sqrt(np.abs(h.astype(np.float64))) >= TOL[dtype] * np.linalg.norm(b[:, j].astype(np.float64))))[0]
            assert below.size, "the single solve did not converge in 400 iterations"
            its.append(int(below[0]))
        _single[key] = its
    return _single[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("s", [2, 4, 9, 16])
@pytest.mark.parametrize("grid", GRIDS)
def test_converges_in_fewer_iterations(grid, s, dtype):
    A = R.laplace2d(*grid)
    b = _rhs(A.shape[0], s).astype(dtype)
    nb = np.linalg.norm(b.astype(np.float64), axis=0)
    got = B.bcg(A, b, tol=TOL[dtype] * nb, maxit=400, dtype=dtype)
    assert got["status"] == B.RUNNING and got["iterations"] < 400
    res = np.linalg.norm(b.astype(np.float64) - A @ got["X"].astype(np.float64), axis=0)
    print(grid, s, np.dtype(dtype).name, "iterations", got["iterations"], "single", min(_single_iterations(grid, s, dtype)),
          "res/tol|b|", float(np.max(res / (TOL[dtype] * nb))), "min pivot ratio", got["min_ratio"])
    assert np.all(res <= 2 * TOL[dtype] * nb)
    assert got["min_ratio"] > 0.1
    if s >= 4:
        assert got["iterations"] < min(_single_iterations(grid, s, dtype))
        if grid == (33, 29):
            assert got["iterations"] <= 0.77 * min(_single_iterations(grid, s, dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["duplicate", "combination"])
def test_dependent_columns_break_down_at_once(kind, dtype):
    A = R.laplace2d(33, 29)
    b = _rhs(A.shape[0], 4).astype(dtype)
    b[:, 3] = b[:, 1] if kind == "duplicate" else 2 * b[:, 1] - 0.5 * b[:, 0]
    got = B.bcg(A, b, tol=1e-4, maxit=20, dtype=dtype)
    assert (got["status"], got["event"], got["iterations"]) == (B.W_FAILED, 0, 0)
    assert not np.any(got["X"])
    assert got["min_ratio"] <= 4 * B.EPS[np.dtype(dtype)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_column_is_plain_cg(dtype):
    A = R.laplace2d(33, 29).astype(dtype)
    b = _rhs(A.shape[0], 1).astype(dtype)
    got = B.bcg(A, b, maxit=30, dtype=dtype)
    _, h = R.cg(A, b[:, 0].copy(), 30)
    eps = B.EPS[np.dtype(dtype)]
    # both are sums of n squares carried through 30 steps of a recurrence whose rounding errors grow with the condition of the
    # Krylov basis: 1e4 eps is what 957 terms and 30 iterations leave room for, far below any difference of method
    np.testing.assert_allclose(got["history"][:, 0].astype(np.float64), h.astype(np.float64), rtol=1e4 * eps)


def test_nan_is_its_own_status():
    C = np.eye(3).tolist()
    C[1][1] = float("nan")
    assert B.chol(C, 3, 2.0 ** -52)[1] == B.NAN
