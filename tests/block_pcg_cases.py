"""The systems, right-hand sides and host preconditioners the preconditioned block CG tests share (tests/test_block_pcg_ref.py on the
CPU, tests/test_gpu_block_pcg*.py on the GPU).

A = D^1/2 L D^1/2: L the five-point Laplacian (shift_ref.laplace2d) on 33 x 29 (957 rows, padded inside the handle, 4 Gram
work-groups) or 64 x 64, D diagonal with entries 10^u, u uniform in [0, 2] from default_rng(12), rounded to the handle's type; A is
rounded to the handle's type too.  Jacobi then really changes the iteration.  Right-hand sides: default_rng(11), as
test_gpu_block.py draws them.

AHEAD lists the tolerance cases in which the restatement needs at least 2 iterations fewer than the slowest column of separate PCG
solves with the same M (test_block_pcg_ref.py asserts that it does): the cases in which the GPU test asserts "strictly fewer"."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import mg_ref
import shift_ref as R

GRIDS = {"33x29": (33, 29), "64x64": (64, 64)}
TOL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-8}
DTYPES = (np.float32, np.float64)
# (preconditioner, grid, s): the tolerance cases, in both types
TOL_CASES = [("jacobi", g, s) for g in GRIDS for s in (2, 9, 16)] + [("multigrid", g, 9) for g in GRIDS] + [("line", "33x29", 2)]
# cases where block PCG is ahead of the slowest single PCG solve by at least 2 iterations, in both types: on this system all of them
# (the smallest margin on the host: 7 iterations, line at s = 2 in float32; Jacobi at s = 16: 48 and more)
AHEAD = list(TOL_CASES)

_SYS = {}


def system(name, dtype):
    """A as the handle holds it (rounded to dtype), as a float64 CSR matrix with sorted indices"""
    key = (name, np.dtype(dtype).name)
    if key not in _SYS:
        nx, ny = GRIDS[name]
        d = (10.0 ** np.random.default_rng(12).uniform(0.0, 2.0, nx * ny)).astype(dtype).astype(np.float64)
        h = sp.diags(np.sqrt(d))
        A = sp.csr_matrix((h @ R.laplace2d(nx, ny) @ h).astype(dtype).astype(np.float64))
        A.sort_indices()
        _SYS[key] = A
    return _SYS[key]


def rhs(name, s, dtype):
    """(n, s), as rounded to dtype"""
    n = GRIDS[name][0] * GRIDS[name][1]
    return np.random.default_rng(11).standard_normal((n, s)).astype(dtype)


def jacobi(name, dtype):
    """1 / diag(A) in the handle's type"""
    dtype = np.dtype(dtype)
    return (dtype.type(1) / system(name, dtype).diagonal().astype(dtype)).astype(dtype)


def host_precond(kind, name, dtype):
    """M for block_pcg_ref.bpcg and pcg below: the Jacobi diagonal in dtype, or a callable on (s, n) blocks -- the V-cycle of mg_ref in
    the arithmetic of dtype, or the solve with the tridiagonal part of A (x-lines)"""
    dtype = np.dtype(dtype)
    A = system(name, dtype)
    if kind == "jacobi":
        return jacobi(name, dtype)
    if kind == "multigrid":
        H = mg_ref.Hierarchy(A, GRIDS[name], dtype)
        return lambda W: np.array([H.vcycle(w, dtype) for w in W]).astype(dtype)
    if kind == "line":
        ab = np.zeros((3, A.shape[0]))
        ab[0, 1:], ab[1], ab[2, :-1] = A.diagonal(1), A.diagonal(), A.diagonal(-1)
        return lambda W: scipy.linalg.solve_banded((1, 1), ab, W.astype(np.float64).T).T.astype(dtype)
    raise ValueError(kind)


def pcg(A, b, M, tol, maxit, dtype):
    """plain PCG on one column in dtype (helmFE_var.py's loop): the iterations to sqrt(r.r) < tol, and x"""
    dtype = np.dtype(dtype)
    A = A.astype(dtype)
    apply = M if callable(M) else (lambda W: (M[None, :] * W).astype(dtype))
    x = np.zeros_like(b)
    r = b.copy()
    z = apply(r[None, :])[0]
    p = z.copy()
    rho = np.dot(r.astype(np.float64), z.astype(np.float64))
    for k in range(1, maxit + 1):
        q = (A @ p).astype(dtype)
        alpha = dtype.type(rho / np.dot(p.astype(np.float64), q.astype(np.float64)))
        x = x + alpha * p
        r = r - alpha * q
        if np.sqrt(np.dot(r.astype(np.float64), r.astype(np.float64))) < tol:
            return k, x
        z = apply(r[None, :])[0]
        rho_new = np.dot(r.astype(np.float64), z.astype(np.float64))
        p = z + dtype.type(rho_new / rho) * p
        rho = rho_new
    return maxit, x
