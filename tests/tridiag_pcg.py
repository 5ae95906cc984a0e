"""Restatement of the reference PCG's sparse-M branch (helmFE_var.py:546-586, `M.nnz > n`: z = spsolve(M, r)) for the
tridiagonal-preconditioner tests, plus the test systems they share.  Unconjugated dots, stop on sqrt(|r.r|) < tol after the
update, returns (x, i) with i the index of the last iteration run -- the reference's return value."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def pcg_sparse(A, b, M, x0=None, tol=1e-6, maxit=1000, history=False, solve=None):
    """solve: optional z = solve(r) in place of spsolve(M, r) (e.g. a factorisation made once with splu)"""
    A = sp.csr_matrix(A)
    M = sp.csr_matrix(M)
    x = np.zeros(b.size, dtype=complex) if x0 is None else x0
    r = b - A.dot(x)
    hist = [np.dot(r, r)]
    i = -1
    for i in range(maxit):
        z = solve(r) if solve is not None else spla.spsolve(M, r)
        rho = np.dot(r, z)
        if i == 0:
            p = z
        else:
            p = z + (rho / rho_2) * p
        q = A.dot(p)
        alpha = rho / np.dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        hist.append(np.dot(r, r))
        if np.sqrt(abs(hist[-1])) < tol:
            break
        rho_2 = rho
    return (x, i, np.asarray(hist)) if history else (x, i)


def band(A, width=2):
    """the entries of A with |i - j| < width (width 2: the tridiagonal part)"""
    c = sp.coo_matrix(A)
    keep = np.abs(c.row - c.col) < width
    return sp.csr_matrix((c.data[keep], (c.row[keep], c.col[keep])), shape=A.shape)


def csr(g, prefix):
    ip, ix, da = g[f"{prefix}_indptr"], g[f"{prefix}_indices"], g[f"{prefix}_data"]
    return sp.csr_matrix((da, ix, ip), shape=(len(ip) - 1,) * 2)


def laplace3d_aniso(nx, ny, nz, cx=1.0, shift=0.0):
    """7-point Laplacian on nx x ny x nz nodes (x fastest), x-coupling cx times the others, plus shift on the diagonal"""
    def t(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")
    Ix, Iy, Iz = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    A = cx * sp.kron(Iz, sp.kron(Iy, t(nx))) + sp.kron(Iz, sp.kron(t(ny), Ix)) + sp.kron(t(nz), sp.kron(Iy, Ix))
    A = sp.csr_matrix(A + shift * sp.identity(nx * ny * nz))
    A.sort_indices()
    return A
