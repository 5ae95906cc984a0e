#!/usr/bin/env python3
"""Generate tests/golden/pcg_tridiag_iterates.npz from the UNMODIFIED reference PCG with a tridiagonal sparse M.

TEST INFRASTRUCTURE ONLY, modelled on oracle/make_golden.py: run once in the build container (`python
scripts/make_golden_tridiag.py`, CG_REFERENCE = the reference checkout); the GPU box never sees the reference, so the numbers are
committed as data.  helmFE_var.py is imported read-only for helmFE_var, rhsA and PCG (whose `M.nnz > n` branch solves
M z = r with spsolve, helmFE_var.py:561-562).  M is built the way the reference's own driver builds `Htrid`: the entries of the
matrix with |i - j| < 10 (helmFE_var.py:660-673), i.e. the tridiagonal coupling along grid lines of more than 10 nodes.
Only inputs and numeric outputs are written.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

REF = os.environ.get("CG_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "pcg_tridiag_iterates.npz")
KS = (1, 2, 3, 7, 12)


def band(A, width=10):
    """the entries of A with |i - j| < width, as a CSR matrix (the driver's Htrid)"""
    c = sp.coo_matrix(A)
    keep = np.abs(c.row - c.col) < width
    return sp.csr_matrix((c.data[keep], (c.row[keep], c.col[keep])), shape=A.shape)


def csr_parts(prefix, A, out):
    A = sp.csr_matrix(A)
    A.sort_indices()
    out[f"{prefix}_indptr"], out[f"{prefix}_indices"], out[f"{prefix}_data"] = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


def aniso_poisson(N, cx):
    """5-point Poisson on N x N nodes (x fastest), x-coupling cx times the y-coupling"""
    T = sp.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
    return sp.csr_matrix(cx * sp.kron(sp.identity(N), T) + sp.kron(T, sp.identity(N)))


def main():
    sys.path.insert(0, REF)
    import helmFE_var as hv  # noqa
    sys.path.pop(0)
    g = {"ks": np.array(KS)}
    N = 16
    H = sp.csr_matrix(hv.helmFE_var(N=N, omega=12.0, C=np.ones((N - 1, N - 1)), rho=0.15, Nhoriz=N, Nvert=N))
    b = hv.rhsA(N, 12.0).flatten()
    M = band(H)
    csr_parts("helm16", H, g)
    csr_parts("helm16_M", M, g)
    g["helm16_b"] = b
    g["helm16_X"] = np.stack([hv.PCG(H, b, M=M, tol=0.0, maxit=k)[0] for k in KS])   # tol 0: exactly k iterations
    x, i = hv.PCG(H, b, M=M, tol=1e-6, maxit=1000)
    g["helm16_tol1e-6_x"], g["helm16_tol1e-6_i"] = x, np.array(i)

    A = aniso_poisson(16, 100.0)
    MA = band(A)
    bA = np.linspace(1.0, 2.0, A.shape[0])
    csr_parts("aniso16", A, g)
    csr_parts("aniso16_M", MA, g)
    g["aniso16_b"] = bA
    g["aniso16_X"] = np.stack([hv.PCG(A, bA, M=MA, tol=0.0, maxit=k)[0] for k in KS])
    x, i = hv.PCG(A, bA, M=MA, tol=1e-10, maxit=1000)
    g["aniso16_tol1e-10_x"], g["aniso16_tol1e-10_i"] = x, np.array(i)
    np.savez_compressed(OUT, **g)
    print(OUT, os.path.getsize(OUT), {k: int(g[k]) for k in ("helm16_tol1e-6_i", "aniso16_tol1e-10_i")})


if __name__ == "__main__":
    main()
