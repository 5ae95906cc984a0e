"""CPU check of the tridiagonal-M golden data: the restatement in tridiag_pcg (z = spsolve(M, r)) reproduces the unmodified
reference PCG's iterates with M = the driver's |i - j| < 10 band (tests/golden/pcg_tridiag_iterates.npz,
scripts/make_golden_tridiag.py).  To 1e-12, not bit for bit: the sparse direct solver may differ between machines."""
import os

import numpy as np

import tridiag_pcg as tp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcg_tridiag_iterates.npz")


def test_restatement_reproduces_reference_tridiag_pcg():
    g = np.load(GOLDEN)
    for name, tol_key, tol in (("helm16", "tol1e-6", 1e-6), ("aniso16", "tol1e-10", 1e-10)):
        A, M, b = tp.csr(g, name), tp.csr(g, f"{name}_M"), g[f"{name}_b"]
        assert M.nnz > M.shape[0]                                        # the reference's spsolve branch
        assert (M - tp.band(A)).count_nonzero() == 0                     # ... with exactly the tridiagonal part of A
        for k, want in zip(g["ks"], g[f"{name}_X"]):
            x, i = tp.pcg_sparse(A, b, M, tol=0.0, maxit=int(k))
            assert i == k - 1
            assert np.linalg.norm(x - want) / np.linalg.norm(want) < 1e-12, (name, k)
        x, i = tp.pcg_sparse(A, b, M, tol=tol, maxit=1000)
        assert i == int(g[f"{name}_{tol_key}_i"])
        want = g[f"{name}_{tol_key}_x"]
        assert np.linalg.norm(x - want) / np.linalg.norm(want) < 1e-12
