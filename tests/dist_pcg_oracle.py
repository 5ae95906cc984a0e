"""What the row-partitioned PCG tests share: the test systems, the preconditioner of a partition assembled GLOBALLY as the
block-diagonal of the per-rank M, and the serial oracle (tridiag_pcg.pcg_sparse in complex double) run with it.

  Jacobi: the global diagonal (a diagonal is block-diagonal under any partition).
  Line:   the global tridiagonal at the stride -- the entries of A at column - row in {-stride, 0, +stride} -- with every link
          that crosses a rank boundary removed (`cut=True`); `cut=False` keeps them: the M a handle would build if it took the
          halo columns of its local numbering for line neighbours, which it must not."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import tridiag_pcg as tp


def aniso_grid(nx, ny, nz, cz=100.0):
    """7-point Laplacian on nx x ny x nz nodes (x fastest) whose z-coupling is cz times the others"""
    def t(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")
    Ix, Iy, Iz = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    A = sp.kron(Iz, sp.kron(Iy, t(nx))) + sp.kron(Iz, sp.kron(t(ny), Ix)) + cz * sp.kron(t(nz), sp.kron(Iy, Ix))
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def chain(n, seed=3):
    """tridiagonal SPD, diagonally dominant, with off-diagonals that vary along the chain"""
    rng = np.random.default_rng(seed)
    off = -rng.uniform(0.5, 1.0, n - 1)
    main = 2.0 + rng.uniform(0.05, 0.5, n)
    A = sp.diags([off, main, off], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def helm(N):
    import cg_numpy
    ip, ix, da = cg_numpy.helm_fe_var(N, 12.0, np.ones((N - 1, N - 1)), 0.15, N, N)
    A = sp.csr_matrix((da, ix, ip), shape=(N * N, N * N))
    A.sort_indices()
    return A, cg_numpy.rhsA(N, 12.0).flatten()


def row_ranges(n, world):
    return [(n * g // world, n * (g + 1) // world) for g in range(world)]


def global_m(A, ranges, pre, cut=True):
    """pre: "jacobi" or ("line", stride)"""
    A = sp.csr_matrix(A)
    if pre == "jacobi":
        return sp.csr_matrix(sp.diags(A.diagonal()))
    stride = int(pre[1])
    c = sp.coo_matrix(A)
    keep = np.isin(c.col - c.row, (-stride, 0, stride))
    if cut:
        starts = np.array([r[0] for r in ranges])
        owner = lambda i: np.searchsorted(starts, i, side="right") - 1
        keep &= owner(c.row) == owner(c.col)
    return sp.csr_matrix((c.data[keep], (c.row[keep], c.col[keep])), shape=A.shape)


def oracle(A, b, M, iters):
    """(x, history of r.r) of `iters` PCG iterations in complex double; M factored once"""
    if M is None:
        M = sp.identity(A.shape[0], format="csr")
    lu = spla.splu(sp.csc_matrix(M).astype(complex))
    x, _, h = tp.pcg_sparse(sp.csr_matrix(A).astype(complex), np.asarray(b).astype(complex), M, tol=0.0, maxit=iters, history=True,
                            solve=lu.solve)
    return x, h


def first_below(hist, b, rel=1e-6):
    """the first k with sqrt|r_k . r_k| < rel ||b||, or None"""
    at = np.flatnonzero(np.sqrt(np.abs(hist)) < rel * np.linalg.norm(b))
    return int(at[0]) if at.size else None


def local_part(A, ranges, rank):
    """this rank's rows with GLOBAL columns: (indptr, global columns, values)"""
    A = sp.csr_matrix(A)
    rb, re = ranges[rank]
    lo, hi = A.indptr[rb], A.indptr[re]
    return (A.indptr[rb:re + 1] - lo).astype(np.int32), A.indices[lo:hi].astype(np.int64), A.data[lo:hi]
