"""What the tests of multigrid PCG on the row-partitioned handle share (cgamd_dist_set_preconditioner_multigrid / _amg): the
preconditioner of a partition assembled GLOBALLY as the block diagonal of per-rank hierarchies, each the host restatement
(mg_ref.Hierarchy, amg_ref.Hierarchy) on the rank's CUT block A[lo:hi, lo:hi] with the rank's own dims; the uncut variant, one
hierarchy on all of A (what a handle would apply if the cut were wrong or missing); and the serial PCG in complex double run with
either (tridiag_pcg.pcg_sparse(..., solve=)).

The hierarchies hold what the device holds -- level matrices and 1 / diag rounded once to the value type `dtype` -- and the cycle
runs in double / complex double (mg_ref.Hierarchy.solve)."""
import numpy as np
import scipy.sparse as sp

import amg_ref
import mg_ref
import tridiag_pcg as tp


def row_ranges(n, world):
    return [(n * g // world, n * (g + 1) // world) for g in range(world)]


def cut_block(A, ranges, rank):
    """the rank's rows without the columns of other ranks, stored order kept"""
    lo, hi = ranges[rank]
    B = sp.csr_matrix(sp.csr_matrix(A)[lo:hi, lo:hi])
    B.sort_indices()            # (the test matrices are stored sorted: the cut keeps that order)
    return B


def local_dims(dims, ranges, rank):
    """the rank's box of a grid numbered x fastest cut into z-slabs of whole planes"""
    nx, ny, nz = dims
    lo, hi = ranges[rank]
    assert lo % (nx * ny) == 0 and hi % (nx * ny) == 0, (dims, ranges[rank])
    return (nx, ny, (hi - lo) // (nx * ny))


def hierarchies(A, ranges, dtype, dims=None, opts=None):
    """one hierarchy per rank on its cut block: the grid form with `dims` (the GLOBAL grid), the algebraic form without"""
    opts = dict(opts or {})
    out = []
    for rank in range(len(ranges)):
        B = cut_block(A, ranges, rank)
        out.append(mg_ref.Hierarchy(B, local_dims(dims, ranges, rank), dtype, **opts) if dims is not None
                   else amg_ref.Hierarchy(B, dtype, **opts))
    return out


def block_solve(hs, ranges):
    """z = M^-1 r with M the block diagonal of the ranks' hierarchies"""
    fs = [h.solve() for h in hs]

    def f(r):
        return np.concatenate([fs[g](r[lo:hi]) for g, (lo, hi) in enumerate(ranges)])
    return f


def uncut_solve(A, dtype, dims=None, opts=None):
    """one hierarchy on all of A"""
    opts = dict(opts or {})
    h = mg_ref.Hierarchy(A, dims, dtype, **opts) if dims is not None else amg_ref.Hierarchy(A, dtype, **opts)
    return h.solve()


def jacobi_solve(A):
    dinv = 1.0 / sp.csr_matrix(A).diagonal()
    return lambda r: dinv * r


def oracle(A, b, solve, iters, tol=0.0):
    """(x, history of r.r) of PCG in complex double with z = solve(r): `iters` iterations, or up to `iters` to sqrt|r.r| < tol"""
    A = sp.csr_matrix(A).astype(complex)
    x, _, h = tp.pcg_sparse(A, np.asarray(b).astype(complex), sp.identity(A.shape[0], format="csr"), tol=tol, maxit=iters, history=True,
                            solve=solve)
    return x, h


def first_below(hist, b, rel=1e-6):
    """the first k with sqrt|r_k . r_k| < rel ||b||, or None"""
    at = np.flatnonzero(np.sqrt(np.abs(hist)) < rel * np.linalg.norm(b))
    return int(at[0]) if at.size else None


def hist_dev(h, ref, scale, keep):
    """max over the kept entries of |h - ref| / |scale| (not finite counts as infinite)"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(h) - ref) / np.abs(scale)
    return float(np.max(np.where(np.isfinite(d), d, np.inf)[keep]))
