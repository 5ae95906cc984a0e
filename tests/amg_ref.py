"""Host restatement of the algebraic aggregation multigrid preconditioner (cgamd_solver_set_preconditioner_amg; include/cgamd.h
states the algorithm): the strength of connection, the rounds of deterministic handshake matching, the numbering of the aggregates,
the chain of passes with the Galerkin product rounded once per pass, and the rules that stop coarsening.  The smoother, its
coefficients and the V-cycle (already written through a map) are mg_ref's.

Every decision of the matching is a comparison of doubles and 32-bit integers, so the maps are the device's exactly whenever the pass
matrices are (integer-valued matrices: every sum exact)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph

import mg_ref

MAX_ROUNDS, MAX_ROW, WIDTH = 32, 64, 8


def pair_hash(i, j):
    """h(i, j), symmetric, in 32-bit unsigned arithmetic (arrays or scalars)"""
    i, j = np.asarray(i, np.uint64), np.asarray(j, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    h = ((lo * np.uint64(0x9E3779B1)) & M) ^ hi
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M
    h ^= h >> np.uint64(16)
    return h


def match_pass(B, theta, max_rounds=MAX_ROUNDS):
    """one pass of handshake matching on the CSR matrix B: (match, rounds) -- match[i] = the partner of row i or -1, rounds = the
    rounds that formed a pair (the matching ends with the first round that forms none, or after max_rounds)"""
    B = sp.csr_matrix(B)
    n = B.shape[0]
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(B.indptr))
    c = B.indices.astype(np.int64)
    s = -np.real(B.data).astype(np.float64)
    off = r != c
    pos = off & (s > 0)                              # (a NaN compares false)
    smax = np.zeros(n)
    np.maximum.at(smax, r[pos], s[pos])
    strong = pos & (s >= theta * smax[r])
    r, c, s = r[strong], c[strong], s[strong]
    h = pair_hash(r, c).astype(np.int64)
    order = np.lexsort((c, -h, -s, r))               # per row: larger s, then larger h, then smaller column
    r, c = r[order], c[order]
    match = np.full(n, -1, np.int64)
    rounds = 0
    while rounds < max_rounds:
        open_ = (match[r] < 0) & (match[c] < 0)      # the matching as it stands when the round begins
        rr, cc = r[open_], c[open_]
        first = np.ones(rr.size, bool)
        first[1:] = rr[1:] != rr[:-1]
        pick = np.full(n, -1, np.int64)
        pick[rr[first]] = cc[first]
        i = np.flatnonzero(pick >= 0)
        i = i[pick[pick[i]] == i]
        if i.size == 0:
            break
        match[i] = pick[i]
        rounds += 1
    return match, rounds


def number(match):
    """(pmap, nc): the root of an aggregate is its smaller member, coarse ids are the ranks of the roots in ascending order"""
    n = match.size
    i = np.arange(n)
    root = (match < 0) | (match > i)
    rank = np.cumsum(root) - root
    return np.where(root, rank, rank[np.where(root, i, match)]), int(root.sum())


def galerkin(A, agg, nc, dtype):
    """mg_ref.galerkin through a map: (csr of dtype, the most distinct columns of a row)"""
    A = sp.csr_matrix(A)
    agg = np.asarray(agg, np.int64)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    key = agg[rows] * nc + agg[A.indices]
    uniq, inv = np.unique(key, return_inverse=True)
    W = mg_ref.wide(dtype)
    acc = np.zeros(uniq.size, W)
    np.add.at(acc, inv, A.data.astype(W))            # in sequence: fine rows ascending, entries in stored order
    counts = np.bincount(uniq // nc, minlength=nc)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    Ac = sp.csr_matrix((acc.astype(dtype), (uniq % nc).astype(np.int32), ptr.astype(np.int32)), shape=(nc, nc))
    return Ac, int(counts.max())


def coarsen(A, dtype, passes=3, theta=0.25, stats=None):
    """the next level from the matrix A of a level: (agg, A_next), or None when the level is not built.  stats, a list, receives
    the rounds of every pass run"""
    nf = A.shape[0]
    B, agg = A, None
    for _ in range(passes):
        match, rounds = match_pass(B, theta)
        if stats is not None:
            stats.append(rounds)
        pmap, nc = number(match)
        Bn, widest = galerkin(B, pmap, nc, dtype)
        if widest > MAX_ROW:
            break                                    # this pass and the ones after it are dropped
        agg = pmap if agg is None else pmap[agg]
        B = Bn
    if agg is None or 5 * B.shape[0] > 4 * nf:
        return None
    return agg, B


class Hierarchy(mg_ref.Hierarchy):
    """mg_ref.Hierarchy with the aggregates matched from the matrix; smooth, vcycle (through L.agg) and solve are inherited"""

    def __init__(self, A, dtype, passes=3, strength=0.25, smooth_steps=1, over_correction=1.6, min_rows=512):
        self.dtype = np.dtype(dtype)
        self.omega, self.steps = float(over_correction), int(smooth_steps)
        A = sp.csr_matrix(A).astype(self.dtype)
        self.levels, self.rounds = [], []
        W = mg_ref.wide(self.dtype)
        while True:
            L = mg_ref.Level()
            L.A, L.n, L.dims = A, A.shape[0], (A.shape[0], 0, 0)
            Aw = A.astype(W)
            diag = Aw.diagonal()
            if np.any(diag == 0) or not np.all(np.isfinite(diag)):
                raise ZeroDivisionError(f"level {len(self.levels)}: zero, missing or non-finite diagonal in row "
                                        f"{int(np.flatnonzero((diag == 0) | ~np.isfinite(diag))[0])}")
            L.dinv = (W(1) / diag).astype(self.dtype)
            absA = sp.csr_matrix((np.abs(Aw.data), A.indices, A.indptr), shape=A.shape)
            L.lmax = float(np.max(np.abs(L.dinv.astype(W)) * np.asarray(absA @ np.ones(L.n))))
            self.levels.append(L)
            if L.n <= min_rows or len(self.levels) == mg_ref.MAX_LEVELS:
                break
            nxt = coarsen(A, self.dtype, passes, strength, self.rounds)
            if nxt is None:
                break
            L.agg, A = nxt
        for l, L in enumerate(self.levels):
            last = l == len(self.levels) - 1
            L.steps = mg_ref.COARSEST_STEPS if last else self.steps
            L.c0, L.c1 = mg_ref.chebyshev_coefficients(L.lmax, mg_ref.KAPPA_COARSEST if last else mg_ref.KAPPA_SMOOTH, L.steps)
        self._cache = {}


def check_map(A, agg, nc, passes):
    """what every map level -> level + 1 must be, whoever made it: a partition of the rows into nc aggregates of at most 2^passes
    rows, numbered in the order of their smallest members, each connected in the graph of A"""
    A = sp.csr_matrix(A)
    agg = np.asarray(agg, np.int64)
    n = A.shape[0]
    assert agg.shape == (n,) and agg.min() >= 0 and agg.max() < nc
    sizes = np.bincount(agg, minlength=nc)
    assert sizes.min() >= 1 and sizes.max() <= 2 ** passes, (sizes.min(), sizes.max())
    first = np.full(nc, n, np.int64)
    np.minimum.at(first, agg, np.arange(n))
    assert np.all(np.diff(first) > 0), "coarse ids must ascend with the smallest member"
    r = np.repeat(np.arange(n), np.diff(A.indptr))
    inside = agg[r] == agg[A.indices]
    G = sp.csr_matrix((np.ones(inside.sum()), (r[inside], A.indices[inside])), shape=(n, n))
    parts, _ = sp.csgraph.connected_components(G, directed=False)
    assert parts == nc, "an aggregate is not connected"


# ---- the systems of the tests -----------------------------------------------------------------------------------------------------------
def zaniso(nx, ny, nz, factor=100.0):
    """7-point Laplacian whose z-coupling is `factor` times the x- and y-coupling, integer-valued"""
    def t(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr") if m > 1 else sp.csr_matrix([[2.0]])
    Ix, Iy, Iz = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    A = sp.csr_matrix(sp.kron(Iz, sp.kron(Iy, t(nx))) + sp.kron(Iz, sp.kron(t(ny), Ix)) + factor * sp.kron(t(nz), sp.kron(Iy, Ix)))
    A.sort_indices()
    return A


def permuted(A, seed=5):
    """P A P^T for a seeded random permutation, columns sorted"""
    perm = np.random.default_rng(seed).permutation(A.shape[0])
    B = sp.csr_matrix(sp.csr_matrix(A)[perm][:, perm])
    B.sort_indices()
    return B


def graph_laplacian(n=2000, neighbours=6, seed=7):
    """seeded random graph Laplacian: `neighbours` random neighbours per row, symmetrised, unit weights, diagonal = degree + 0.1"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), neighbours)
    c = rng.integers(0, n, n * neighbours)
    keep = r != c
    G = sp.csr_matrix((np.ones(keep.sum()), (r[keep], c[keep])), shape=(n, n))
    G = sp.csr_matrix(((G + G.T) > 0).astype(np.float64))
    deg = np.asarray(G.sum(axis=1)).ravel()
    A = sp.csr_matrix(sp.diags(deg + 0.1) - G)
    A.sort_indices()
    return A


def arrowhead(n=300):
    """a star: row 0 coupled to every other row, nothing else"""
    A = sp.lil_matrix((n, n))
    A.setdiag(np.full(n, 4.0))
    A[0, 1:] = -0.01
    A[1:, 0] = -0.01
    A[0, 0] = 8.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def diagonal(n=300):
    return sp.csr_matrix(sp.diags(np.linspace(1.0, 2.0, n)))


def positive_tridiagonal(n=300):
    A = sp.csr_matrix(sp.diags([0.5 * np.ones(n - 1), 2 * np.ones(n), 0.5 * np.ones(n - 1)], [-1, 0, 1]))
    A.sort_indices()
    return A


def pcg_count(A, b, solve, tol, maxit=500):
    """iterations of PCG in double until sqrt(r.r) < tol, the preconditioner a function z = solve(r) (None: plain CG)"""
    A = sp.csr_matrix(A).astype(np.float64)
    x = np.zeros_like(b, dtype=np.float64)
    r = b.astype(np.float64).copy()
    z = solve(r) if solve else r
    p = z.copy()
    rz = r @ z
    for it in range(1, maxit + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.sqrt(r @ r) < tol:
            return it
        z = solve(r) if solve else r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return maxit
