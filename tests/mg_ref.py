"""Host restatement of the aggregation multigrid preconditioner (cgamd_solver_set_preconditioner_multigrid; include/cgamd.h and
DESIGN.md section 4 state the algorithm): the aggregate map, the Galerkin product P^T A P, the Chebyshev-Jacobi smoother and the
V-cycle, in a chosen arithmetic.

What the device holds is restated as the device holds it -- the level matrices and 1 / diag rounded once to the value type, lmax
in double, the smoother coefficients computed in double and rounded to the real type -- and `arith` picks the arithmetic of the
cycle itself: the value type (the yardstick of the device's rounding error) or np.longdouble / np.clongdouble (the exact cycle of
those inputs).  Sums run in the documented order: fine rows ascending, entries in stored order."""
import numpy as np
import scipy.sparse as sp

MAX_LEVELS = 16
KAPPA_SMOOTH, KAPPA_COARSEST, COARSEST_STEPS = 4.0, 30.0, 8


def wide(dtype, extended=False):
    cplx = np.dtype(dtype).kind == "c"
    if extended:
        return np.clongdouble if cplx else np.longdouble
    return np.complex128 if cplx else np.float64


def real_of(dtype):
    return np.empty(0, dtype).real.dtype.type


def coarse_dims(dims):
    return tuple((int(d) + 1) // 2 for d in dims)


def agg_map(dims):
    """agg[i] of every fine node, x fastest: (x, y, z) -> (x >> 1, y >> 1, z >> 1) on the grid of coarse_dims"""
    nx, ny, nz = (int(d) for d in dims)
    cnx, cny, _ = coarse_dims(dims)
    i = np.arange(nx * ny * nz, dtype=np.int64)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    return (x >> 1) + cnx * ((y >> 1) + cny * (z >> 1))


def galerkin(A, dims, dtype):
    """P^T A P of a CSR matrix with piecewise-constant P: entry (I, J) sums the fine entries (i, j) with agg(i) = I, agg(j) = J,
    fine rows ascending and entries in stored order (np.add.at adds in sequence), in double / complex double, rounded once to
    dtype.  Columns ascending, structural zeros kept.  Returns (csr, sum of |terms| per entry in double)."""
    A = sp.csr_matrix(A)
    agg = agg_map(dims)
    nc = int(np.prod(coarse_dims(dims)))
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    key = agg[rows] * nc + agg[A.indices]
    uniq, inv = np.unique(key, return_inverse=True)
    W = wide(dtype)
    acc, mag = np.zeros(uniq.size, W), np.zeros(uniq.size, np.float64)
    np.add.at(acc, inv, A.data.astype(W))
    np.add.at(mag, inv, np.abs(A.data.astype(W)))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(uniq // nc, minlength=nc))])
    Ac = sp.csr_matrix((acc.astype(dtype), (uniq % nc).astype(np.int32), ptr.astype(np.int32)), shape=(nc, nc))
    return Ac, mag


def chebyshev_coefficients(lmax, kappa, steps):
    """(c0[k], c1[k]) of step k on [lmax / kappa, lmax], in double: d = c0 d + c1 dinv (b - A x); c0[0] is unused"""
    lmin = lmax / kappa
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    c0, c1 = [0.0], [1.0 / theta]
    for _ in range(1, steps):
        rho_k = 1.0 / (2.0 * sigma - rho)
        c0.append(rho_k * rho)
        c1.append(2.0 * rho_k / delta)
        rho = rho_k
    return c0, c1


class Level:
    pass


class Hierarchy:
    def __init__(self, A, dims, dtype, smooth_steps=1, over_correction=1.6, min_rows=512):
        self.dtype = np.dtype(dtype)
        self.omega, self.steps = float(over_correction), int(smooth_steps)
        dims = tuple(int(d) for d in dims) + (1,) * (3 - len(dims))
        A = sp.csr_matrix(A).astype(self.dtype)
        assert A.shape[0] == int(np.prod(dims))
        self.levels = []
        while True:
            L = Level()
            L.A, L.dims, L.n = A, dims, A.shape[0]
            W = wide(self.dtype)
            Aw = A.astype(W)
            diag = Aw.diagonal()
            if np.any(diag == 0) or not np.all(np.isfinite(diag)):
                raise ZeroDivisionError(f"level {len(self.levels)}: zero, missing or non-finite diagonal in row "
                                        f"{int(np.flatnonzero((diag == 0) | ~np.isfinite(diag))[0])}")
            L.dinv = (W(1) / diag).astype(self.dtype)
            absA = sp.csr_matrix((np.abs(Aw.data), A.indices, A.indptr), shape=A.shape)
            L.lmax = float(np.max(np.abs(L.dinv.astype(W)) * np.asarray(absA @ np.ones(L.n))))
            self.levels.append(L)
            if L.n <= min_rows or len(self.levels) == MAX_LEVELS or int(np.prod(coarse_dims(dims))) >= L.n:
                break
            L.agg = agg_map(dims)
            A, L.mag = galerkin(A, dims, self.dtype)
            dims = coarse_dims(dims)
        for l, L in enumerate(self.levels):
            last = l == len(self.levels) - 1
            L.steps = COARSEST_STEPS if last else self.steps
            L.c0, L.c1 = chebyshev_coefficients(L.lmax, KAPPA_COARSEST if last else KAPPA_SMOOTH, L.steps)
        self._cache = {}

    def _in(self, W):
        """the inputs of the cycle in arithmetic W: what the device holds (value type / real type), represented in W"""
        key = np.dtype(W).name
        if key not in self._cache:
            R, Rv = real_of(W), real_of(self.dtype)
            self._cache[key] = [(L.A.astype(W), L.dinv.astype(W), [R(Rv(c)) for c in L.c0], [R(Rv(c)) for c in L.c1])
                                for L in self.levels], R(Rv(self.omega))
        return self._cache[key]

    def smooth(self, l, b, x, W):
        """S(b, x) on level l; x = None: from zero (no product in the first step)"""
        A, dinv, c0, c1 = self._in(W)[0][l]
        d = None
        for k in range(self.levels[l].steps):
            res = b if x is None else b - A @ x
            t = c1[k] * (dinv * res)
            d = t if k == 0 else c0[k] * d + t
            x = d.copy() if x is None else x + d
        return x

    def vcycle(self, r, arith=None, l=0):
        """z = M^-1 r for one vector, every operation in `arith` (default: the value type)"""
        W = np.dtype(arith or self.dtype).type
        b = np.asarray(r).astype(W)
        x = self.smooth(l, b, None, W)
        if l == len(self.levels) - 1:
            return x
        L = self.levels[l]
        A = self._in(W)[0][l][0]
        res = b - A @ x
        bc = np.zeros(self.levels[l + 1].n, W)
        np.add.at(bc, L.agg, res)             # in sequence: fine rows ascending
        e = self.vcycle(bc, W, l + 1)
        x = x + self._in(W)[1] * e[L.agg]
        return self.smooth(l, b, x, W)

    def solve(self, arith=None):
        """z = solve(r) for tridiag_pcg.pcg_sparse(..., solve=): that loop runs in complex; a real cycle is linear over the reals"""
        W = np.dtype(arith or wide(self.dtype))

        def f(r):
            if W.kind == "c":
                return self.vcycle(r, W).astype(complex)
            return self.vcycle(np.real(r), W).astype(float) + 1j * self.vcycle(np.imag(r), W).astype(float)
        return f


def laplace3d(nx, ny, nz):
    def t(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr") if m > 1 else sp.csr_matrix([[2.0]])
    Ix, Iy, Iz = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    A = sp.kron(Iz, sp.kron(Iy, t(nx))) + sp.kron(Iz, sp.kron(t(ny), Ix)) + sp.kron(t(nz), sp.kron(Iy, Ix))
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def variable7(nx, ny, nz, seed=3):
    """variable-coefficient 7-point matrix: D^(1/2) (Laplacian + shift) D^(1/2) with a random positive diagonal scaling, SPD"""
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    s = sp.diags(np.sqrt(rng.uniform(0.5, 2.0, n)))
    A = sp.csr_matrix(s @ (laplace3d(nx, ny, nz) + sp.diags(rng.uniform(0.0, 0.5, n))) @ s)
    A.sort_indices()
    return A


def stencil27(nx, ny, nz):
    """27-point matrix (9-point in 2-D, 3-point in 1-D): sum over the axes of Kronecker products with one [-1, 2, -1] stiffness
    factor and [1, 4, 1] mass factors"""
    def k(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr") if m > 1 else sp.csr_matrix([[2.0]])

    def m_(m):
        return sp.diags([np.ones(m - 1), 4 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csr") if m > 1 else sp.csr_matrix([[4.0]])
    Kx, Ky, Kz, Mx, My, Mz = k(nx), k(ny), k(nz), m_(nx), m_(ny), m_(nz)
    A = sp.kron(Mz, sp.kron(My, Kx)) + sp.kron(Mz, sp.kron(Ky, Mx)) + sp.kron(Kz, sp.kron(My, Mx))
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A
