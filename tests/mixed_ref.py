"""The mixed-precision CG of include/cgamd.h ("Mixed precision", cgamd_mixed_solve) restated in numpy, one right-hand side: the
recurrence in float32 / complex64 with its sums taken in double, x and the true residual in float64 / complex128, residual
replacement with the search direction kept.  It is the scheme, step for step, not the device's bits: the order of the sums and the
SpMV's accumulation differ.  What it serves: the iteration counts and the reach of the scheme on the host (test_abi_mixed.py), and
the systems the device tests run on.

Also here: the test systems (5-point Poisson on nx x ny, 7-point on nx x ny x nz, x fastest, Dirichlet) as CSR arrays, and a CSR
product with the row sums in a chosen type."""
import numpy as np


def poisson2d_rect(nx, ny):
    """5-point Laplacian on an nx x ny grid (x fastest), diag 4 / off-diag -1: (indptr, indices, data float64), columns ascending"""
    return _stencil((nx, ny))


def poisson3d(nx, ny, nz):
    """7-point Laplacian on nx x ny x nz (x fastest), diag 6 / off-diag -1"""
    return _stencil((nx, ny, nz))


def _stencil(dims):
    n = int(np.prod(dims))
    idx = np.arange(n)
    coords, stride, strides = [], 1, []
    for d in dims:
        coords.append((idx // stride) % d)
        strides.append(stride)
        stride *= d
    cols, vals = [idx], [np.full(n, 2.0 * len(dims))]
    valid = [np.ones(n, bool)]
    for c, d, st in zip(coords, dims, strides):
        for sign in (-1, 1):
            ok = (c + sign >= 0) & (c + sign < d)
            cols.append(idx + sign * st)
            vals.append(np.full(n, -1.0))
            valid.append(ok)
    cols, vals, valid = np.stack(cols, 1), np.stack(vals, 1), np.stack(valid, 1)
    order = np.argsort(np.where(valid, cols, n + 1), axis=1, kind="stable")
    cols, vals, valid = (np.take_along_axis(a, order, 1) for a in (cols, vals, valid))
    indptr = np.concatenate(([0], np.cumsum(valid.sum(1)))).astype(np.int32)
    return indptr, cols[valid].astype(np.int32), vals[valid].astype(np.float64)


def csr_matvec(indptr, indices, data, x, acc=None):
    """y = A x, products in the type of data * x, every row summed in `acc` (default: that type), rounded once to the product type.
    Rows must not be empty."""
    prod = data * x[indices]
    out = prod.dtype
    if acc is not None:
        prod = prod.astype(acc)
    return np.add.reduceat(prod, indptr[:-1]).astype(out)


def _acc(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def _dot(a, b):
    """unconjugated a.b summed in double / complex double"""
    acc = _acc(a.dtype)
    return np.sum(a.astype(acc) * b.astype(acc))


def mixed_cg(indptr, indices, data, b, x0=None, tol=1e-10, maxit=1000, delta=0.1, max_segment=0, m_lo=None):
    """cgamd_mixed_solve for one right-hand side.  data, b, x0: float64 or complex128; m_lo: the diagonal preconditioner of the
    inner handle (float32 / complex64 values that multiply r) or None.  Returns (x, info) with info a dict of iterations,
    replacements, resnorm (sqrt|r.r| of the true residual of x), status (0 / 1 / 2) and scale."""
    hi = np.dtype(data.dtype)
    lo = np.dtype(np.complex64 if hi.kind == "c" else np.float32)
    a_lo = data.astype(lo)
    x = np.zeros(b.shape, hi) if x0 is None else np.array(x0, dtype=hi)
    its = repl = 0
    status, scale, d = 1, 1.0, None
    while True:
        r = b - csr_matvec(indptr, indices, data, x)
        res = float(np.sqrt(abs(np.sum(r * r))))
        if not res >= tol:
            status = 2 if np.isnan(res) else 0
            break
        if not np.isfinite(res):
            status = 2
            break
        if its >= maxit:
            break
        if d is None:
            nrm = float(np.sqrt(np.sum(np.abs(r) ** 2)))
            scale = float(np.ldexp(1.0, int(np.frexp(nrm)[1]) - 1)) if np.isfinite(nrm) and nrm > 0 else 1.0       # 2^ilogb
        rl = (r * (1.0 / scale)).astype(lo)
        xl = np.zeros_like(rl)
        z = rl if m_lo is None else (m_lo * rl).astype(lo)
        if d is None:
            d = z.copy()                                # the first segment: set_rhs; later ones keep the direction
        rho = lo.type(_dot(rl, z))
        start = float(np.sqrt(abs(lo.type(_dot(rl, rl)))))
        t = max(delta * start, tol / scale)
        seg = maxit - its if max_segment <= 0 else min(max_segment, maxit - its)
        for _ in range(seg):
            q = csr_matvec(indptr, indices, a_lo, d, _acc(lo))
            alpha = lo.type(_acc(lo)(rho) / _dot(d, q))
            xl = (xl + alpha * d).astype(lo)
            rl = (rl - alpha * q).astype(lo)
            z = rl if m_lo is None else (m_lo * rl).astype(lo)
            rho_new = lo.type(_dot(rl, z))
            dn = lo.type(_dot(rl, rl))
            beta = lo.type(_acc(lo)(rho_new) / _acc(lo)(rho))
            rho = rho_new
            d = (z + beta * d).astype(lo)
            its += 1
            if not float(np.sqrt(abs(dn))) >= t:
                break
        x = x + scale * xl.astype(hi)
        repl += 1
    return x, {"iterations": its, "replacements": repl, "resnorm": res, "status": status, "scale": scale}


def cg_hi(indptr, indices, data, b, tol, maxit):
    """plain CG in the type of data, stopped on sqrt|r.r| < tol: the iteration count the mixed solve is held against"""
    x = np.zeros_like(b)
    r = b.copy()
    d = r.copy()
    delta = np.sum(r * r)
    for k in range(1, maxit + 1):
        q = csr_matvec(indptr, indices, data, d)
        alpha = delta / np.sum(d * q)
        x = x + alpha * d
        r = r - alpha * q
        dn = np.sum(r * r)
        if not float(np.sqrt(abs(dn))) >= tol:
            return x, k
        d = r + (dn / delta) * d
        delta = dn
    return x, maxit
