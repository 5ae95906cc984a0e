"""Restatement of the reference PCG's sparse-M branch (helmFE_var.py:546-586, `M.nnz > n`: z = spsolve(M, r)) for the
tridiagonal-preconditioner tests, plus the test systems they share.  Unconjugated dots, stop on sqrt(|r.r|) < tol after the
update, returns (x, i) with i the index of the last iteration run -- the reference's return value.

Below it, the sweep z = M^-1 r as an operation of its own: an extended-precision solve (thomas_ext), the same two sweeps done
sequentially in the value type (sweep_in_type: the yardstick of the tolerance), the segment rule restated (segments) and the
per-segment checker (check_sweep)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def pcg_sparse(A, b, M, x0=None, tol=1e-6, maxit=1000, history=False, solve=None, residual=False):
    """solve: optional z = solve(r) in place of spsolve(M, r) (e.g. a factorisation made once with splu); residual: return
    (x, i, history, r) with r the recurrence's own residual after the last iteration run"""
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
    if residual:
        return x, i, np.asarray(hist), r
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


# ---- the sweep z = M^-1 r on its own -----------------------------------------------------------------------------------------
# M is given as the library takes it: lower[i] = M[i][i - stride], diag[i] = M[i][i], upper[i] = M[i][i + stride] (entries that
# would leave the matrix are ignored); r is (nrhs, n).  A chain is the rows c, c + stride, c + 2 stride, ...

def _wide(dtype, extended):
    cplx = np.dtype(dtype).kind == "c"
    if extended:
        return np.clongdouble if cplx else np.longdouble
    return np.complex128 if cplx else np.float64


def _factors(lower, diag, upper, stride, W):
    """Thomas LU without pivoting along every chain, every operation in W: per row (-l, -w c, w) with l_i = a_i / u_(i-stride),
    u_i = b_i - l_i c_(i-stride), w_i = 1 / u_i -- the three arrays the kernels read (cgamd_solver_set_preconditioner_tridiag)"""
    n, s = len(diag), int(stride)
    a, b, c = np.array(lower, dtype=W), np.array(diag, dtype=W), np.array(upper, dtype=W)
    a[:s] = 0
    c[n - s:] = 0
    nl, ne, w = np.zeros(n, W), np.zeros(n, W), np.zeros(n, W)
    if s == 1:                     # one chain: scalars of type W, row by row
        u_prev, c_prev, out = W(1), W(0), []
        for ai, bi, ci in zip(a, b, c):
            l = ai / u_prev
            u_prev = bi - l * c_prev
            wi = W(1) / u_prev
            out.append((-l, -(wi * ci), wi))
            c_prev = ci
        nl[:], ne[:], w[:] = (np.array(col, dtype=W) for col in zip(*out))
        return nl, ne, w
    u_prev, c_prev = np.ones(s, W), np.zeros(s, W)
    for k in range(0, n, s):       # every chain's next row at once
        m = min(s, n - k)
        l = a[k:k + m] / u_prev[:m]
        u = b[k:k + m] - l * c_prev[:m]
        wi = W(1) / u
        nl[k:k + m], ne[k:k + m], w[k:k + m] = -l, -(wi * c[k:k + m]), wi
        u_prev[:m], c_prev[:m] = u, c[k:k + m]
    return nl, ne, w


def _recurrence(a, b, stride, reverse=False):
    """v_i = a_i v_(i - stride) + b_i along every chain (reverse: v_(i + stride), from the chain's last row), sequentially, one
    multiplication and one addition per row, each rounded once to the arrays' own type; b and the result are (nrhs, n)"""
    nrhs, n = b.shape
    s = int(stride)
    v = np.empty_like(b)
    if s == 1:
        step = -1 if reverse else 1
        for r in range(nrhs):
            p, out = b.dtype.type(0), []
            for ai, bi in zip(a[::step], b[r, ::step]):
                p = ai * p + bi
                out.append(p)
            v[r, ::step] = np.array(out, dtype=b.dtype)
        return v
    p = np.zeros((nrhs, s), b.dtype)
    starts = range(0, n, s)
    for k in (reversed(starts) if reverse else starts):
        m = min(s, n - k)
        p[:, :m] = a[k:k + m] * p[:, :m] + b[:, k:k + m]
        v[:, k:k + m] = p[:, :m]
    return v


def thomas_ext(lower, diag, upper, r, stride=1):
    """z with M z = r in np.longdouble / np.clongdouble (factorisation and both sweeps): the exact solve, for every value type, of
    the inputs as given -- pass the diagonals and r as rounded to the handle's value type, which is what the device receives"""
    W = _wide(np.result_type(np.asarray(diag).dtype, np.asarray(r).dtype), True)
    nl, ne, w = _factors(lower, diag, upper, stride, W)
    y = _recurrence(nl, np.atleast_2d(np.asarray(r)).astype(W), stride)
    return _recurrence(ne, w * y, stride, reverse=True)


def sweep_in_type(lower, diag, upper, r, dtype, stride=1):
    """the two sweeps done sequentially in the value type: the factors -l, -w c, w computed in double / complex double and
    rounded to the type (tri_factor), then y_i = (-l_i) y_prev + r_i and z_i = (-w_i c_i) z_next + w_i y_i with one rounding per
    operation and no FMA (the library is built with -ffp-contract=off).  Not the kernels' order: the yardstick of their error"""
    dtype = np.dtype(dtype)
    nl, ne, w = (f.astype(dtype) for f in _factors(lower, diag, upper, stride, _wide(dtype, False)))
    y = _recurrence(nl, np.atleast_2d(np.asarray(r)).astype(dtype), stride)
    return _recurrence(ne, w * y, stride, reverse=True)


def segments(lower, diag, upper, dtype, stride=1):
    """the segments the chains fall into, by the documented rule (include/cgamd.h): row i starts one when it heads its
    chain (i < stride) or when BOTH stored couplings to row i - stride, -l_i and -w c of row i - stride, round to zero in the
    value type; a one-sided zero does not cut.  Returns an (nsegs, 3) array of (first row, length, stride) ordered by first row"""
    dtype = np.dtype(dtype)
    n, s = len(diag), int(stride)
    nl, ne, _ = (f.astype(dtype) for f in _factors(lower, diag, upper, s, _wide(dtype, False)))
    start = np.ones(n, bool)
    start[s:] = (nl[s:] == 0) & (ne[:n - s] == 0)
    chain_major = np.argsort(np.arange(n) % s, kind="stable")          # chain 0's rows in order, then chain 1's, ...
    at = np.flatnonzero(start[chain_major])                             # every chain's head is a start
    out = np.stack([chain_major[at], np.diff(np.append(at, n)), np.full(at.size, s)], axis=1).astype(np.int64)
    return out[np.argsort(out[:, 0])]


def sweep_error(z, z_ref, segs):
    """e(z) = max over segments of max_i |z_i - z_ref,i| / max_i |z_ref,i| for one right-hand side: every line is measured on its
    own scale.  A segment whose reference is all zero must be reproduced exactly."""
    first, length, stride = segs[:, 0], segs[:, 1], segs[:, 2]
    at = np.concatenate([[0], np.cumsum(length)[:-1]])
    rows = np.repeat(first, length) + (np.arange(length.sum()) - np.repeat(at, length)) * np.repeat(stride, length)
    assert np.array_equal(np.sort(rows), np.arange(len(z_ref))), "the segments must cover every row once"
    z_ref = np.asarray(z_ref)
    num = np.maximum.reduceat(np.abs(np.asarray(z).astype(z_ref.dtype) - z_ref)[rows], at)
    den = np.maximum.reduceat(np.abs(z_ref)[rows], at)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den == 0, np.where(num == 0, 0.0, np.inf), num / den)
    return float(np.max(e)) if np.all(e == e) else float("nan")


def check_sweep(z, z_ref, z_seq, segs, dtype, label=""):
    """a computed z = M^-1 r against the extended-precision z_ref, per right-hand side and per segment:
        e(z) <= 4 max(e(z_seq), 4 eps(dtype))
    with z_seq the sequential sweep in the same arithmetic (sweep_in_type).  The bound never looks at the code under test; the
    factor 4 is room over the 0.45x to 1.52x that a restatement of the kernels' scan order (per-thread maps, 64-lane scan, wave
    totals, chunk carries) measured against the sequential sweep on reasonably conditioned chains.  Both figures are
    printed before the assertion; returns them per right-hand side."""
    eps = float(np.finfo(np.dtype(dtype)).eps)
    z, z_ref, z_seq = np.atleast_2d(z), np.atleast_2d(z_ref), np.atleast_2d(z_seq)
    assert z.shape == z_ref.shape == z_seq.shape, (z.shape, z_ref.shape, z_seq.shape)
    figures = []
    for r in range(z_ref.shape[0]):
        e_dev, e_seq = sweep_error(z[r], z_ref[r], segs), sweep_error(z_seq[r], z_ref[r], segs)
        bound = 4.0 * max(e_seq, 4.0 * eps)
        print(f"  sweep {label} {np.dtype(dtype).name} rhs {r}: {len(segs)} segments, e(z) {e_dev:.3e}, e(z_seq) {e_seq:.3e}, "
              f"ratio {e_dev / e_seq if e_seq > 0 else float('inf'):.2f}, bound {bound:.3e}")
        figures.append((e_dev, e_seq))
    for r, (e_dev, e_seq) in enumerate(figures):
        assert e_dev <= 4.0 * max(e_seq, 4.0 * eps), (label, np.dtype(dtype).name, r, e_dev, e_seq)
    return figures
