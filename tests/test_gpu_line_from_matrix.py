"""Preconditioners built on the device from the handle's own matrix: Solver.set_preconditioner(("line", stride)) /
cgamd_solver_set_preconditioner_line (M = the entries of A at column - row in {-stride, 0, +stride}, extracted, factored and planned
by precond_build.hip) and Solver.set_preconditioner("jacobi") / cgamd_solver_set_preconditioner_jacobi.  The oracle is the restated
reference PCG (tridiag_pcg.pcg_sparse with M factored once by splu); systems, right-hand sides and tolerances are those of
test_gpu_tridiag_strided (tols, and its `keep` rule for history entries).  No bit-equality is asked between the device-built
factors and those of the array entries (the host divides through complex arithmetic); the device path is bit-stable against
itself."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import tridiag_pcg as tp

pytestmark = pytest.mark.gpu


def parts(A, dtype):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(dtype)


def solver(pkg, ctx, A, dtype, nrhs=1, flags=0):
    ip, ix, da = parts(A, dtype)
    return pkg.Solver(ctx, A.shape[0], len(ix), da, ip, ix, nrhs, flags=flags)


def laplace3d(nx, ny, nz, cx=1.0, cy=1.0, cz=1.0):
    """7-point Laplacian on nx x ny x nz nodes (x fastest) with a coupling factor per axis"""
    def t(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")
    Ix, Iy, Iz = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    A = cx * sp.kron(Iz, sp.kron(Iy, t(nx))) + cy * sp.kron(Iz, sp.kron(t(ny), Ix)) + cz * sp.kron(t(nz), sp.kron(Iy, Ix))
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def lines(A, s):
    """M: the entries of A at |i - j| in {0, s}"""
    c = sp.coo_matrix(A)
    d = np.abs(c.row.astype(np.int64) - c.col)
    keep = (d == 0) | (d == s)
    return sp.csr_matrix((c.data[keep], (c.row[keep], c.col[keep])), shape=A.shape)


def three(M, s, dtype, n):
    lower, diag, upper = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    diag[:] = M.diagonal(0)
    lower[s:] = M.diagonal(-s)
    upper[:n - s] = M.diagonal(s)
    return lower, diag, upper


def cut_system(rng, n, s, ncuts):
    """diagonal 5.5 + U(0, 1), couplings -U(0.2, 1) at distance s (ncuts of them zeroed) and -0.8 at distances 1 and 5"""
    off = -rng.uniform(0.2, 1.0, n - s)
    if ncuts:
        off[rng.choice(n - s, size=ncuts, replace=False)] = 0.0
    near, five = -0.8 * np.ones(n - 1), -0.8 * np.ones(n - 5)
    A = sp.diags([off, five, near, 5.5 + rng.uniform(0.0, 1.0, n), near, five, off], [-s, -5, -1, 0, 1, 5, s], format="csr")
    A.eliminate_zeros()
    return A


def lu_solve(M):
    lu = spla.splu(sp.csc_matrix(M))
    if np.iscomplexobj(M.data):
        return lambda r: lu.solve(r)
    return lambda r: lu.solve(r.real) + 1j * lu.solve(r.imag)


def tols(dtype):
    return (1e-9, 1e-10) if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-4)


def oracle(A, M, B, iters):
    """the restated reference PCG per right-hand side, M factored once: [(x, history)]"""
    solve = lu_solve(M)
    out = []
    for r in range(B.shape[0]):
        xo, _, ho = tp.pcg_sparse(A, B[r].astype(complex), M, tol=0.0, maxit=iters, history=True, solve=solve)
        out.append((xo, ho))
    return out


def check_run(x, h, ref, dtype, label=""):
    """x / history of a device run against [(x, history)] per right-hand side; every figure is printed before it is asserted"""
    xt, ht = tols(dtype)
    n = ref[0][0].size
    for r, (xo, ho) in enumerate(ref):
        keep = np.abs(ho) / np.abs(ho[0]) > (1e-8 if xt < 1e-6 else 1e-4)     # reduction-order noise only while not converged
        herr = np.max(np.abs(h[keep, r] - ho[keep]) / np.abs(ho[keep]))
        xr = x[r * n:(r + 1) * n]
        xerr = np.linalg.norm(xr - xo) / np.linalg.norm(xo)
        print(f"  {label} n={n} {np.dtype(dtype).name} rhs {r}: {int(keep.sum())} history entries compared, history err "
              f"{herr:.3e} (< {ht:g}), x err {xerr:.3e} (< {xt:g})")
        assert herr < ht, (label, r, dtype, herr)
        assert xerr < xt, (label, r, dtype, xerr)


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


GRIDS = [(24, 21, 17), (23, 21, 17)]
_parity_ref = {}


def parity_system(grid, axis, cplx):
    """the systems, right-hand sides and oracle runs of test_gpu_tridiag_strided's parity test (x-lines added), made once"""
    key = (grid, axis, cplx)
    if key not in _parity_ref:
        nx, ny, nz = grid
        n = nx * ny * nz
        s = {"x": 1, "y": nx, "z": nx * ny}[axis]
        A = laplace3d(nx, ny, nz, **{"c" + axis: 10.0})
        if cplx:
            A = sp.csr_matrix(A * (1.0 + 0.05j))
        M = tp.band(A) if s == 1 else lines(A, s)
        rng = np.random.default_rng(11)
        B = rng.standard_normal((3, n))
        if cplx:
            B = B * (1.0 + 0.3j * rng.standard_normal((3, n)))      # phase-controlled: |b.b| stays near 0.8 b^H b
        _parity_ref[key] = (A, M, B, s, oracle(A, M, B, 12))
    return _parity_ref[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_line_parity_x_y_and_z_lines(pkg, gpu, dtype, grid, axis):
    """strides 1, nx and nx ny, every value type, 3 right-hand sides, 12 iterations; 23 x 21 x 17 has an odd row count (padding
    rows).  Built from the matrix on the device (source 2), then the same handle with the arrays cut by numpy (source 1): both
    against scipy PCG, the same loop"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    A, M, B, s, ref = parity_system(grid, axis, np.dtype(dtype).kind == "c")
    sv = solver(pkg, ctx, A, dtype, nrhs=3)
    assert sv.preconditioner_source == 0
    sv.set_preconditioner(("line", s))
    assert sv.preconditioner_source == 2
    launches = lib.cgamd_solver_loop_launches(sv.handle)
    x, h = sv.solve(B.reshape(-1).astype(dtype), None, 12)
    sv.set_preconditioner(M)
    assert sv.preconditioner_source == 1
    launches1 = lib.cgamd_solver_loop_launches(sv.handle)
    x1, h1 = sv.solve(B.reshape(-1).astype(dtype), None, 12)
    sv.close()
    assert launches == launches1 == 4
    check_run(x, h, ref, dtype, "from the matrix")
    check_run(x1, h1, ref, dtype, "from arrays")


def test_line_variable_coefficients_unsorted_columns_duplicates(pkg, gpu):
    """fp64, 120 000 rows at stride 37 with 300 cuts (segments of one row to thousands, chains of unequal length: 120 000 is no
    multiple of 37); every row's entries in random order, one diagonal entry and one stride-37 entry stored as two entries that sum
    to the original; 8 iterations against splu"""
    ctx, _, _ = gpu
    rng = np.random.default_rng(5)
    n, s = 120_000, 37
    A = cut_system(rng, n, s, 300)
    M = lines(A, s)
    B = rng.standard_normal((1, n))
    c = sp.coo_matrix(A)
    row, col, val = c.row.astype(np.int64), c.col.astype(np.int64), c.data.copy()
    for r, cc in ((1234, 1234), (50_000, 50_000 + s)):
        at = np.flatnonzero((row == r) & (col == cc))
        assert at.size == 1 and val[at[0]] != 0
        v = val[at[0]]
        val[at[0]] = 0.25 * v
        row, col, val = np.append(row, r), np.append(col, cc), np.append(val, v - 0.25 * v)
    order = np.lexsort((rng.random(row.size), row))       # rows in order, the entries of a row shuffled
    row, col, val = row[order], col[order], val[order]
    ip = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(row, minlength=n), out=ip[1:])
    assert np.any(np.diff(col[ip[7]:ip[8]]) < 0) or np.any(np.diff(col[ip[8]:ip[9]]) < 0)
    sv = pkg.Solver(ctx, n, len(col), val, ip, col.astype(np.int32), 1)
    sv.set_preconditioner(("line", s))
    assert sv.preconditioner_source == 2
    assert pkg._lib.load().cgamd_solver_loop_launches(sv.handle) == 4
    x, h = sv.solve(B.reshape(-1), None, 8)
    sv.close()
    check_run(x, h, oracle(A, M, B, 8), np.float64)


def test_line_many_short_segments(pkg, gpu):
    """fp64, 540 000 rows at stride 3, every coupling (i, i + 3) with (i // 3) % 2 == 1 zeroed: 270 000 segments of two rows, more
    than one segment per thread of the sweep's 1024 work-groups; 8 iterations against splu"""
    ctx, _, _ = gpu
    rng = np.random.default_rng(7)
    n, s = 540_000, 3
    off = -rng.uniform(0.2, 1.0, n - s)
    off[(np.arange(n - s) // 3) % 2 == 1] = 0.0
    near, five = -0.8 * np.ones(n - 1), -0.8 * np.ones(n - 5)
    A = sp.diags([off, five, near, 5.5 + rng.uniform(0.0, 1.0, n), near, five, off], [-s, -5, -1, 0, 1, 5, s], format="csr")
    A.eliminate_zeros()
    M = lines(A, s)
    assert np.count_nonzero(off) == 270_000               # one kept coupling per segment of two rows
    B = rng.standard_normal((1, n))
    sv = solver(pkg, ctx, A, np.float64)
    sv.set_preconditioner(("line", s))
    assert sv.preconditioner_source == 2
    x, h = sv.solve(B.reshape(-1), None, 8)
    sv.close()
    check_run(x, h, oracle(A, M, B, 8), np.float64)


def test_line_long_segments_and_the_host_route(pkg, gpu):
    """60 000 rows at stride 2 are two segments of 30 000 rows: whichever route the call takes (source 2 or 3), the result is within
    tolerance of splu.  dev.line_host_route = 1 forces the host route (source 3) on the 24 x 21 x 17 z-line system: within
    tolerance of the run built on the device"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    rng = np.random.default_rng(5)
    n, s = 60_000, 2
    A = cut_system(rng, n, s, 0)
    M = lines(A, s)
    B = rng.standard_normal((1, n))
    sv = solver(pkg, ctx, A, np.float64)
    sv.set_preconditioner(("line", s))
    print(f"  two segments of {n // 2} rows: source {sv.preconditioner_source}")
    assert sv.preconditioner_source in (2, 3)
    x, h = sv.solve(B.reshape(-1), None, 8)
    sv.close()
    check_run(x, h, oracle(A, M, B, 8), np.float64)

    A, M, B, s, ref = parity_system((24, 21, 17), "z", False)
    runs = {}
    for route in (0, 1):
        pkg._lib.check(lib.cgamd_tune(b"dev.line_host_route", route))       # a handle keeps the configuration it was created under
        try:
            sv = solver(pkg, ctx, A, np.float64, nrhs=3)
        finally:
            pkg._lib.check(lib.cgamd_tune(b"dev.line_host_route", 0))
        sv.set_preconditioner(("line", s))
        assert sv.preconditioner_source == (3 if route else 2)
        assert lib.cgamd_solver_loop_launches(sv.handle) == 4
        runs[route] = sv.solve(B.reshape(-1), None, 12)
        sv.close()
    n = A.shape[0]
    check_run(runs[1][0], runs[1][1], [(runs[0][0][r * n:(r + 1) * n], runs[0][1][:, r]) for r in range(3)], np.float64,
              "host route against device route")
    check_run(runs[1][0], runs[1][1], ref, np.float64, "host route")


def test_line_invariants(pkg, gpu):
    """bits: run to run, 15 + 15 = 30 iterations, graphs = plain launches, a borrowed device matrix = the owned one; removing M
    gives a fresh handle's bits; an array-form diagonal after it gives a diagonal-only handle's bits; launched loop only"""
    import torch
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    nx, ny, nz = 40, 30, 20
    A = laplace3d(nx, ny, nz, cz=10.0)
    n = A.shape[0]
    s = nx * ny
    b = np.linspace(1.0, 2.0, n)

    def run(flags=0, split=None, m=("line", s), borrowed=False):
        if borrowed:
            ip, ix, da = parts(A, np.float64)
            keep = [torch.from_numpy(a).to(torch.device("cuda", 0)) for a in (da, ip, ix)]
            torch.cuda.synchronize()
            sv = pkg.Solver(ctx, n, len(ix), keep[0], keep[1], keep[2], 1, flags=pkg._lib.MATRIX_ON_DEVICE | flags, dtype=np.float64)
        else:
            sv = solver(pkg, ctx, A, np.float64, flags=flags)
        sv.set_preconditioner(m)
        if isinstance(m, tuple):
            assert sv.preconditioner_source == 2
        sv.set_rhs(b)
        for k in split or (30,):
            sv.iterate(k)
        out = (sv.x(), sv.history())
        sv.close()
        return out

    first = run()
    assert same_bits(run(), first)
    assert same_bits(run(split=(15, 15)), first)
    assert same_bits(run(flags=pkg._lib.NO_GRAPH), first)
    assert same_bits(run(borrowed=True), first)

    sv = solver(pkg, ctx, A, np.float64)
    sv.set_preconditioner(("line", s))
    sv.set_rhs(b)
    assert lib.cgamd_solver_loop_launches(sv.handle) == 4
    its = ctypes.c_int(0)
    assert lib.cgamd_solver_iterate_tol(sv.handle, 10, 1e-6, ctypes.byref(its)) == pkg._lib.ERR_STATE
    # removal: the bits of a handle that never had a preconditioner
    sv.set_preconditioner(None)
    assert sv.preconditioner_source == 0
    sv.set_rhs(b)
    sv.iterate(30)
    removed = (sv.x(), sv.history())
    f = solver(pkg, ctx, A, np.float64)
    f.set_rhs(b)
    f.iterate(30)
    assert same_bits(removed, (f.x(), f.history()))
    assert lib.cgamd_solver_loop_launches(sv.handle) == lib.cgamd_solver_loop_launches(f.handle)
    f.close()
    # an array-form diagonal after the lines
    m = 1.0 / A.diagonal()
    sv.set_preconditioner(("line", s))
    sv.set_preconditioner(m)
    assert sv.preconditioner_source == 1
    sv.set_rhs(b)
    sv.iterate(30)
    after = (sv.x(), sv.history())
    sv.close()
    assert same_bits(after, run(m=m))


def test_line_and_jacobi_follow_reload_matrix(pkg, gpu):
    """an owned handle with the lines (or Jacobi) of its matrix, a solve, reload_matrix with the same pattern (cz = 3, scaled
    symmetrically by a diagonal), another solve: the bits of a fresh handle on the new matrix after the same call.  A preconditioner
    from the caller's arrays is kept across the reload, as before"""
    ctx, _, _ = gpu
    nx, ny, nz = 40, 30, 20
    n, s = nx * ny * nz, nx * ny
    A = laplace3d(nx, ny, nz, cz=10.0)
    D = sp.diags(1.0 + 0.1 * np.sin(np.arange(n)))
    A2 = sp.csr_matrix(D @ laplace3d(nx, ny, nz, cz=3.0) @ D)
    A2.sort_indices()
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    b = np.linspace(1.0, 2.0, n)
    ip2, ix2, da2 = parts(A2, np.float64)
    for m, source in ((("line", s), 2), ("jacobi", 2), (lines(A, s), 1)):
        sv = solver(pkg, ctx, A, np.float64)
        sv.set_preconditioner(m)
        before = sv.solve(b, None, 10)
        sv.reload_matrix(da2, ip2, ix2)
        assert sv.preconditioner_source == source
        got = sv.solve(b, None, 10)
        sv.close()
        f = solver(pkg, ctx, A2, np.float64)
        f.set_preconditioner(m)
        want = f.solve(b, None, 10)
        f.close()
        assert not same_bits(before, got)
        assert same_bits(got, want), m if not hasattr(m, "nnz") else "arrays"


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_jacobi_from_the_matrix(pkg, gpu, dtype):
    """"jacobi" against the array form given (1 / diag in double).astype(dtype): one correctly rounded double division and one
    rounding on both sides, so fp32 and fp64 agree to the bit; the complex types are held to tols"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    rng = np.random.default_rng(3)
    n = 30_000
    A = cut_system(rng, n, 37, 50)
    cplx = np.dtype(dtype).kind == "c"
    if cplx:
        A = sp.csr_matrix(A * (1.0 + 0.05j))
    b = rng.standard_normal(n).astype(dtype)
    diag = A.diagonal().astype(dtype)                    # as the handle holds it
    m = (1.0 / diag.astype(np.complex128 if cplx else np.float64)).astype(dtype)
    out, launches = [], []
    for form in ("jacobi", m):
        sv = solver(pkg, ctx, A, dtype)
        sv.set_preconditioner(form)
        assert sv.preconditioner_source == (2 if isinstance(form, str) else 1)
        launches.append(lib.cgamd_solver_loop_launches(sv.handle))
        out.append(sv.solve(b, None, 10))
        sv.close()
    assert launches[0] == launches[1]
    if cplx:
        check_run(out[0][0], out[0][1], [(out[1][0], out[1][1][:, 0])], dtype, "device 1/diag against numpy's")
    else:
        differ = np.flatnonzero(out[0][0] != out[1][0])
        print(f"  {np.dtype(dtype).name}: {differ.size} entries of x differ", out[0][0][differ[:4]], out[1][0][differ[:4]])
        assert same_bits(out[0], out[1])


def test_line_errors(pkg, gpu):
    """strides outside [1, size - 1]; a row without a stored diagonal (a chain's first row, where diagonal 0 is the pivot itself), a
    zero pivot (the construction of test_strided_errors) and a NaN: CGAMD_ERR_INVALID naming the row, of two bad rows in different
    chains the smaller one; the array-form Jacobi set before stays in force with its bits; "jacobi" names the row without a
    diagonal"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    nx, ny, nz = 40, 30, 20
    A = laplace3d(nx, ny, nz, cz=10.0)
    n = A.shape[0]
    s = nx * ny
    b = np.linspace(1.0, 2.0, n)
    ip, ix, da = parts(A, np.float64)
    rows = np.repeat(np.arange(n), np.diff(ip))

    def at(r, c):
        k = np.flatnonzero((rows == r) & (ix == c))
        assert k.size == 1
        return int(k[0])

    sv = solver(pkg, ctx, A, np.float64)
    for bad_stride in (0, -3, n, n + 1):
        assert lib.cgamd_solver_set_preconditioner_line(sv.handle, bad_stride) == pkg._lib.ERR_INVALID, bad_stride
    assert sv.preconditioner_source == 0
    sv.close()

    row, other = 7 + 3 * s, 11 + 2 * s                     # different chains, other < row
    head = 7                                               # heads its chain: u = the diagonal
    k = at(head, head)
    no_diag = (np.delete(da, k), ip - (np.arange(n + 1) > head).astype(np.int32), np.delete(ix, k))
    zero_pivot = da.copy()
    zero_pivot[[at(row, row), at(row, row - s)]] = 0.0    # stored zeros: u_row = 0
    nan = da.copy()
    nan[at(row, row + s)] = np.nan
    two = zero_pivot.copy()
    two[[at(other, other), at(other, other - s)]] = 0.0
    m = 1.0 / A.diagonal()
    for label, (v, p, c), named in (("no diagonal", no_diag, head), ("zero pivot", (zero_pivot, ip, ix), row),
                                    ("NaN", (nan, ip, ix), row), ("two bad rows", (two, ip, ix), other)):
        def make():
            h = pkg.Solver(ctx, n, len(c), v, p, c, 1)
            h.set_preconditioner(m)
            return h
        sv = make()
        with pytest.raises(pkg._lib.CgAmdError) as ei:
            sv.set_preconditioner(("line", s))
        print(f"  {label}: {ei.value}")
        assert ei.value.status == pkg._lib.ERR_INVALID, label
        assert f"row {named} " in str(ei.value) + " ", (label, str(ei.value))
        assert sv.preconditioner_source == 1
        got = sv.solve(b, None, 8)
        sv.close()
        ref = make()
        want = ref.solve(b, None, 8)
        ref.close()
        assert same_bits(got, want), label

    sv = pkg.Solver(ctx, n, len(no_diag[2]), no_diag[0], no_diag[1], no_diag[2], 1)
    with pytest.raises(pkg._lib.CgAmdError) as ei:
        sv.set_preconditioner("jacobi")
    assert ei.value.status == pkg._lib.ERR_INVALID and f"row {head}" in str(ei.value)
    assert sv.preconditioner_source == 0
    sv.close()
