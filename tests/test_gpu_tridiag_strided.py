"""Line preconditioner along the y or z axis of a grid: a tridiagonal M whose coupled rows lie `stride` apart
(cgamd_solver_set_preconditioner_tridiag_strided, precond_strided.hip; Solver.set_preconditioner picks it for a sparse M with
stored non-zeros on |i - j| in {0, s}).  The oracle is the restated reference PCG (tridiag_pcg.pcg_sparse: spsolve, or splu
factored once); tolerances are those of test_gpu_tridiag.check_run."""
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


def lu_solve(M):
    lu = spla.splu(sp.csc_matrix(M))
    if np.iscomplexobj(M.data):
        return lambda r: lu.solve(r)
    return lambda r: lu.solve(r.real) + 1j * lu.solve(r.imag)


def tols(dtype):
    return (1e-9, 1e-10) if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-4)


def check_run(x, h, A, M, B, iters, dtype, solve=None):
    """x / history of a device run against the restatement, per right-hand side; every figure is printed before it is asserted"""
    xt, ht = tols(dtype)
    n = A.shape[0]
    for r in range(B.shape[0]):
        xo, _, ho = tp.pcg_sparse(A, B[r].astype(complex), M, tol=0.0, maxit=iters, history=True, solve=solve)
        keep = np.abs(ho) / np.abs(ho[0]) > (1e-8 if xt < 1e-6 else 1e-4)     # reduction-order noise only while not converged
        herr = np.max(np.abs(h[keep, r] - ho[keep]) / np.abs(ho[keep]))
        xr = x[r * n:(r + 1) * n]
        xerr = np.linalg.norm(xr - xo) / np.linalg.norm(xo)
        print(f"  n={n} {np.dtype(dtype).name} rhs {r}: {int(keep.sum())} history entries compared, history err {herr:.3e} "
              f"(< {ht:g}), x err {xerr:.3e} (< {xt:g})")
        assert herr < ht, (r, dtype, herr)
        assert xerr < xt, (r, dtype, xerr)


GRIDS = [(24, 21, 17), (23, 21, 17)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("axis", ["y", "z"])
def test_strided_parity_y_and_z_lines(pkg, gpu, dtype, grid, axis):
    """y-lines (stride nx) and z-lines (stride nx ny), every value type, 3 right-hand sides sharing M, 12 iterations; 23 x 21 x 17
    has an odd row count (padding rows in fp64 / complex64 / fp32); coupling x10 along the preconditioned axis"""
    ctx, _, _ = gpu
    nx, ny, nz = grid
    n = nx * ny * nz
    s = nx if axis == "y" else nx * ny
    A = laplace3d(nx, ny, nz, cy=10.0 if axis == "y" else 1.0, cz=10.0 if axis == "z" else 1.0)
    cplx = np.dtype(dtype).kind == "c"
    if cplx:
        A = sp.csr_matrix(A * (1.0 + 0.05j))
    M = lines(A, s)
    rng = np.random.default_rng(11)
    B = rng.standard_normal((3, n))
    if cplx:
        # complex right-hand sides g (1 + 0.3j h), g and h normal: every entry has its own phase, but b.b = sum g^2 (1 - 0.09 h^2
        # + 0.6j h) keeps |b.b| near 0.8 b^H b.  The history is the UNCONJUGATED r.r; with independent normal real and imaginary
        # parts sum r_i^2 cancels to about r^H r / sqrt(n) (1/93 here), and a relative error on it measures that cancellation
        # and no solver: complex64 arithmetic restated on the CPU (factors rounded to the value type, Thomas per line, products
        # in the value type summed in double) is then 1e-4 to 1e-3 away from the oracle on these grids after 12 iterations,
        # against 1e-6 to 4e-6 with the right-hand sides used here.
        B = B * (1.0 + 0.3j * rng.standard_normal((3, n)))
    sv = solver(pkg, ctx, A, dtype, nrhs=3)
    sv.set_preconditioner(M)
    assert pkg._lib.load().cgamd_solver_loop_launches(sv.handle) == 4
    x, h = sv.solve(B.reshape(-1).astype(dtype), None, 12)
    sv.close()
    check_run(x, h, A, M, B, 12, dtype, solve=lu_solve(M))


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_strided_pcg_returns_the_reference_x_and_i(pkg, gpu, dtype):
    """Solver.pcg(b, M=z-lines) returns the oracle's (x, i) on the z-anisotropic 24 x 21 x 17 system, and needs fewer than half
    the iterations of Jacobi (the oracle alone: 47 against 119)"""
    ctx, _, _ = gpu
    nx, ny, nz = 24, 21, 17
    n = nx * ny * nz
    A = laplace3d(nx, ny, nz, cz=10.0)
    if np.dtype(dtype).kind == "c":
        A = sp.csr_matrix(A * (1.0 + 0.05j))
    M = lines(A, nx * ny)
    b = np.linspace(1.0, 2.0, n)
    xo, io = tp.pcg_sparse(A, b.astype(complex), M, tol=1e-8, maxit=1000, solve=lu_solve(M))
    sv = solver(pkg, ctx, A, dtype)
    x, i_line = sv.pcg(b.astype(dtype), M=M, tol=1e-8, maxit=1000, check_every=5)
    xerr = np.linalg.norm(x - xo) / np.linalg.norm(xo)
    _, i_jacobi = sv.pcg(b.astype(dtype), M=(1.0 / A.diagonal()).astype(dtype), tol=1e-8, maxit=1000, check_every=5)
    sv.close()
    print(f"  {np.dtype(dtype).name}: i = {i_line} (oracle {io}), x err {xerr:.3e}, Jacobi i = {i_jacobi}")
    assert i_line == io, (i_line, io)
    assert xerr < 1e-8, xerr
    assert 2 * i_line < i_jacobi, (i_line, i_jacobi)


def cut_system(rng, n, s, ncuts):
    """diagonal 5.5 + U(0, 1), couplings -U(0.2, 1) at distance s (ncuts of them zeroed) and -0.8 at distances 1 and 5"""
    off = -rng.uniform(0.2, 1.0, n - s)
    if ncuts:
        off[rng.choice(n - s, size=ncuts, replace=False)] = 0.0
    near, five = -0.8 * np.ones(n - 1), -0.8 * np.ones(n - 5)
    A = sp.diags([off, five, near, 5.5 + rng.uniform(0.0, 1.0, n), near, five, off], [-s, -5, -1, 0, 1, 5, s], format="csr")
    A.eliminate_zeros()
    return A


def test_strided_irregular_cuts_and_a_long_segment(pkg, gpu):
    """fp64: 120 000 rows at stride 37 with 300 random cuts (segments of one row to thousands, lanes of a wave with different
    lengths and scattered first rows), and 60 000 rows at stride 2 (two segments of 30 000 rows: the serial case); A has terms
    M leaves out; 8 iterations against splu"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    rng = np.random.default_rng(5)
    for n, s, ncuts in ((120_000, 37, 300), (60_000, 2, 0)):
        A = cut_system(rng, n, s, ncuts)
        M = lines(A, s)
        B = rng.standard_normal((1, n))
        sv = solver(pkg, ctx, A, np.float64)
        sv.set_preconditioner(M)
        assert lib.cgamd_solver_loop_launches(sv.handle) == 4
        x, h = sv.solve(B.reshape(-1), None, 8)
        sv.close()
        check_run(x, h, A, M, B, 8, np.float64, solve=lu_solve(M))


def test_strided_invariants(pkg, gpu):
    """bits: 15 + 15 = 30 iterations, graphs = plain launches, run to run; stride 1 through the new entry = the stride-1 entry;
    removing M gives a fresh handle's bits; a diagonal M after it gives a diagonal-only handle's bits; strided after stride-1
    gives a strided-only handle's bits; launched loop only"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    nx, ny, nz = 40, 30, 20
    A = laplace3d(nx, ny, nz, cz=10.0)
    n = A.shape[0]
    s = nx * ny
    M, M1 = lines(A, s), tp.band(A)
    b = np.linspace(1.0, 2.0, n)

    def run(flags=0, split=None, m=M, before=None):
        sv = solver(pkg, ctx, A, np.float64, flags=flags)
        if before is not None:
            sv.set_preconditioner(before)
        sv.set_preconditioner(m)
        sv.set_rhs(b)
        for k in split or (30,):
            sv.iterate(k)
        out = (sv.x(), sv.history())
        sv.close()
        return out

    x0, h0 = run()
    for other in (run(split=(15, 15)), run(flags=pkg._lib.NO_GRAPH), run(), run(before=M1)):
        assert np.array_equal(other[0], x0) and np.array_equal(other[1], h0)
    assert not np.array_equal(run(m=M1)[1], h0)             # the two forms are different preconditioners of this system

    # stride 1 through the new entry: the stride-1 entry itself
    lo, di, up = three(M1, 1, np.float64, n)
    outs = []
    for strided in (True, False):
        sv = solver(pkg, ctx, A, np.float64)
        if strided:
            st = lib.cgamd_solver_set_preconditioner_tridiag_strided(sv.handle, 1, pkg._lib.ptr(lo), pkg._lib.ptr(di), pkg._lib.ptr(up), 0)
        else:
            st = lib.cgamd_solver_set_preconditioner_tridiag(sv.handle, pkg._lib.ptr(lo), pkg._lib.ptr(di), pkg._lib.ptr(up), 0)
        pkg._lib.check(st)
        sv.set_rhs(b)
        sv.iterate(30)
        outs.append((sv.x(), sv.history()))
        sv.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])

    sv = solver(pkg, ctx, A, np.float64)
    sv.set_preconditioner(M)
    sv.set_rhs(b)
    assert lib.cgamd_solver_loop_launches(sv.handle) == 4
    its = ctypes.c_int(0)
    assert lib.cgamd_solver_iterate_tol(sv.handle, 10, 1e-6, ctypes.byref(its)) == pkg._lib.ERR_STATE
    # removal: the bits of a handle that never had a preconditioner
    sv.set_preconditioner(None)
    sv.set_rhs(b)
    sv.iterate(30)
    xr, hr = sv.x(), sv.history()
    f = solver(pkg, ctx, A, np.float64)
    f.set_rhs(b)
    f.iterate(30)
    assert np.array_equal(xr, f.x()) and np.array_equal(hr, f.history())
    assert lib.cgamd_solver_loop_launches(sv.handle) == lib.cgamd_solver_loop_launches(f.handle)
    f.close()
    # diagonal after strided
    m = 1.0 / A.diagonal()
    sv.set_preconditioner(M)
    sv.set_preconditioner(m)
    sv.set_rhs(b)
    sv.iterate(30)
    xd, hd = sv.x(), sv.history()
    sv.close()
    xj, hj = run(m=m)
    assert np.array_equal(xd, xj) and np.array_equal(hd, hj)


def test_strided_errors(pkg, gpu):
    """stride 0 and stride = size are CGAMD_ERR_INVALID; a zero pivot is CGAMD_ERR_INVALID naming the row, and the handle keeps
    working; an M with offsets {0, 1, s} is a ValueError"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    nx, ny, nz = 40, 30, 20
    A = laplace3d(nx, ny, nz, cz=10.0)
    n = A.shape[0]
    s = nx * ny
    M = lines(A, s)
    b = np.linspace(1.0, 2.0, n)
    sv = solver(pkg, ctx, A, np.float64)
    lo, di, up = three(M, s, np.float64, n)
    for bad_stride in (0, -3, n, n + 1):
        st = lib.cgamd_solver_set_preconditioner_tridiag_strided(sv.handle, bad_stride, pkg._lib.ptr(lo), pkg._lib.ptr(di), pkg._lib.ptr(up), 0)
        assert st == pkg._lib.ERR_INVALID, bad_stride
    with pytest.raises(ValueError, match="diagonal or tridiagonal"):
        sv.set_preconditioner(sp.csr_matrix(M + tp.band(A)))          # offsets {0, 1, s}
    row = 7 + 3 * s
    bad = M.tolil()
    bad[row, row] = 0.0                                               # with a zero coupling beside it: u_row = 0
    bad[row, row - s] = 0.0
    with pytest.raises(pkg._lib.CgAmdError) as ei:
        sv.set_preconditioner(sp.csr_matrix(bad))
    assert ei.value.status == pkg._lib.ERR_INVALID and f"row {row}" in str(ei.value)
    sv.set_preconditioner(M)
    x, h = sv.solve(b, None, 8)
    sv.close()
    check_run(x, h, A, M, b[None, :], 8, np.float64, solve=lu_solve(M))


def test_strided_device_inputs_full_size(pkg, gpu):
    """the C entry with device inputs (torch tensors, on_device = 1): 200 x 100 x 100 (2M rows), z-coupling x20, stride 20 000,
    40 iterations against a scipy PCG that factors M once"""
    import torch
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    nx, ny, nz = 200, 100, 100
    A = laplace3d(nx, ny, nz, cz=20.0)
    n = A.shape[0]
    s = nx * ny
    assert n >= 2_000_000 and s == 20_000
    M = lines(A, s)
    dev = torch.device("cuda", 0)
    lo, di, up = three(M, s, np.float64, n)
    lower, diag, upper = (torch.from_numpy(v).to(dev) for v in (lo, di, up))
    torch.cuda.synchronize()
    sv = solver(pkg, ctx, A, np.float64)
    pkg._lib.check(lib.cgamd_solver_set_preconditioner_tridiag_strided(sv.handle, s, pkg._lib.ptr(lower), pkg._lib.ptr(diag),
                                                                       pkg._lib.ptr(upper), 1))
    assert lib.cgamd_solver_loop_launches(sv.handle) == 4
    b = np.sin(np.arange(n) * 0.001) + 1.0
    x, h = sv.solve(b, None, 40)
    sv.close()
    check_run(x, h, A, M, b[None, :], 40, np.float64, solve=lu_solve(M))
