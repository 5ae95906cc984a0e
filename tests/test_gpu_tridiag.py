"""Tridiagonal (line) preconditioner: the reference PCG's spsolve branch (helmFE_var.py:561-562) with a tridiagonal sparse M,
solved on the device by the line sweeps of precond.hip (cgamd_solver_set_preconditioner_tridiag, Solver.set_preconditioner)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import tridiag_pcg as tp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcg_tridiag_iterates.npz")


def parts(A, dtype):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(dtype)


def solver(pkg, ctx, A, dtype, nrhs=1, flags=0):
    ip, ix, da = parts(A, dtype)
    return pkg.Solver(ctx, A.shape[0], len(ix), da, ip, ix, nrhs, flags=flags)


def tols(dtype):
    return (1e-9, 1e-10) if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-4)


def check_run(x, h, A, M, B, iters, dtype, solve=None):
    """x / history of a device run against the restatement, per right-hand side"""
    xt, ht = tols(dtype)
    n = A.shape[0]
    for r in range(B.shape[0]):
        xo, _, ho = tp.pcg_sparse(A, B[r].astype(complex), M, tol=0.0, maxit=iters, history=True, solve=solve)
        keep = np.abs(ho) / np.abs(ho[0]) > (1e-8 if xt < 1e-6 else 1e-4)     # reduction-order noise only while not converged
        assert np.max(np.abs(h[keep, r] - ho[keep]) / np.abs(ho[keep])) < ht, (r, dtype)
        xr = x[r * n:(r + 1) * n]
        assert np.linalg.norm(xr - xo) / np.linalg.norm(xo) < xt, (r, dtype, np.linalg.norm(xr - xo) / np.linalg.norm(xo))


def test_tridiag_pcg_against_reference_golden(pkg, gpu):
    """Solver.pcg(b, M=Htrid) returns the reference's (x, i); s.solve after set_preconditioner(Htrid) gives its k-iterates"""
    ctx, _, _ = gpu
    g = np.load(GOLDEN)
    for name, dtype, tol_key, tol in (("helm16", np.complex128, "tol1e-6", 1e-6), ("aniso16", np.float64, "tol1e-10", 1e-10)):
        A, M, b = tp.csr(g, name), tp.csr(g, f"{name}_M"), g[f"{name}_b"]
        s = solver(pkg, ctx, A, dtype)
        x, i = s.pcg(b.astype(dtype), M=M, tol=tol, maxit=1000, check_every=5)
        assert i == int(g[f"{name}_{tol_key}_i"]), (name, i)
        want = g[f"{name}_{tol_key}_x"]
        assert np.linalg.norm(x - want) / np.linalg.norm(want) < 1e-8, name
        s.set_preconditioner(M)
        assert pkg._lib.load().cgamd_solver_loop_launches(s.handle) == 4
        for k, want in zip(g["ks"], g[f"{name}_X"]):
            x, h = s.solve(b.astype(dtype), None, int(k))
            assert np.linalg.norm(x - want) / np.linalg.norm(want) < 1e-9, (name, k)
            _, _, ho = tp.pcg_sparse(A, b, M, tol=0.0, maxit=int(k), history=True)
            assert np.max(np.abs(h[:, 0] - ho) / np.abs(ho)) < 1e-10, (name, k)
        s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_tridiag_pcg_dtypes_multi_rhs(pkg, gpu, dtype):
    """every value type, 3 right-hand sides sharing M, 61 x 61 shifted Poisson (61 segments, 3721 rows: padding rows in fp64 /
    complex64, chunks of several lines), against the restatement per right-hand side"""
    ctx, _, _ = gpu
    N = 61
    T = sp.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
    A = 3.0 * sp.kron(sp.identity(N), T) + sp.kron(T, sp.identity(N)) + sp.diags(np.linspace(0.5, 4.0, N * N))
    if np.dtype(dtype).kind == "c":
        A = A * (1.0 + 0.05j)
    A = sp.csr_matrix(A)
    M = tp.band(A)
    rng = np.random.default_rng(11)
    B = rng.standard_normal((3, N * N)) + (1j * rng.standard_normal((3, N * N)) if np.dtype(dtype).kind == "c" else 0)
    s = solver(pkg, ctx, A, dtype, nrhs=3)
    s.set_preconditioner(M)
    x, h = s.solve(B.reshape(-1).astype(dtype), None, 12)
    s.close()
    check_run(x, h, A, M, B, 12, dtype)


def test_tridiag_segments_longer_than_a_chunk(pkg, gpu):
    """the three-launch sweep: a 1-D system of 200 000 rows (one segment) and a matrix with random segment breaks (segments of
    1 to 3000 rows), fp64, against scipy"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    rng = np.random.default_rng(5)
    n = 200_000
    main = 2.0 + rng.uniform(0.01, 1.0, n)
    A1 = sp.diags([-np.ones(n - 1), main, -np.ones(n - 1)], [-1, 0, 1], format="csr")
    M1 = sp.diags([-0.9 * np.ones(n - 1), main, -0.9 * np.ones(n - 1)], [-1, 0, 1], format="csr")
    # random segments: tridiagonal blocks, coupled in A by a symmetric long-range term that M leaves out
    n2 = 150_000
    cuts = np.sort(rng.choice(np.arange(1, n2), size=200, replace=False))
    off = -rng.uniform(0.2, 1.0, n2 - 1)
    off[cuts - 1] = 0.0
    far = -0.3 * np.ones(n2 - 37)
    A2 = sp.diags([far, off, 3.0 + rng.uniform(0.0, 1.0, n2), off, far], [-37, -1, 0, 1, 37], format="csr")
    M2 = tp.band(A2)
    assert np.max(np.diff(np.concatenate([[0], cuts, [n2]]))) > 1024
    for A, M in ((A1, M1), (A2, M2)):
        B = rng.standard_normal((1, A.shape[0]))
        lu = spla.splu(sp.csc_matrix(M))
        s = solver(pkg, ctx, A, np.float64)
        s.set_preconditioner(M)
        assert lib.cgamd_solver_loop_launches(s.handle) == 6
        x, h = s.solve(B.reshape(-1), None, 10)
        s.close()
        check_run(x, h, A, M, B, 10, np.float64, solve=lambda r: lu.solve(r.real) + 1j * lu.solve(r.imag))


def aniso3d():
    return tp.laplace3d_aniso(40, 30, 20, cx=10.0)


def test_tridiag_invariants(pkg, gpu):
    """bits: 15 + 15 = 30 iterations, graphs = plain launches, run to run; launched loop only; removing M gives a fresh
    handle's bits; a diagonal M after the tridiagonal one gives a diagonal-only handle's bits"""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    A = aniso3d()
    M = tp.band(A)
    n = A.shape[0]
    b = np.linspace(1.0, 2.0, n)

    def run(flags=0, split=None, m=M):
        s = solver(pkg, ctx, A, np.float64, flags=flags)
        s.set_preconditioner(m)
        s.set_rhs(b)
        for k in split or (30,):
            s.iterate(k)
        out = (s.x(), s.history())
        s.close()
        return out

    x0, h0 = run()
    for other in (run(split=(15, 15)), run(flags=pkg._lib.NO_GRAPH), run()):
        assert np.array_equal(other[0], x0) and np.array_equal(other[1], h0)
    s = solver(pkg, ctx, A, np.float64)
    s.set_preconditioner(M)
    s.set_rhs(b)
    assert lib.cgamd_solver_loop_launches(s.handle) >= 2
    its = ctypes.c_int(0)
    assert lib.cgamd_solver_iterate_tol(s.handle, 10, 1e-6, ctypes.byref(its)) == pkg._lib.ERR_STATE
    # removal: the bits of a handle that never had a preconditioner
    s.set_preconditioner(None)
    s.set_rhs(b)
    s.iterate(30)
    xr, hr = s.x(), s.history()
    f = solver(pkg, ctx, A, np.float64)
    f.set_rhs(b)
    f.iterate(30)
    assert np.array_equal(xr, f.x()) and np.array_equal(hr, f.history())
    assert lib.cgamd_solver_loop_launches(s.handle) == lib.cgamd_solver_loop_launches(f.handle)
    f.close()
    # diagonal after tridiagonal
    m = 1.0 / A.diagonal()
    s.set_preconditioner(M)
    s.set_preconditioner(m)
    s.set_rhs(b)
    s.iterate(30)
    xd, hd = s.x(), s.history()
    s.close()
    xj, hj = run(m=m)
    assert np.array_equal(xd, xj) and np.array_equal(hd, hj)


def test_tridiag_errors(pkg, gpu):
    """an entry off the band is a ValueError; a zero pivot is CGAMD_ERR_INVALID naming the row, and the handle keeps working"""
    ctx, _, _ = gpu
    A = aniso3d()
    n = A.shape[0]
    b = np.linspace(1.0, 2.0, n)
    s = solver(pkg, ctx, A, np.float64)
    with pytest.raises(ValueError, match="diagonal or tridiagonal"):
        s.set_preconditioner(tp.band(A, width=41))          # the y-coupling at distance 40
    bad = tp.band(A).tolil()
    bad[7, 7] = 0.0                                         # with a zero off-diagonal beside it: u_7 = 0
    bad[7, 6] = 0.0
    with pytest.raises(pkg._lib.CgAmdError) as ei:
        s.set_preconditioner(sp.csr_matrix(bad))
    assert ei.value.status == pkg._lib.ERR_INVALID and "row 7" in str(ei.value)
    M = tp.band(A)
    s.set_preconditioner(M)
    x, h = s.solve(b, None, 8)
    s.close()
    check_run(x, h, A, M, b[None, :], 8, np.float64)


def test_tridiag_device_inputs_full_size(pkg, gpu):
    """the C entry with device inputs (torch tensors, on_device = 1), anisotropic 7-point system of 2M rows, 40 iterations
    against a scipy PCG that factors M once"""
    import torch
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    A = tp.laplace3d_aniso(200, 100, 100, cx=20.0)
    n = A.shape[0]
    assert n >= 2_000_000
    M = tp.band(A)
    dev = torch.device("cuda", 0)
    lower = torch.zeros(n, dtype=torch.float64, device=dev)
    upper = torch.zeros(n, dtype=torch.float64, device=dev)
    lower[1:] = torch.from_numpy(M.diagonal(-1)).to(dev)
    upper[:-1] = torch.from_numpy(M.diagonal(1)).to(dev)
    diag = torch.from_numpy(M.diagonal(0).copy()).to(dev)
    torch.cuda.synchronize()
    s = solver(pkg, ctx, A, np.float64)
    pkg._lib.check(lib.cgamd_solver_set_preconditioner_tridiag(s.handle, pkg._lib.ptr(lower), pkg._lib.ptr(diag),
                                                                pkg._lib.ptr(upper), 1))
    assert lib.cgamd_solver_loop_launches(s.handle) == 4
    b = np.sin(np.arange(n) * 0.001) + 1.0
    x, h = s.solve(b, None, 40)
    s.close()
    lu = spla.splu(sp.csc_matrix(M))
    check_run(x, h, A, M, b[None, :], 40, np.float64, solve=lambda r: lu.solve(r.real) + 1j * lu.solve(r.imag))
