"""Aggregation multigrid preconditioner on the device (cgamd_solver_set_preconditioner_multigrid, csrc/multigrid.hip and
csrc/multigrid_setup.cpp) against the host restatement mg_ref.py: the Galerkin matrices entry by entry, the V-cycle on its own, the
PCG loop, the tolerance stop, the bit-level promises and every error and refusal of the entry."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import mg_ref
import tridiag_pcg as tp

pytestmark = pytest.mark.gpu
ALL = [np.float32, np.float64, np.complex64, np.complex128]


def parts(A, dtype):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(dtype)


def solver(pkg, ctx, A, dtype, nrhs=1, flags=0, **kw):
    ip, ix, da = parts(A, dtype)
    return pkg.Solver(ctx, A.shape[0], len(ix), da, ip, ix, nrhs, flags=flags, **kw)


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


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def system(kind, dims, dtype):
    A = mg_ref.variable7(*dims) if kind == "var7" else mg_ref.stencil27(*dims) if kind == "stencil27" else mg_ref.laplace3d(*dims)
    if np.dtype(dtype).kind == "c":
        A = sp.csr_matrix(A * (1.0 + 0.05j))
    return A


def rhs(dims, dtype, nrhs, seed=11):
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    B = rng.standard_normal((nrhs, n))
    if np.dtype(dtype).kind == "c":
        B = B + 1j * rng.standard_normal((nrhs, n))
    return B.astype(dtype)


# ---- Galerkin matrices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("kind", ["var7", "stencil27"])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 7, 1), (13, 1, 1)])
def test_galerkin_matrices(pkg, gpu, dims, kind, dtype):
    """every level's pointers and columns are scipy's P^T A P of the level above (sorted, nothing eliminated), its values within 2 ulp
    of the value type of the double-precision product, relative to the sum of |terms| of the entry; dims and rows by the formula"""
    ctx = gpu[0]
    A = system(kind, dims, dtype)
    s = solver(pkg, ctx, A, dtype)
    s.set_preconditioner(("multigrid", dims, {"min_rows": 2}))
    levels = s.mg_levels()
    want_dims = [dims]
    while int(np.prod(want_dims[-1])) > 2:
        want_dims.append(mg_ref.coarse_dims(want_dims[-1]))
    assert [(L["nx"], L["ny"], L["nz"]) for L in levels] == want_dims
    assert [L["rows"] for L in levels] == [int(np.prod(d)) for d in want_dims]
    ip, ix, da = s.mg_level_matrix(0)
    p0 = parts(A, dtype)
    assert np.array_equal(ip, p0[0]) and np.array_equal(ix, p0[1]) and same(da, p0[2])
    eps = float(np.finfo(np.dtype(dtype)).eps)
    W = mg_ref.wide(dtype)
    for l in range(1, len(levels)):
        fine = sp.csr_matrix((da.astype(W), ix, ip), shape=(levels[l - 1]["rows"],) * 2)
        agg = mg_ref.agg_map(want_dims[l - 1])
        P = sp.csr_matrix((np.ones(agg.size), (np.arange(agg.size), agg)), shape=(agg.size, levels[l]["rows"]))
        pattern = sp.csr_matrix((np.ones(fine.nnz), ix, ip), shape=fine.shape)
        S = sp.csr_matrix(P.T @ pattern @ P)          # all terms positive: nothing cancels, the pattern of the product
        S.sort_indices()
        ip, ix, da = s.mg_level_matrix(l)
        assert levels[l]["nnz"] == S.nnz
        assert np.array_equal(ip, S.indptr) and np.array_equal(ix, S.indices), (l, dims, kind)
        prod = np.asarray((P.T @ fine @ P).todense())
        mag = np.asarray((P.T @ sp.csr_matrix((np.abs(fine.data), fine.indices, fine.indptr), shape=fine.shape) @ P).todense())
        rows = np.repeat(np.arange(levels[l]["rows"]), np.diff(ip))
        err = np.abs(da.astype(W) - prod[rows, ix]) / mag[rows, ix]
        print(f"  level {l} {want_dims[l]} {kind} {np.dtype(dtype).name}: nnz {S.nnz}, max error {err.max() / eps:.3f} ulp of sum |terms|")
        assert err.max() <= 2.0 * eps, (l, dims, kind, dtype)
        if kind == "var7":
            assert int(np.max(np.diff(ip))) <= 7
    s.close()


# ---- the V-cycle on its own -------------------------------------------------------------------------------------------------------------
def cycle_error(z, z_ref):
    z_ref = np.asarray(z_ref)
    return float(np.max(np.abs(np.asarray(z).astype(z_ref.dtype) - z_ref)) / np.max(np.abs(z_ref)))


def check_cycle(s, H, B, dtype, label):
    """error of the device z against the extended-precision cycle <= 4 max(error of the cycle in the value type, 4 eps): the bound
    never looks at the code under test.  Both figures are printed before the assertion"""
    n = B.shape[1]
    z = s.mg_apply(B.reshape(-1)).reshape(B.shape)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    figures = []
    for r in range(B.shape[0]):
        z_ref = H.vcycle(B[r], mg_ref.wide(dtype, True))
        e_dev, e_type = cycle_error(z[r], z_ref), cycle_error(H.vcycle(B[r], dtype), z_ref)
        print(f"  V-cycle {label} {np.dtype(dtype).name} n {n} rhs {r}: e(z) {e_dev:.3e}, e(z in type) {e_type:.3e}, "
              f"ratio {e_dev / e_type if e_type > 0 else float('inf'):.2f}, bound {4.0 * max(e_type, 4.0 * eps):.3e}")
        figures.append((e_dev, e_type))
    for r, (e_dev, e_type) in enumerate(figures):
        assert e_dev <= 4.0 * max(e_type, 4.0 * eps), (label, np.dtype(dtype).name, r, e_dev, e_type)


OPTS = {"min_rows": 32}


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("dims", [(13, 11, 9), (16, 16, 16)])
def test_vcycle_alone(pkg, gpu, dims, dtype, nrhs):
    """13 x 11 x 9 = 1287 rows (padding rows in fp64 / complex64, ragged aggregates) and 16^3, four levels each"""
    ctx = gpu[0]
    A = system("var7", dims, dtype)
    H = mg_ref.Hierarchy(A, dims, dtype, **OPTS)
    s = solver(pkg, ctx, A, dtype, nrhs)
    s.set_preconditioner(("multigrid", dims, OPTS))
    levels = s.mg_levels()
    assert len(levels) == len(H.levels) == 4
    for L, Lh in zip(levels, H.levels):
        assert abs(L["lmax"] - Lh.lmax) <= 1e-13 * Lh.lmax
    check_cycle(s, H, rhs(dims, dtype, nrhs), dtype, "x".join(map(str, dims)))
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_vcycle_more_smoothing_steps_and_one_level(pkg, gpu, dtype):
    """two and three smoothing steps (the later Chebyshev steps and their d vector) without over-correction, and a hierarchy of one
    level (the eight-step smoother alone)"""
    ctx = gpu[0]
    dims = (13, 11, 9)
    A = system("var7", dims, dtype)
    s = solver(pkg, ctx, A, dtype, 2)
    for opts in ({"min_rows": 32, "smooth_steps": 2, "over_correction": 1.0}, {"min_rows": 32, "smooth_steps": 3},
                 {"min_rows": 5000}):
        s.set_preconditioner(("multigrid", dims, opts))
        H = mg_ref.Hierarchy(A, dims, dtype, **opts)
        assert len(s.mg_levels()) == len(H.levels)
        check_cycle(s, H, rhs(dims, dtype, 2), dtype, str(opts))
    s.close()


# ---- fixed-count PCG --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("dims", [(13, 11, 9), (16, 16, 16)])
def test_fixed_count_pcg(pkg, gpu, dims, dtype):
    """8 iterations, 3 right-hand sides, against pcg_sparse with the restated cycle as its solve"""
    ctx = gpu[0]
    A = system("var7", dims, dtype)
    H = mg_ref.Hierarchy(A, dims, dtype, **OPTS)
    B = rhs(dims, dtype, 3)
    s = solver(pkg, ctx, A, dtype, 3)
    s.set_preconditioner(("multigrid", dims, OPTS))
    lib = pkg._lib.load()
    assert lib.cgamd_solver_preconditioner_source(s.handle) == 2
    assert lib.cgamd_solver_loop_launches(s.handle) == 5 + 1 + 5 * 3 + 14      # four levels, one smoothing step
    assert lib.cgamd_solver_iter_moved_bytes(s.handle) > 3 * lib.cgamd_solver_spmv_moved_bytes(s.handle)
    x, h = s.solve(B.reshape(-1), None, 8)
    s.close()
    check_run(x, h, A, sp.identity(A.shape[0]), B, 8, dtype, solve=H.solve())


# ---- convergence ------------------------------------------------------------------------------------------------------------------------
def test_convergence_32_cubed(pkg, gpu):
    """32^3 fp64 to 1e-8 ||b|| through solve_until: stops in the first iteration that meets the tolerance, x has the bits of set_rhs;
    iterate(its), and the count is at most a third of plain CG's on the same handle (the restatement alone: 19 against 119)"""
    ctx = gpu[0]
    N = 32
    A = mg_ref.laplace3d(N, N, N)
    b = np.random.default_rng(1).standard_normal(N ** 3)
    tol = 1e-8 * np.linalg.norm(b)
    s = solver(pkg, ctx, A, np.float64)
    s.set_preconditioner(("multigrid", (N, N, N)))
    assert [L["rows"] for L in s.mg_levels()] == [32768, 4096, 512]
    x, its, h = s.solve_until(b, tol=tol, maxit=400)
    its_mg = int(its[0])
    norms = np.sqrt(np.abs(h[:, 0]))
    assert its_mg == int(np.flatnonzero(~(norms[1:] >= tol))[0]) + 1
    assert np.linalg.norm(b - A @ x) <= 2.0 * tol
    s.set_rhs(b)
    s.iterate(its_mg)
    assert same(s.x(), x)
    s.set_preconditioner(None)
    _, its_cg, _ = s.solve_until(b, tol=tol, maxit=400)
    print(f"32^3 to 1e-8 ||b||: multigrid PCG {its_mg} iterations, plain CG {int(its_cg[0])}")
    assert its_mg <= int(its_cg[0]) / 3
    s.close()


def test_until_three_right_hand_sides(pkg, gpu):
    """a tolerance per right-hand side: each column stops on its own and keeps the bits of iterate(its_r)"""
    ctx = gpu[0]
    dims = (13, 11, 9)
    A = system("var7", dims, np.float64)
    B = rhs(dims, np.float64, 3)
    tol = np.array([1e-3, 1e-9, 1e-6]) * np.linalg.norm(B, axis=1)
    s = solver(pkg, ctx, A, np.float64, 3)
    s.set_preconditioner(("multigrid", dims, OPTS))
    x, its, h = s.solve_until(B.reshape(-1), tol=tol, maxit=200, check_every=4)
    assert its[0] < its[2] < its[1] < 200
    n = A.shape[0]
    for r in range(3):
        norms = np.sqrt(np.abs(h[:, r]))
        assert its[r] == int(np.flatnonzero(~(norms[1:] >= tol[r]))[0]) + 1
        s.set_rhs(B.reshape(-1))
        s.iterate(int(its[r]))
        assert same(s.x()[r * n:(r + 1) * n], x[r * n:(r + 1) * n]), r
    s.close()


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
def test_bits(pkg, gpu):
    """run to run; iterate(3) + iterate(5) = iterate(8); plain launches = graphs; removing the preconditioner restores the plain bits;
    another preconditioner replaces it and it replaces another"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (13, 11, 9)
    A = system("var7", dims, np.float64)
    b = rhs(dims, np.float64, 2).reshape(-1)
    M = ("multigrid", dims, OPTS)

    def run(flags=0, split=(16,), m=M, before=None):
        s = solver(pkg, ctx, A, np.float64, 2, flags=flags)
        if before is not None:
            s.set_preconditioner(before)
        s.set_preconditioner(m)
        s.set_rhs(b)
        for k in split:
            s.iterate(k)
        out = (s.x(), s.history(), len(s.mg_levels()), lib.cgamd_solver_preconditioner_source(s.handle))
        s.close()
        return out

    x0, h0, nl, src = run()
    assert nl == 4 and src == 2
    for other in (run(), run(split=(3, 5, 8)), run(flags=L.NO_GRAPH), run(before="jacobi"), run(before=("line", 1))):
        assert same(other[0], x0) and same(other[1], h0)
    plain = run(m=None)
    assert plain[2] == 0 and plain[3] == 0 and not same(plain[0], x0)
    back = run(m=None, before=M)
    assert same(back[0], plain[0]) and same(back[1], plain[1]) and back[2] == 0
    jac = run(m="jacobi")
    rep = run(m="jacobi", before=M)
    assert same(rep[0], jac[0]) and same(rep[1], jac[1]) and rep[2] == 0


# ---- refresh_values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.complex128])
def test_refresh_values_rebuilds_the_hierarchy(pkg, gpu, dtype):
    """a borrowed value array scaled by 2 in place: after refresh_values the coarse values are doubled and the cycle returns z / 2"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    A = system("var7", dims, dtype)
    ip, ix, da = parts(A, dtype)
    dv, dp, dc = (pkg.DeviceBuffer(ctx, hostbuf=a) for a in (da, ip, ix))
    s = pkg.Solver(ctx, A.shape[0], len(ix), dv, dp, dc, 1, flags=L.MATRIX_ON_DEVICE, dtype=dtype)
    s.set_preconditioner(("multigrid", dims, OPTS))
    r = rhs(dims, dtype, 1).reshape(-1)
    z1, m1 = s.mg_apply(r), [s.mg_level_matrix(l) for l in range(len(s.mg_levels()))]
    da2 = (2 * da).astype(dtype)
    L.check(lib.cgamd_memcpy_h2d(ctx.handle, L.ptr(dv), L.ptr(da2), da2.nbytes))
    s.refresh_values(None)
    assert lib.cgamd_solver_preconditioner_source(s.handle) == 2 and len(s.mg_levels()) == len(m1) >= 3
    for l, (p1, c1, v1) in enumerate(m1):
        p2, c2, v2 = s.mg_level_matrix(l)
        assert np.array_equal(p1, p2) and np.array_equal(c1, c2) and same(v2, (2 * v1).astype(dtype)), l
    z2 = s.mg_apply(r)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    assert np.max(np.abs(2 * z2 - z1)) <= 4 * eps * np.max(np.abs(z1))
    # a refresh that cannot rebuild (a zero diagonal) removes the preconditioner and names level and row
    bad = da2.copy()
    bad[ip[4]:ip[5]][ix[ip[4]:ip[5]] == 4] = 0
    L.check(lib.cgamd_memcpy_h2d(ctx.handle, L.ptr(dv), L.ptr(bad), bad.nbytes))
    with pytest.raises(pkg.CgAmdError, match=r"refresh_values: level 0: zero, missing or non-finite diagonal in row 4"):
        s.refresh_values(None)
    assert s.mg_levels() == [] and lib.cgamd_solver_preconditioner_source(s.handle) == 0
    s.close()


# ---- errors and refusals ----------------------------------------------------------------------------------------------------------------
def mg_status(lib, s, nx, ny, nz, steps=0, omega=0.0, min_rows=0):
    return lib.cgamd_solver_set_preconditioner_multigrid(s.handle, nx, ny, nz, steps, ctypes.c_double(omega), min_rows)


def test_invalid_arguments_leave_the_handle_as_it_was(pkg, gpu):
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    A = system("var7", dims, np.float64)
    b = rhs(dims, np.float64, 1).reshape(-1)
    s = solver(pkg, ctx, A, np.float64)
    s.set_preconditioner(("multigrid", dims, OPTS))
    want = s.solve(b, None, 6)
    for args in ((9, 7, 4), (9, 7, 6), (0, 7, 45), (9, -7, -5), (315, 1, 0), (9, 7, 5, 5), (9, 7, 5, -1), (9, 7, 5, 0, float("nan")),
                 (9, 7, 5, 0, -1.0), (9, 7, 5, 0, float("inf")), (9, 7, 5, 0, 0.0, -1)):
        assert mg_status(lib, s, *args) == L.ERR_INVALID, args
        assert b"set_preconditioner_multigrid" in lib.cgamd_last_error()
    info = (ctypes.c_longlong * 6)()
    assert lib.cgamd_solver_mg_level(s.handle, 7, info) == L.ERR_INVALID and lib.cgamd_solver_mg_level(s.handle, -1, info) == L.ERR_INVALID
    got = s.solve(b, None, 6)
    assert same(got[0], want[0]) and same(got[1], want[1]) and len(s.mg_levels()) == 3
    # with the preconditioner set: no device-side stop of the resident loops, no residual replacement
    s.set_rhs(b)
    run = ctypes.c_int(0)
    assert lib.cgamd_solver_iterate_tol(s.handle, 10, ctypes.c_double(1e-3), ctypes.byref(run)) == L.ERR_STATE
    rd = pkg.DeviceBuffer(ctx, hostbuf=b)
    assert lib.cgamd_solver_replace_residual(s.handle, L.ptr(rd)) == L.ERR_STATE
    assert b"multigrid" in lib.cgamd_last_error()
    rd.release()
    s.iterate(6)
    assert same(s.x(), want[0])
    s.set_preconditioner(None)
    assert s.mg_levels() == []
    assert lib.cgamd_solver_mg_level(s.handle, 0, info) == L.ERR_STATE
    assert lib.cgamd_solver_mg_apply(s.handle, L.ptr(b), L.ptr(b)) == L.ERR_STATE
    s.close()


def test_setup_errors_name_level_and_row(pkg, gpu):
    """a zero diagonal on level 0, one that appears only on level 1, and a coarse row of more than 64 distinct columns; a
    preconditioner set before stays in force"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    n = 16
    T = sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="lil")
    b = np.linspace(1.0, 2.0, n)
    zero0 = T.copy()
    zero0[5, 5] = 0.0
    zero1 = T.copy()
    zero1[6, 6] = zero1[7, 7] = 1.0            # aggregate 3 = rows 6, 7: 1 + 1 - 1 - 1 = 0 on level 1 only
    for M, text in ((zero0, b"level 0: zero, missing or non-finite diagonal in row 5"),
                    (zero1, b"level 1: zero, missing or non-finite diagonal in row 3")):
        A = sp.csr_matrix(M)
        ip, ix = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        s = pkg.Solver(ctx, n, len(ix), A.data.astype(np.float64), ip, ix, 1)
        s.set_preconditioner(np.full(n, 0.5))
        want = s.solve(b, None, 4)
        assert mg_status(lib, s, n, 1, 1, 0, 0.0, 2) == L.ERR_INVALID
        assert text in lib.cgamd_last_error(), lib.cgamd_last_error()
        assert lib.cgamd_solver_preconditioner_source(s.handle) == 1 and s.mg_levels() == []
        got = s.solve(b, None, 4)
        assert same(got[0], want[0]) and same(got[1], want[1])
        s.close()
    # row 0 reaches 70 aggregates
    n = 256
    W = sp.lil_matrix(sp.identity(n) * 4.0)
    W[0, np.arange(0, 140, 2)] = 1.0
    s = solver(pkg, ctx, W, np.float32)
    assert mg_status(lib, s, n, 1, 1, 0, 0.0, 2) == L.ERR_INVALID
    assert b"level 1: coarse row 0 has more than 64 distinct columns" in lib.cgamd_last_error(), lib.cgamd_last_error()
    assert s.mg_levels() == []
    s.close()


def test_handles_the_entry_does_not_serve(pkg, gpu):
    """batched, Hermitian (complex), row-major and unfused handles: CGAMD_ERR_STATE, and they solve as before"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (24, 24, 1)
    A = system("lap", dims, np.float64)
    n = A.shape[0]
    ip, ix, da = parts(A, np.float64)
    L.check(lib.cgamd_tune(b"spmm_rowmajor", 2))             # fp64 x 16 keeps its right-hand sides interleaved under this knob
    try:
        rm = pkg.Solver(ctx, n, len(ix), da, ip, ix, 16)
    finally:
        L.check(lib.cgamd_tune(b"spmm_rowmajor", 1))
    handles = [(rm, 16),
               (pkg.Solver(ctx, n, len(ix), da, ip, ix, 2, flags=L.UNFUSED), 2),
               (pkg.Solver(ctx, n, len(ix), np.tile(da, 2), ip, ix, 2, batched=True), 2),
               (pkg.Solver(ctx, n, len(ix), da.astype(np.complex128), ip, ix, 1, hermitian=True), 1)]
    try:
        for s, nrhs in handles:
            b = np.tile(np.linspace(1.0, 2.0, n), nrhs).astype(s.dtype)
            want = s.solve(b, None, 5)
            assert mg_status(lib, s, *dims) == L.ERR_STATE
            assert b"set_preconditioner_multigrid" in lib.cgamd_last_error()
            assert lib.cgamd_solver_mg_levels(s.handle) == 0 and lib.cgamd_solver_preconditioner_source(s.handle) == 0
            got = s.solve(b, None, 5)
            assert same(got[0], want[0]) and same(got[1], want[1])
    finally:
        for s, _ in handles:
            s.close()
    # the real value types run the same recurrence with the flag: served
    s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, hermitian=True)
    s.set_preconditioner(("multigrid", dims))
    assert len(s.mg_levels()) == 2
    s.close()


def test_pcg_entry(pkg, gpu):
    """Solver.pcg(b, M=("multigrid", dims), tol=...) through the existing path: the reference's (x, i), the preconditioner removed
    afterwards"""
    ctx = gpu[0]
    dims = (20, 20, 1)
    A = system("lap", dims, np.float64)
    b = rhs(dims, np.float64, 1).reshape(-1)
    H = mg_ref.Hierarchy(A, dims, np.float64, min_rows=32)
    tol = 1e-8 * np.linalg.norm(b)
    xo, io = tp.pcg_sparse(A, b.astype(complex), sp.identity(A.shape[0]), tol=tol, maxit=200, solve=H.solve())
    s = solver(pkg, ctx, A, np.float64)
    x, i = s.pcg(b, M=("multigrid", dims, {"min_rows": 32}), tol=tol, maxit=200)
    assert i == io and np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-9
    assert s.mg_levels() == []
    s.close()


def test_cli_multigrid(pkg, gpu, tmp_path):
    """oclcgex ... --double --multigrid NX NY NZ --history F on a 32 x 24 grid: the history of 12 iterations is the library's own
    (the same handle calls) and falls by far more than plain CG's in as many iterations"""
    dims = (32, 24, 1)
    A = system("lap", dims, np.float64)
    n = A.shape[0]
    low = sp.tril(A).tocoo()
    p, hp = str(tmp_path / "lap32x24.mtx"), str(tmp_path / "history.bin")
    pkg.mmio.mmwrite(p, n, low.row, low.col, low.data, "real", "symmetric")
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "oclcgex")
    r = subprocess.run([exe, p, "1", "0", "12", "--double", "--multigrid", "32", "24", "1", "--history", hp], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "multigrid: 2 levels, 25 launches per iteration" in r.stdout
    h = np.fromfile(hp, dtype=np.float64)
    s = solver(pkg, gpu[0], A, np.float64)
    b = np.full(n, 5.0)
    _, plain = s.solve(b, None, 12)
    s.set_preconditioner(("multigrid", dims))
    _, want = s.solve(b, None, 12)
    s.close()
    assert h.shape == (13,) and np.allclose(h, want[:, 0], rtol=1e-12, atol=0.0)
    assert h[12] < 1e-6 * plain[12, 0]
    bad = subprocess.run([exe, p, "1", "0", "12", "--double", "--multigrid", "32", "25", "1"], capture_output=True, text=True)
    assert bad.returncode == 2 and "nx * ny * nz must equal the size" in bad.stderr
