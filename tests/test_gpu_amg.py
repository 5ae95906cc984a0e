"""Algebraic aggregation multigrid on the device (cgamd_solver_set_preconditioner_amg, csrc/amg.hip and csrc/multigrid_setup.cpp)
against the host restatement amg_ref.py: the maps array for array, the Galerkin matrices through the device's own maps, the V-cycle on
its own, the PCG loop, convergence on systems the box aggregates cannot serve, the rules that stop coarsening, the bit-level promises
and every error and refusal of the entry."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref
import mg_ref
from test_gpu_multigrid import check_cycle, check_run, parts, rhs, same, solver

pytestmark = pytest.mark.gpu
ALL = [np.float32, np.float64, np.complex64, np.complex128]


def as_type(A, dtype):
    return sp.csr_matrix(A * (1.0 + 0.05j)) if np.dtype(dtype).kind == "c" else sp.csr_matrix(A)


def device_maps(s):
    levels = s.mg_levels()
    return levels, [s.mg_aggregates(l) for l in range(len(levels) - 1)]


def assert_same_hierarchy(s, H):
    """rows and maps of every level equal the restatement's, array for array"""
    levels, maps = device_maps(s)
    assert [L["rows"] for L in levels] == [L.n for L in H.levels]
    assert all((L["nx"], L["ny"], L["nz"]) == (L["rows"], 0, 0) for L in levels)
    for l, (agg, nc) in enumerate(maps):
        assert nc == H.levels[l + 1].n and np.array_equal(agg, H.levels[l].agg), l
    return levels


# ---- 1: the maps, exact ---------------------------------------------------------------------------------------------------------------
INTEGER_SYSTEMS = {"lap": lambda: mg_ref.laplace3d(7, 6, 5), "stencil27": lambda: mg_ref.stencil27(7, 6, 5), "z100": lambda: amg_ref.zaniso(9, 7, 6)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("passes", [1, 2, 3])
@pytest.mark.parametrize("kind", list(INTEGER_SYSTEMS))
def test_maps_exact(pkg, gpu, kind, passes, dtype):
    """integer-valued matrices: every real-part sum of every pass is exact, so every comparison of the matching is the restatement's
    and the maps are equal array for array, on every level down to two rows"""
    A = as_type(INTEGER_SYSTEMS[kind](), dtype)
    opts = {"passes": passes, "min_rows": 2}
    H = amg_ref.Hierarchy(A, dtype, **opts)
    assert len(H.levels) >= 3 and max(H.rounds) <= amg_ref.MAX_ROUNDS
    s = solver(pkg, gpu[0], A, dtype)
    s.set_preconditioner(("amg", opts))
    levels = assert_same_hierarchy(s, H)
    for l in range(1, len(levels)):
        ip, ix, da = s.mg_level_matrix(l)
        Ah = H.levels[l].A
        assert np.array_equal(ip, Ah.indptr) and np.array_equal(ix, Ah.indices) and same(da, Ah.data), l
    with pytest.raises(pkg.CgAmdError):
        s.mg_aggregates(len(levels) - 1)
    s.close()


# ---- 2: maps and Galerkin matrices on random values -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 7, 1), (13, 1, 1)])
def test_maps_and_galerkin_random_values(pkg, gpu, dims, dtype):
    """the DEVICE's maps are partitions into connected aggregates of at most 8 rows numbered by their smallest members; every level's
    pattern is scipy's P^T pattern P with the device's map, its values within 2 eps of the double product relative to the sum of
    |terms| (three roundings, one per pass: at most 1.5 eps)"""
    A = as_type(mg_ref.variable7(*dims), dtype)
    s = solver(pkg, gpu[0], A, dtype)
    s.set_preconditioner(("amg", {"passes": 3, "min_rows": 2}))
    levels, maps = device_maps(s)
    assert len(levels) >= 2
    eps = float(np.finfo(np.dtype(dtype)).eps)
    W = mg_ref.wide(dtype)
    ip, ix, da = s.mg_level_matrix(0)
    p0 = parts(A, dtype)
    assert np.array_equal(ip, p0[0]) and np.array_equal(ix, p0[1]) and same(da, p0[2])
    for l in range(1, len(levels)):
        agg, nc = maps[l - 1]
        nf = levels[l - 1]["rows"]
        fine = sp.csr_matrix((da.astype(W), ix, ip), shape=(nf, nf))
        assert nc == levels[l]["rows"]
        amg_ref.check_map(fine, agg, nc, 3)
        P = sp.csr_matrix((np.ones(nf), (np.arange(nf), agg)), shape=(nf, nc))
        pattern = sp.csr_matrix((np.ones(fine.nnz), ix, ip), shape=fine.shape)
        S = sp.csr_matrix(P.T @ pattern @ P)
        S.sort_indices()
        ip, ix, da = s.mg_level_matrix(l)
        assert levels[l]["nnz"] == S.nnz
        assert np.array_equal(ip, S.indptr) and np.array_equal(ix, S.indices), (l, dims)
        prod = np.asarray((P.T @ fine @ P).todense())
        mag = np.asarray((P.T @ sp.csr_matrix((np.abs(fine.data), fine.indices, fine.indptr), shape=fine.shape) @ P).todense())
        rows = np.repeat(np.arange(nc), np.diff(ip))
        err = np.abs(da.astype(W) - prod[rows, ix]) / mag[rows, ix]
        print(f"  level {l} rows {nc} {np.dtype(dtype).name}: nnz {S.nnz}, max error {err.max() / eps:.3f} eps of sum |terms|")
        assert err.max() <= 2.0 * eps, (l, dims, dtype)
    s.close()


# ---- 3: the V-cycle on its own --------------------------------------------------------------------------------------------------------
DIMS = (13, 11, 9)
OPTS = {"min_rows": 32}


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dtype", ALL)
def test_vcycle_alone(pkg, gpu, dtype, nrhs):
    """13 x 11 x 9 = 1287 rows (padding rows in fp64 / complex64), aggregates of every size: the existing bound of check_cycle"""
    A = as_type(mg_ref.variable7(*DIMS), dtype)
    H = amg_ref.Hierarchy(A, dtype, **OPTS)
    s = solver(pkg, gpu[0], A, dtype, nrhs)
    s.set_preconditioner(("amg", OPTS))
    levels = assert_same_hierarchy(s, H)
    assert len(levels) >= 3
    for L, Lh in zip(levels, H.levels):
        assert abs(L["lmax"] - Lh.lmax) <= 1e-13 * Lh.lmax
    check_cycle(s, H, rhs(DIMS, dtype, nrhs), dtype, "amg " + "x".join(map(str, DIMS)))
    s.close()


# ---- 4: fixed-count PCG ---------------------------------------------------------------------------------------------------------------
PCG_DIMS = (16, 16, 16)


@pytest.mark.parametrize("dtype", ALL)
def test_fixed_count_pcg(pkg, gpu, dtype):
    """8 iterations, 3 right-hand sides, against pcg_sparse with the restated cycle as its solve, at the existing tolerances; the
    launch count by the formula.  The system is 16^3 because of what complex64 itself can hold: the algebraic cycle converges faster
    than the box cycle, the unconjugated r.r of the last iterations kept lies 1e-3 ... 1e-4 below the first, and a PCG loop written
    in numpy with EVERY operation in complex64 (no device code involved) already stands 1.9e-4 from the double-precision history on
    13 x 11 x 9 with these right-hand sides -- above the 1e-4 asked -- and 1.9e-5 on 16^3 (fp32: 5e-7 and 3e-7)."""
    A = as_type(mg_ref.variable7(*PCG_DIMS), dtype)
    H = amg_ref.Hierarchy(A, dtype, **OPTS)
    B = rhs(PCG_DIMS, dtype, 3)
    s = solver(pkg, gpu[0], A, dtype, 3)
    s.set_preconditioner(("amg", OPTS))
    lib = pkg._lib.load()
    nl = len(assert_same_hierarchy(s, H))
    assert nl >= 3
    assert lib.cgamd_solver_preconditioner_source(s.handle) == 2
    assert lib.cgamd_solver_loop_launches(s.handle) == 5 + 1 + 5 * (nl - 1) + 14
    assert lib.cgamd_solver_iter_moved_bytes(s.handle) > 3 * lib.cgamd_solver_spmv_moved_bytes(s.handle)
    x, h = s.solve(B.reshape(-1), None, 8)
    s.close()
    check_run(x, h, A, sp.identity(A.shape[0]), B, 8, dtype, solve=H.solve())


# ---- 5: convergence -------------------------------------------------------------------------------------------------------------------
def converge(pkg, gpu, A, label):
    n = A.shape[0]
    b = np.random.default_rng(11).standard_normal(n)
    tol = 1e-6 * np.linalg.norm(b)
    H = amg_ref.Hierarchy(A, np.float64)
    its_ref = amg_ref.pcg_count(A, b, lambda r: H.vcycle(r), tol)
    s = solver(pkg, gpu[0], A, np.float64)
    s.set_preconditioner("amg")
    assert_same_hierarchy(s, H)
    x, its, h = s.solve_until(b, tol=tol, maxit=400)
    its_dev = int(its[0])
    norms = np.sqrt(np.abs(h[:, 0]))
    assert its_dev == int(np.flatnonzero(~(norms[1:] >= tol))[0]) + 1
    s.set_rhs(b)
    s.iterate(its_dev)
    assert same(s.x(), x)
    assert np.linalg.norm(b - A @ x) <= 2.0 * tol
    s.set_preconditioner("jacobi")
    _, its_j, _ = s.solve_until(b, tol=tol, maxit=400)
    s.close()
    print(f"  {label} to 1e-6 ||b||: device {its_dev}, restatement {its_ref}, Jacobi {int(its_j[0])}")
    assert abs(its_dev - its_ref) <= 2, (its_dev, its_ref)
    return its_dev, int(its_j[0])


def test_convergence_anisotropic(pkg, gpu):
    """24 x 20 x 16 with 100 x z-coupling (the restatement alone: 22 against the grid multigrid's 40 and Jacobi's 70)"""
    its_dev, its_j = converge(pkg, gpu, amg_ref.zaniso(24, 20, 16), "24x20x16 z-100")
    assert its_j >= 2 * its_dev


def test_convergence_permuted(pkg, gpu):
    """a randomly permuted 16^3 Laplacian: no grid to give"""
    converge(pkg, gpu, amg_ref.permuted(mg_ref.laplace3d(16, 16, 16)), "16^3 permuted")


# ---- 6: the rules that stop coarsening ------------------------------------------------------------------------------------------------
STOP_CASES = {"graph passes 1": (amg_ref.graph_laplacian, 1), "graph passes 3": (amg_ref.graph_laplacian, 3), "arrowhead": (amg_ref.arrowhead, 3),
              "diagonal": (amg_ref.diagonal, 3), "positive tridiagonal": (amg_ref.positive_tridiagonal, 3)}


@pytest.mark.parametrize("case", list(STOP_CASES))
def test_stop_rules(pkg, gpu, case):
    """rows of more than 64 columns drop a pass, no pass kept or coarsening below 0.8 ends the hierarchy: never an error"""
    make, passes = STOP_CASES[case]
    A = make()
    opts = {"passes": passes, "min_rows": 2}
    H = amg_ref.Hierarchy(A, np.float64, **opts)
    s = solver(pkg, gpu[0], A, np.float64)
    s.set_preconditioner(("amg", opts))
    levels = assert_same_hierarchy(s, H)
    print(f"  {case}: rows {[L['rows'] for L in levels]}")
    if not case.startswith("graph"):
        assert len(levels) == 1
    B = np.linspace(1.0, 2.0, A.shape[0])[None, :]
    x, h = s.solve(B.reshape(-1), None, 4)
    s.close()
    check_run(x, h, A, sp.identity(A.shape[0]), B, 4, np.float64, solve=H.solve())


# ---- 7: bits --------------------------------------------------------------------------------------------------------------------------
def test_bits(pkg, gpu):
    """run to run; iterate(3) + iterate(5) = iterate(8); plain launches = graphs; amg -> grid multigrid -> amg; removing it restores
    the plain bits"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    A = mg_ref.variable7(*DIMS)
    b = rhs(DIMS, np.float64, 2).reshape(-1)
    M = ("amg", OPTS)

    def run(flags=0, split=(8,), m=M, before=()):
        s = solver(pkg, ctx, A, np.float64, 2, flags=flags)
        for other in before:
            s.set_preconditioner(other)
        s.set_preconditioner(m)
        s.set_rhs(b)
        for k in split:
            s.iterate(k)
        out = (s.x(), s.history(), len(s.mg_levels()), lib.cgamd_solver_preconditioner_source(s.handle))
        s.close()
        return out

    x0, h0, nl, src = run()
    assert nl >= 3 and src == 2
    for other in (run(), run(split=(3, 5)), run(flags=L.NO_GRAPH), run(before=("jacobi",)), run(before=(M, ("multigrid", DIMS, OPTS)))):
        assert same(other[0], x0) and same(other[1], h0)
    grid = run(m=("multigrid", DIMS, OPTS))
    assert not same(grid[0], x0)
    swapped = run(m=("multigrid", DIMS, OPTS), before=(M,))
    assert same(swapped[0], grid[0]) and same(swapped[1], grid[1])
    plain = run(m=None)
    back = run(m=None, before=(M,))
    assert same(back[0], plain[0]) and same(back[1], plain[1]) and back[2] == 0 and back[3] == 0 and not same(plain[0], x0)


@pytest.mark.parametrize("dtype", [np.float32, np.complex128])
def test_refresh_values_rebuilds_maps_and_matrices(pkg, gpu, dtype):
    """new values in a borrowed array: after refresh_values the hierarchy -- maps included -- and a solve are those of a fresh handle"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    A1, A2 = as_type(mg_ref.variable7(*dims, seed=3), dtype), as_type(mg_ref.variable7(*dims, seed=4), dtype)
    ip, ix, da1 = parts(A1, dtype)
    da2 = parts(A2, dtype)[2]
    b = rhs(dims, dtype, 1).reshape(-1)
    dv, dp, dc = (pkg.DeviceBuffer(ctx, hostbuf=a) for a in (da1, ip, ix))
    s = pkg.Solver(ctx, A1.shape[0], len(ix), dv, dp, dc, 1, flags=L.MATRIX_ON_DEVICE, dtype=dtype)
    s.set_preconditioner(("amg", OPTS))
    L.check(lib.cgamd_memcpy_h2d(ctx.handle, L.ptr(dv), L.ptr(da2), da2.nbytes))
    s.refresh_values(None)
    assert lib.cgamd_solver_preconditioner_source(s.handle) == 2
    levels, maps = device_maps(s)
    mats = [s.mg_level_matrix(l) for l in range(len(levels))]
    got = s.solve(b, None, 6)
    s.close()
    f = solver(pkg, ctx, A2, dtype)
    f.set_preconditioner(("amg", OPTS))
    levels_f, maps_f = device_maps(f)
    assert len(levels) == len(levels_f) >= 3
    assert all(a[1] == c[1] and np.array_equal(a[0], c[0]) for a, c in zip(maps, maps_f))
    for l, m in enumerate(mats):
        assert all(same(u, v) for u, v in zip(m, f.mg_level_matrix(l))), l
    want = f.solve(b, None, 6)
    f.close()
    assert same(got[0], want[0]) and same(got[1], want[1])


# ---- 8: the tolerance stop with three right-hand sides --------------------------------------------------------------------------------
def test_until_three_right_hand_sides(pkg, gpu):
    """a tolerance per right-hand side: each column stops on its own and keeps the bits of iterate(its_r)"""
    A = mg_ref.variable7(*DIMS)
    B = rhs(DIMS, np.float64, 3)
    tol = np.array([1e-3, 1e-9, 1e-6]) * np.linalg.norm(B, axis=1)
    s = solver(pkg, gpu[0], A, np.float64, 3)
    s.set_preconditioner(("amg", OPTS))
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


# ---- 9: errors and refusals -----------------------------------------------------------------------------------------------------------
def amg_status(lib, s, passes=0, strength=0.0, steps=0, omega=0.0, min_rows=0):
    return lib.cgamd_solver_set_preconditioner_amg(s.handle, passes, ctypes.c_double(strength), steps, ctypes.c_double(omega), min_rows)


def test_invalid_arguments_leave_the_handle_as_it_was(pkg, gpu):
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    A = mg_ref.variable7(*dims)
    b = rhs(dims, np.float64, 1).reshape(-1)
    s = solver(pkg, ctx, A, np.float64)
    s.set_preconditioner(("amg", OPTS))
    nl = len(s.mg_levels())
    want = s.solve(b, None, 6)
    for args in ((4,), (-1,), (0, -0.25), (0, 1.5), (0, float("nan")), (0, float("inf")), (0, 0.0, 5), (0, 0.0, -1), (0, 0.0, 0, float("nan")),
                 (0, 0.0, 0, -1.0), (0, 0.0, 0, float("inf")), (0, 0.0, 0, 0.0, -1)):
        assert amg_status(lib, s, *args) == L.ERR_INVALID, args
        assert b"set_preconditioner_amg" in lib.cgamd_last_error()
    nc = ctypes.c_int(0)
    assert lib.cgamd_solver_mg_aggregates(s.handle, nl - 1, None, ctypes.byref(nc)) == L.ERR_INVALID
    assert lib.cgamd_solver_mg_aggregates(s.handle, -1, None, ctypes.byref(nc)) == L.ERR_INVALID
    got = s.solve(b, None, 6)
    assert same(got[0], want[0]) and same(got[1], want[1]) and len(s.mg_levels()) == nl
    # with the preconditioner set: no device-side stop of the resident loops, no residual replacement
    s.set_rhs(b)
    run = ctypes.c_int(0)
    assert lib.cgamd_solver_iterate_tol(s.handle, 10, ctypes.c_double(1e-3), ctypes.byref(run)) == L.ERR_STATE
    rd = pkg.DeviceBuffer(ctx, hostbuf=b)
    assert lib.cgamd_solver_replace_residual(s.handle, L.ptr(rd)) == L.ERR_STATE
    rd.release()
    s.iterate(6)
    assert same(s.x(), want[0])
    s.set_preconditioner(None)
    assert s.mg_levels() == []
    assert lib.cgamd_solver_mg_aggregates(s.handle, 0, None, ctypes.byref(nc)) == L.ERR_STATE
    s.close()


def test_handles_the_entry_does_not_serve(pkg, gpu):
    """batched, Hermitian (complex), row-major and unfused handles: CGAMD_ERR_STATE, and they solve as before"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    A = mg_ref.laplace3d(24, 24, 1)
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
            assert amg_status(lib, s) == L.ERR_STATE
            assert b"set_preconditioner_amg" in lib.cgamd_last_error()
            assert lib.cgamd_solver_mg_levels(s.handle) == 0 and lib.cgamd_solver_preconditioner_source(s.handle) == 0
            got = s.solve(b, None, 5)
            assert same(got[0], want[0]) and same(got[1], want[1])
    finally:
        for s, _ in handles:
            s.close()
    # the real value types run the same recurrence with the flag: served
    s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, hermitian=True)
    s.set_preconditioner(("amg", {"min_rows": 32}))
    assert len(s.mg_levels()) >= 2
    s.close()


# ---- 10: the map of a grid hierarchy --------------------------------------------------------------------------------------------------
def test_aggregates_of_a_grid_hierarchy(pkg, gpu):
    dims = (7, 6, 5)
    s = solver(pkg, gpu[0], mg_ref.variable7(*dims), np.float32)
    s.set_preconditioner(("multigrid", dims, {"min_rows": 2}))
    levels = s.mg_levels()
    for l in range(len(levels) - 1):
        agg, nc = s.mg_aggregates(l)
        assert nc == levels[l + 1]["rows"]
        assert np.array_equal(agg, mg_ref.agg_map((levels[l]["nx"], levels[l]["ny"], levels[l]["nz"])))
    with pytest.raises(pkg.CgAmdError):
        s.mg_aggregates(len(levels) - 1)
    s.close()


# ---- 11: Python and command-line entries ----------------------------------------------------------------------------------------------
def test_pcg_entry(pkg, gpu):
    """Solver.pcg(b, M="amg"): the iteration the restatement stops in (one check either way), the preconditioner removed afterwards"""
    A = amg_ref.permuted(mg_ref.laplace3d(12, 10, 8))
    b = np.random.default_rng(11).standard_normal(A.shape[0])
    tol = 1e-8 * np.linalg.norm(b)
    H = amg_ref.Hierarchy(A, np.float64, min_rows=32)
    its_ref = amg_ref.pcg_count(A, b, lambda r: H.vcycle(r), tol)
    s = solver(pkg, gpu[0], A, np.float64)
    x, i = s.pcg(b, M=("amg", {"min_rows": 32}), tol=tol, maxit=200)
    assert abs(i + 1 - its_ref) <= 2 and np.linalg.norm(b - A @ x) <= 2.0 * tol
    assert s.mg_levels() == []
    s.close()


def test_cli_amg(pkg, gpu, tmp_path):
    """oclcgex file.mtx 1 0 20 --double --amg --history F on a Matrix-Market file: the history of the Python handle; refused with
    --mixed"""
    A = amg_ref.zaniso(12, 10, 8)
    n = A.shape[0]
    low = sp.tril(A).tocoo()
    p, hp = str(tmp_path / "z100.mtx"), str(tmp_path / "history.bin")
    pkg.mmio.mmwrite(p, n, low.row, low.col, low.data, "real", "symmetric")
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "oclcgex")
    r = subprocess.run([exe, p, "1", "0", "20", "--double", "--amg", "--history", hp], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    s = solver(pkg, gpu[0], A, np.float64)
    s.set_preconditioner("amg")
    launches = pkg._lib.load().cgamd_solver_loop_launches(s.handle)
    assert f"multigrid: {len(s.mg_levels())} levels, {launches} launches per iteration" in r.stdout
    _, want = s.solve(np.full(n, 5.0), None, 20)
    s.close()
    h = np.fromfile(hp, dtype=np.float64)
    assert h.shape == (21,) and np.allclose(h, want[:, 0], rtol=1e-12, atol=0.0)
    bad = subprocess.run([exe, p, "1", "0", "20", "--double", "--amg", "--mixed", "--tol", "1e-8"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--amg" in bad.stderr
