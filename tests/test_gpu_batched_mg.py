"""Multigrid PCG on the batched handle (cgamd_solver_set_preconditioner_batched_multigrid; csrc/multigrid_batched.hip and
csrc/multigrid_setup.cpp): one hierarchy per system on shared aggregates and patterns.

Oracles: for the setup, a single-system handle made from A_r with the same arguments (bit for bit: the sums have a stated order); for
the cycle and the PCG loop, the host restatement mg_ref.Hierarchy(A_r, ...) per system with the rules and tolerances of
test_gpu_multigrid.py (check_cycle's bound, check_run's tolerances and keep mask).  Nothing is tuned to a device result.

The systems of every test but the convergence one: NSYS = 3 on one pattern, A_r = mg_ref.variable7(*dims, seed=3 + r) plus (0, 1, 4)[r]
on the diagonal, times (1 + 0.05j) for the complex types, min_rows 32.  On 13 x 11 x 9 that gives four levels (1287, 210, 36, 8 rows)
and per-system bounds of 2.65 / 2.33 / 1.75 on level 0 and 1.47 / 1.35 / 1.23 on level 3 (mg_ref): a cycle that used one system's
coefficients for all is off by tens of per cent."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import mg_ref
from test_gpu_multigrid import check_run, cycle_error, rhs, same, solver

pytestmark = pytest.mark.gpu
ALL = [np.float32, np.float64, np.complex64, np.complex128]
NSYS = 3
SHIFT = (0.0, 1.0, 4.0)
OPTS = {"min_rows": 32}
DIMS = (13, 11, 9)

_SYS, _HIER = {}, {}


def systems(dims, dtype, shift=SHIFT):
    """[A_0, A_1, A_2] in the wide type on one pattern, made once"""
    key = (dims, np.dtype(dtype).kind == "c", shift)
    if key not in _SYS:
        out = []
        for r in range(NSYS):
            A = sp.csr_matrix(mg_ref.variable7(*dims, seed=3 + r) + shift[r] * sp.identity(int(np.prod(dims))))
            if key[1]:
                A = sp.csr_matrix(A * (1.0 + 0.05j))
            A.sort_indices()
            out.append(A)
        assert all(np.array_equal(A.indptr, out[0].indptr) and np.array_equal(A.indices, out[0].indices) for A in out)
        _SYS[key] = out
    return _SYS[key]


def hierarchies(dims, dtype, opts=OPTS):
    key = (dims, np.dtype(dtype).name, tuple(sorted(opts.items())))
    if key not in _HIER:
        _HIER[key] = [mg_ref.Hierarchy(A, dims, dtype, **opts) for A in systems(dims, dtype)]
    return _HIER[key]


def batched(pkg, ctx, mats, dtype, flags=0, **kw):
    ip, ix = mats[0].indptr.astype(np.int32), mats[0].indices.astype(np.int32)
    stack = np.concatenate([A.data for A in mats]).astype(dtype)
    return pkg.Solver(ctx, mats[0].shape[0], len(ix), stack, ip, ix, len(mats), flags=flags, batched=True, **kw)


def mg_status(lib, s, nx, ny, nz, steps=0, omega=0.0, min_rows=0):
    return lib.cgamd_solver_set_preconditioner_batched_multigrid(s.handle, nx, ny, nz, steps, ctypes.c_double(omega), min_rows)


# ---- 1. the setup, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("dims,min_rows", [((7, 6, 5), 2), ((9, 7, 1), 2), ((13, 1, 1), 2), (DIMS, 32)])
def test_setup_has_the_bits_of_single_system_handles(pkg, gpu, dims, min_rows, dtype):
    """every level and system: ptr, cols, the value bits and the bits of the bound are those of a single-system handle made from A_r
    with the same arguments; level 0 is the caller's arrays"""
    ctx = gpu[0]
    mats = systems(dims, dtype)
    M = ("multigrid", dims, {"min_rows": min_rows})
    s = batched(pkg, ctx, mats, dtype)
    s.set_preconditioner(M)
    levels = s.mg_levels()
    assert s.preconditioner_source == 2
    if dims == DIMS:
        assert [L["rows"] for L in levels] == [1287, 210, 36, 8]
    got = [s.mg_level_matrix(l) for l in range(len(levels))]
    bounds = [s.mg_level_bounds(l) for l in range(len(levels))]
    agg = [s.mg_aggregates(l) for l in range(len(levels) - 1)]
    info = (ctypes.c_longlong * 6)()
    for l in range(len(levels)):                    # info[5] of the level: the bits of the LARGEST bound
        pkg._lib.check(pkg._lib.load().cgamd_solver_mg_level(s.handle, l, info))
        assert np.array([info[5]], dtype=np.int64).view(np.float64)[0] == bounds[l].max()
    s.close()
    for l, L in enumerate(levels):
        assert L["lmax"] == [float(v) for v in bounds[l]] and got[l][2].shape == (NSYS, L["nnz"])
    for r, A in enumerate(mats):
        one = solver(pkg, ctx, A, dtype)
        one.set_preconditioner(M)
        single = one.mg_levels()
        assert [(L["rows"], L["nnz"], L["nx"], L["ny"], L["nz"]) for L in single] == [(L["rows"], L["nnz"], L["nx"], L["ny"], L["nz"]) for L in levels]
        for l in range(len(levels)):
            ip, ix, da = one.mg_level_matrix(l)
            assert np.array_equal(ip, got[l][0]) and np.array_equal(ix, got[l][1]), (r, l)
            assert same(da, got[l][2][r]), (r, l, np.dtype(dtype).name)
            assert same(one.mg_level_bounds(l), bounds[l][r:r + 1]), (r, l, one.mg_level_bounds(l), bounds[l])
            assert levels[l]["lmax"][r] == single[l]["lmax"]
            if l + 1 < len(levels):
                a1, n1 = one.mg_aggregates(l)
                assert n1 == agg[l][1] and np.array_equal(a1, agg[l][0])
        if r == 0:
            assert same(got[0][2][0], A.data.astype(dtype))
        one.close()
    if dims == DIMS and np.dtype(dtype) == np.dtype(np.float64):
        H = hierarchies(dims, dtype)
        for r in range(NSYS):
            for l in (0, 3):
                assert abs(bounds[l][r] - H[r].levels[l].lmax) <= 1e-13 * H[r].levels[l].lmax
        assert bounds[0][0] > 1.1 * bounds[0][1] > 1.1 * 1.1 * bounds[0][2]       # the systems differ by tens of per cent


# ---- 2. the cycle alone -----------------------------------------------------------------------------------------------------------------
def check_cycle_per_system(pkg, ctx, s, mats, H, B, dims, dtype, M, label):
    """column r against the hierarchy of A_r by the rule of test_gpu_multigrid.check_cycle: error against the extended-precision cycle
    <= 4 max(error of the cycle in the value type, 4 eps).  Whether the column has the BITS of the single-system cycle is printed, not
    asserted: it depends on the summation order of the batched SpMV"""
    z = s.mg_apply(B.reshape(-1)).reshape(B.shape)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    figures = []
    for r in range(B.shape[0]):
        z_ref = H[r].vcycle(B[r], mg_ref.wide(dtype, True))
        e_dev, e_type = cycle_error(z[r], z_ref), cycle_error(H[r].vcycle(B[r], dtype), z_ref)
        one = solver(pkg, ctx, mats[r], dtype)
        one.set_preconditioner(M)
        z1 = one.mg_apply(B[r])
        one.close()
        print(f"  batched V-cycle {label} {np.dtype(dtype).name} system {r}: e(z) {e_dev:.3e}, e(z in type) {e_type:.3e}, "
              f"bound {4.0 * max(e_type, 4.0 * eps):.3e}; bits of the single-system cycle: {same(z1, z[r])}"
              f" (max difference {np.max(np.abs(z1 - z[r])):.3e})")
        figures.append((e_dev, e_type))
    for r, (e_dev, e_type) in enumerate(figures):
        assert e_dev <= 4.0 * max(e_type, 4.0 * eps), (label, np.dtype(dtype).name, r, e_dev, e_type)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("dims", [DIMS, (16, 16, 16)])
def test_vcycle_alone(pkg, gpu, dims, dtype):
    ctx = gpu[0]
    mats, H = systems(dims, dtype), hierarchies(dims, dtype)
    M = ("multigrid", dims, OPTS)
    s = batched(pkg, ctx, mats, dtype)
    s.set_preconditioner(M)
    assert len(s.mg_levels()) == len(H[0].levels) == 4
    check_cycle_per_system(pkg, ctx, s, mats, H, rhs(dims, dtype, NSYS), dims, dtype, M, "x".join(map(str, dims)))
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_vcycle_more_smoothing_steps_and_one_level(pkg, gpu, dtype):
    """two and three smoothing steps (the later Chebyshev steps read both coefficients of their column) and a hierarchy of one level"""
    ctx = gpu[0]
    mats = systems(DIMS, dtype)
    s = batched(pkg, ctx, mats, dtype)
    for opts in ({"min_rows": 32, "smooth_steps": 2, "over_correction": 1.0}, {"min_rows": 32, "smooth_steps": 3}, {"min_rows": 5000}):
        M = ("multigrid", DIMS, opts)
        s.set_preconditioner(M)
        H = hierarchies(DIMS, dtype, opts)
        assert len(s.mg_levels()) == len(H[0].levels)
        check_cycle_per_system(pkg, ctx, s, mats, H, rhs(DIMS, dtype, NSYS), DIMS, dtype, M, str(opts))
    s.close()


# ---- 3. fixed-count PCG -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
def test_fixed_count_pcg(pkg, gpu, dtype):
    """8 iterations; x and the history of system r against pcg_sparse(A_r, b_r, solve=H_r.solve())"""
    ctx = gpu[0]
    lib = pkg._lib.load()
    mats, H = systems(DIMS, dtype), hierarchies(DIMS, dtype)
    B = rhs(DIMS, dtype, NSYS)
    n = mats[0].shape[0]
    s = batched(pkg, ctx, mats, dtype)
    s.set_preconditioner("jacobi")
    jacobi_bytes = lib.cgamd_solver_iter_moved_bytes(s.handle)
    s.set_preconditioner(("multigrid", DIMS, OPTS))
    assert lib.cgamd_solver_preconditioner_source(s.handle) == 2
    assert lib.cgamd_solver_loop_launches(s.handle) == 5 + 1 + 5 * 3 + 14      # four levels, one smoothing step
    assert lib.cgamd_solver_iter_moved_bytes(s.handle) >= jacobi_bytes > 0
    assert lib.cgamd_solver_iter_bytes(s.handle, 1) >= jacobi_bytes
    x, h = s.solve(B.reshape(-1), None, 8)
    s.close()
    for r in range(NSYS):
        check_run(x[r * n:(r + 1) * n], h[:, r:r + 1], mats[r], sp.identity(n), B[r:r + 1], 8, dtype, solve=H[r].solve())


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------
def test_bits(pkg, gpu):
    """run to run; iterate(3) + iterate(5) = iterate(8); plain launches = graphs; a permuted batch is the permuted result; set then
    removed = a fresh handle; it replaces and is replaced by "jacobi" and ("line", 1) with the bits of a handle that had only the last"""
    ctx, L = gpu[0], pkg._lib
    mats = systems(DIMS, np.float64)
    B = rhs(DIMS, np.float64, NSYS)
    n = mats[0].shape[0]
    M = ("multigrid", DIMS, OPTS)

    def run(flags=0, split=(8,), m=M, before=None, perm=(0, 1, 2)):
        s = batched(pkg, ctx, [mats[p] for p in perm], np.float64, flags=flags)
        if before is not None:
            s.set_preconditioner(before)
        s.set_preconditioner(m)
        s.set_rhs(B[list(perm)].reshape(-1))
        for k in split:
            s.iterate(k)
        out = (s.x(), s.history(), len(s.mg_levels()), s.preconditioner_source)
        s.close()
        return out

    x0, h0, nl, src = run()
    assert nl == 4 and src == 2
    for other in (run(), run(split=(3, 5)), run(flags=L.NO_GRAPH), run(before="jacobi"), run(before=("line", 1))):
        assert same(other[0], x0) and same(other[1], h0)
    perm = (2, 0, 1)
    xp, hp = run(perm=perm)[:2]
    assert not same(xp, x0)
    for k, p in enumerate(perm):
        assert same(xp[k * n:(k + 1) * n], x0[p * n:(p + 1) * n]) and same(hp[:, k], h0[:, p]), (k, p)
    plain = run(m=None)
    assert plain[2] == 0 and plain[3] == 0 and not same(plain[0], x0)
    back = run(m=None, before=M)
    assert same(back[0], plain[0]) and same(back[1], plain[1]) and back[2] == 0
    for other in ("jacobi", ("line", 1)):
        alone, after = run(m=other), run(m=other, before=M)
        assert same(after[0], alone[0]) and same(after[1], alone[1]) and after[2] == 0 and not same(alone[0], x0)


# ---- 5. iterate_until -------------------------------------------------------------------------------------------------------------------
def test_until_three_tolerances(pkg, gpu):
    """a tolerance per system: each column stops on its own and holds the bits of iterate(its_r)"""
    ctx = gpu[0]
    mats = systems(DIMS, np.float64)
    B = rhs(DIMS, np.float64, NSYS)
    n = mats[0].shape[0]
    tol = np.array([1e-3, 1e-9, 1e-6]) * np.linalg.norm(B, axis=1)
    s = batched(pkg, ctx, mats, np.float64)
    s.set_preconditioner(("multigrid", DIMS, OPTS))
    x, its, h = s.solve_until(B.reshape(-1), tol=tol, maxit=200, check_every=4)
    assert its[2] < its[0] < its[1] < 200           # (the restatement: 6, 7 and 15 iterations)
    for r in range(NSYS):
        norms = np.sqrt(np.abs(h[:, r]))
        assert its[r] == int(np.flatnonzero(~(norms[1:] >= tol[r]))[0]) + 1
        s.set_rhs(B.reshape(-1))
        s.iterate(int(its[r]))
        assert same(s.x()[r * n:(r + 1) * n], x[r * n:(r + 1) * n]), r
    s.close()


# ---- 6. refresh_values and reload_matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_refresh_and_reload_rebuild_every_hierarchy(pkg, gpu, dtype):
    """system 1 scaled by 2 in place in a borrowed device array, then refresh_values; the same values through reload_matrix on a handle
    that owns its matrix: the bits of a fresh handle on the new values, the coarse values of system 1 doubled, the others untouched"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    mats = systems(dims, dtype)
    M = ("multigrid", dims, OPTS)
    ip, ix = mats[0].indptr.astype(np.int32), mats[0].indices.astype(np.int32)
    n, nnz = mats[0].shape[0], len(ix)
    stack = np.concatenate([A.data for A in mats]).astype(dtype)
    stack2 = stack.copy()
    stack2[nnz:2 * nnz] *= 2
    b = rhs(dims, dtype, NSYS).reshape(-1)

    fresh = pkg.Solver(ctx, n, nnz, stack2, ip, ix, NSYS, batched=True)
    fresh.set_preconditioner(M)
    want = fresh.solve(b, None, 6)
    fresh.close()

    dv, dp, dc = (pkg.DeviceBuffer(ctx, hostbuf=a) for a in (stack, ip, ix))
    s = pkg.Solver(ctx, n, nnz, dv, dp, dc, NSYS, flags=L.MATRIX_ON_DEVICE, dtype=dtype, batched=True)
    s.set_preconditioner(M)
    first = s.solve(b, None, 6)
    m1 = [s.mg_level_matrix(l) for l in range(len(s.mg_levels()))]
    assert len(m1) >= 3 and not same(first[0], want[0])
    L.check(lib.cgamd_memcpy_h2d(ctx.handle, L.ptr(dv), L.ptr(stack2), stack2.nbytes))
    s.refresh_values(None)
    assert s.preconditioner_source == 2 and len(s.mg_levels()) == len(m1)
    for l, (p1, c1, v1) in enumerate(m1):
        p2, c2, v2 = s.mg_level_matrix(l)
        assert np.array_equal(p1, p2) and np.array_equal(c1, c2), l
        assert same(v2[1], (2 * v1[1]).astype(dtype)) and same(v2[0], v1[0]) and same(v2[2], v1[2]), l
    got = s.solve(b, None, 6)
    assert same(got[0], want[0]) and same(got[1], want[1])
    s.close()
    for buf in (dv, dp, dc):
        buf.release()

    own = pkg.Solver(ctx, n, nnz, stack, ip, ix, NSYS, batched=True)
    own.set_preconditioner(M)
    own.solve(b, None, 6)
    own.reload_matrix(stack2, ip, ix)
    assert own.preconditioner_source == 2 and len(own.mg_levels()) == len(m1)
    got = own.solve(b, None, 6)
    assert same(got[0], want[0]) and same(got[1], want[1])
    # values the hierarchies cannot be built from: loaded, the preconditioner removed, the error names system, level and row
    bad = stack2.copy()
    row = 4
    bad[2 * nnz + ip[row]:2 * nnz + ip[row + 1]][ix[ip[row]:ip[row + 1]] == row] = 0
    with pytest.raises(pkg.CgAmdError, match=r"refresh_values: zero, missing or non-finite diagonal in system 2 level 0 row 4"):
        own.refresh_values(bad)
    assert own.mg_levels() == [] and own.preconditioner_source == 0
    own.close()


# ---- 7. convergence ---------------------------------------------------------------------------------------------------------------------
def test_convergence_against_jacobi(pkg, gpu):
    """24 x 20 x 16, the unshifted systems, fp64, to 1e-8 ||b||: every system stops in the first iteration that meets its tolerance and
    its multigrid count is at most half its count under "jacobi" on the same handle (the restatement alone: 18 against 52-53)"""
    ctx = gpu[0]
    dims = (24, 20, 16)
    mats = systems(dims, np.float64, shift=(0.0, 0.0, 0.0))
    n = mats[0].shape[0]
    B = rhs(dims, np.float64, NSYS)
    tol = 1e-8 * np.linalg.norm(B, axis=1)
    s = batched(pkg, ctx, mats, np.float64)
    s.set_preconditioner(("multigrid", dims))
    x, its_mg, h = s.solve_until(B.reshape(-1), tol=tol, maxit=400)
    s.set_preconditioner("jacobi")
    _, its_j, _ = s.solve_until(B.reshape(-1), tol=tol, maxit=400)
    s.close()
    print(f"24 x 20 x 16 to 1e-8 ||b||: multigrid PCG {list(map(int, its_mg))} iterations, Jacobi PCG {list(map(int, its_j))}")
    for r in range(NSYS):
        norms = np.sqrt(np.abs(h[:, r]))
        assert its_mg[r] == int(np.flatnonzero(~(norms[1:] >= tol[r]))[0]) + 1
        assert np.linalg.norm(B[r] - mats[r] @ x[r * n:(r + 1) * n]) <= 2.0 * tol[r]
        assert 2 * int(its_mg[r]) <= int(its_j[r]) < 400, (r, its_mg, its_j)


# ---- 8. errors and refusals -------------------------------------------------------------------------------------------------------------
def test_setup_errors_name_system_level_and_row(pkg, gpu):
    """a zero diagonal in system 1 only, and one that appears only on level 1 of system 2; the preconditioner set before keeps its bits"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    n = 16
    T = sp.csr_matrix(sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]))
    T.sort_indices()
    ip, ix = T.indptr.astype(np.int32), T.indices.astype(np.int32)

    def with_diag(values):
        d = T.data.copy()
        for i, v in values.items():
            d[ip[i]:ip[i + 1]][ix[ip[i]:ip[i + 1]] == i] = v
        return d

    b = np.tile(np.linspace(1.0, 2.0, n), NSYS)
    cases = (([T.data, with_diag({5: 0.0}), T.data], b"zero, missing or non-finite diagonal in system 1 level 0 row 5"),
             # aggregate 3 = rows 6, 7: 1 + 1 - 1 - 1 = 0 on level 1 only
             ([T.data, T.data, with_diag({6: 1.0, 7: 1.0})], b"zero, missing or non-finite diagonal in system 2 level 1 row 3"))
    for vals, text in cases:
        s = pkg.Solver(ctx, n, len(ix), np.concatenate(vals), ip, ix, NSYS, batched=True)
        s.set_preconditioner(np.full((NSYS, n), 0.5))
        want = s.solve(b, None, 4)
        assert mg_status(lib, s, n, 1, 1, 0, 0.0, 2) == L.ERR_INVALID
        assert text in lib.cgamd_last_error() and b"set_preconditioner_batched_multigrid" in lib.cgamd_last_error(), lib.cgamd_last_error()
        assert s.preconditioner_source == 1 and s.mg_levels() == []
        got = s.solve(b, None, 4)
        assert same(got[0], want[0]) and same(got[1], want[1])
        s.close()


def test_invalid_arguments_and_refused_calls(pkg, gpu):
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    mats = systems(dims, np.float64)
    b = rhs(dims, np.float64, NSYS).reshape(-1)
    s = batched(pkg, ctx, mats, np.float64)
    s.set_preconditioner(("multigrid", dims, OPTS))
    want = s.solve(b, None, 6)
    for args in ((9, 7, 4), (9, 7, 6), (0, 7, 45), (9, -7, -5), (315, 1, 0), (9, 7, 5, 5), (9, 7, 5, -1), (9, 7, 5, 0, float("nan")),
                 (9, 7, 5, 0, -1.0), (9, 7, 5, 0, float("inf")), (9, 7, 5, 0, 0.0, -1)):
        assert mg_status(lib, s, *args) == L.ERR_INVALID, args
        assert b"set_preconditioner_batched_multigrid" in lib.cgamd_last_error()
    out = (ctypes.c_double * NSYS)()
    assert lib.cgamd_solver_mg_level_bounds(s.handle, 7, out, NSYS) == L.ERR_INVALID
    assert lib.cgamd_solver_mg_level_bounds(s.handle, 0, out, NSYS + 1) == L.ERR_INVALID
    got = s.solve(b, None, 6)
    assert same(got[0], want[0]) and same(got[1], want[1]) and len(s.mg_levels()) == 3
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
    assert s.mg_levels() == [] and lib.cgamd_solver_mg_level_bounds(s.handle, 0, out, 1) == L.ERR_STATE
    s.close()


def test_handles_the_entry_does_not_serve(pkg, gpu):
    """a handle that is not batched is sent to the single entry; Hermitian (complex) and unfused batched handles: CGAMD_ERR_STATE, and
    they solve as before"""
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    dims = (9, 7, 5)
    mats = systems(dims, np.complex128)
    real = systems(dims, np.float64)
    n = mats[0].shape[0]
    handles = [(solver(pkg, ctx, real[0], np.float64, NSYS), b"use cgamd_solver_set_preconditioner_multigrid"),
               (batched(pkg, ctx, [sp.csr_matrix(A.real) for A in mats], np.complex128, hermitian=True), b"CGAMD_HERMITIAN"),
               (batched(pkg, ctx, real, np.float64, flags=L.UNFUSED), b"CGAMD_UNFUSED")]
    try:
        for s, text in handles:
            b = rhs(dims, s.dtype, NSYS).reshape(-1)
            want = s.solve(b, None, 5)
            assert mg_status(lib, s, *dims) == L.ERR_STATE
            assert text in lib.cgamd_last_error() and b"set_preconditioner_batched_multigrid" in lib.cgamd_last_error(), lib.cgamd_last_error()
            assert lib.cgamd_solver_mg_levels(s.handle) == 0 and s.preconditioner_source == 0
            got = s.solve(b, None, 5)
            assert same(got[0], want[0]) and same(got[1], want[1])
    finally:
        for s, _ in handles:
            s.close()
    # the real value types run the same recurrence with the flag: served; and a batch of one system
    s = batched(pkg, ctx, real[:1], np.float64, hermitian=True)
    s.set_preconditioner(("multigrid", dims, OPTS))
    assert len(s.mg_levels()) == 3 and len(s.mg_levels()[0]["lmax"]) == 1
    s.close()


# ---- 9. solve_subdomains ----------------------------------------------------------------------------------------------------------------
def test_solve_subdomains_with_multigrid(pkg, gpu):
    """three sub-domain matrices in complex64: per sub-domain the bits of the batched handle set up by hand, and not those of the
    unpreconditioned call"""
    ctx = gpu[0]
    mats = systems(DIMS, np.complex64)
    n = mats[0].shape[0]
    B = rhs(DIMS, np.complex64, NSYS)
    res = [B[r] for r in range(NSYS)]
    M = ("multigrid", DIMS, OPTS)
    out = pkg.solve_subdomains(ctx, mats, res, 8, dtype=np.complex64, preconditioner=M)
    plain = pkg.solve_subdomains(ctx, mats, res, 8, dtype=np.complex64)
    s = batched(pkg, ctx, mats, np.complex64)
    s.set_preconditioner(M)
    x, _ = s.solve(B.reshape(-1), None, 8)
    s.close()
    for r in range(NSYS):
        assert out[r].shape == (n,) and same(out[r], x[r * n:(r + 1) * n].astype(complex)), r
        assert not same(plain[r], out[r])
