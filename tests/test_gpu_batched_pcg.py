"""Preconditioned CG on the batched handle: one M per system (cgamd_solver_set_preconditioner_batched, _batched_jacobi, _batched_line;
Solver.set_preconditioner on a batched handle; solve_subdomains(..., preconditioner=)).

Oracle: tridiag_pcg.pcg_sparse(A_r, b_r, M_r, tol=0, maxit=k, history=True, solve=splu(M_r)) per system -- the restated reference PCG
test_gpu_line_from_matrix.py uses, with M_r cut from A_r by scipy (tp.band for stride 1, the entries at |i - j| in {0, s} otherwise,
diags(A_r.diagonal()) for Jacobi).  Tolerances are that file's: x error below 1e-9 and history error below 1e-10 in fp64 / complex128,
1e-4 / 1e-4 in fp32 / complex64, the history compared while |delta_k / delta_0| > 1e-8 (wide) or 1e-4 (narrow).  The restatement run
with vectors rounded to fp32 / complex64 against itself in complex128 stays at or below 4.9e-7 (history) and 2.5e-7 (x) on the grids and
3.3e-7 / 1.3e-7 on the "different cuts" systems, so the narrow bounds hold with a margin of 200; nothing is tuned to a device result.

Systems on one pattern are test_gpu_batched's: a_r[j] = a[j] s[row(j)] s[col(j)], seeds 100 + r.  A mix-up of systems cannot pass:
solving A_r with M_(r+1) moves delta_1 by 20 % (Jacobi) or by 8x (line)."""
import ctypes
import types

import numpy as np
import pytest
import scipy.sparse as sp

import tridiag_pcg as tp
from test_gpu_batched import batched, pattern, scaled
from test_gpu_line_from_matrix import GRIDS, laplace3d, lines, lu_solve, tols

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
ALL = list(DT)
NSYS = 3
ITERS = 12


def is_cplx(dtype):
    return np.dtype(dtype).kind == "c"


def cut(A, s):
    """M of the line form at stride s, as scipy cuts it from A"""
    return tp.band(A) if s == 1 else lines(A, s)


def oracle(mats, Ms, B, iters):
    """the restated reference PCG, system r with its own A_r, M_r and b_r: [(x, history)]"""
    out = []
    for A, M, b in zip(mats, Ms, B):
        xo, _, ho = tp.pcg_sparse(A, b.astype(complex), M, tol=0.0, maxit=iters, history=True, solve=lu_solve(M))
        out.append((xo, ho))
    return out


def check_run(x, h, ref, dtype, label=""):
    """x / history of a device run against [(x, history)] per system; every figure is printed before it is asserted.  Returns the
    smallest number of history entries compared."""
    xt, ht = tols(dtype)
    n = ref[0][0].size
    kept, figures = [], []
    for r, (xo, ho) in enumerate(ref):
        keep = np.abs(ho) / np.abs(ho[0]) > (1e-8 if xt < 1e-6 else 1e-4)
        herr = np.max(np.abs(h[keep, r] - ho[keep]) / np.abs(ho[keep]))
        xerr = np.linalg.norm(x[r * n:(r + 1) * n] - xo) / np.linalg.norm(xo)
        print(f"  {label} n={n} {np.dtype(dtype).name} system {r}: {int(keep.sum())} history entries compared, history err "
              f"{herr:.3e} (< {ht:g}), x err {xerr:.3e} (< {xt:g})")
        kept.append(int(keep.sum()))
        figures.append((herr, xerr))
    for r, (herr, xerr) in enumerate(figures):
        assert herr < ht, (label, r, dtype, herr)
        assert xerr < xt, (label, r, dtype, xerr)
    return min(kept)


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


# ---- the grid systems: laplace3d with one strong axis, three scalings, made once --------------------------------------------------
_GRID = {}


def grid_systems(grid, axis, cplx, seeds=(100, 101, 102)):
    key = (grid, axis, cplx, seeds)
    if key not in _GRID:
        nx, ny, nz = grid
        A = laplace3d(nx, ny, nz, **{"c" + axis: 10.0})
        if cplx:
            A = sp.csr_matrix(A * (1.0 + 0.05j))
        A.sort_indices()
        ip, ix = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        n = A.shape[0]
        vals = [scaled(ip, A.data, ix, sd) for sd in seeds]
        rng = np.random.default_rng(11)
        B = rng.standard_normal((len(seeds), n))
        if cplx:
            B = B * (1.0 + 0.3j * rng.standard_normal((len(seeds), n)))      # phase-controlled: |b.b| stays near 0.8 b^H b
        _GRID[key] = types.SimpleNamespace(ip=ip, ix=ix, n=n, vals=vals, B=B, s={"x": 1, "y": nx, "z": nx * ny}[axis],
                                           mats=[sp.csr_matrix((v, ix, ip), shape=(n, n)) for v in vals], ref={})
    return _GRID[key]


def grid_ref(c, kind):
    """the oracle runs of a grid case under "jacobi" or "line", made once"""
    if kind not in c.ref:
        Ms = [sp.diags(A.diagonal()).tocsr() if kind == "jacobi" else cut(A, c.s) for A in c.mats]
        c.ref[kind] = oracle(c.mats, Ms, c.B, ITERS)
    return c.ref[kind]


def solve(s, c, dtype, iters=(ITERS,)):
    s.set_rhs(c.B.reshape(-1).astype(dtype))
    for k in iters:
        s.iterate(k)
    return s.x(), s.history()


# ---- 1. Jacobi parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("grid", GRIDS)
def test_jacobi_parity(pkg, gpu, grid, dt):
    """m_r = 1 / diag(A_r) built on the device (source 2), then the same handle with the caller's array: host, then device"""
    dtype = DT[dt]
    ctx = gpu[0]
    lib = pkg._lib.load()
    c = grid_systems(grid, "x", is_cplx(dtype))
    ref = grid_ref(c, "jacobi")
    m = np.stack([1.0 / A.diagonal() for A in c.mats]).astype(dtype)
    s = batched(pkg, ctx, c.ip, c.ix, c.vals, dtype)
    try:
        assert s.preconditioner_source == 0
        s.set_preconditioner("jacobi")
        assert s.preconditioner_source == 2 and lib.cgamd_solver_loop_launches(s.handle) == 4
        x, h = solve(s, c, dtype)
        check_run(x, h, ref, dtype, "jacobi from the matrices")
        s.set_preconditioner(m)                       # (n_rhs, size)
        assert s.preconditioner_source == 1 and lib.cgamd_solver_loop_launches(s.handle) == 4
        x1, h1 = solve(s, c, dtype)
        check_run(x1, h1, ref, dtype, "host array")
        buf = pkg.DeviceBuffer(ctx, hostbuf=m.reshape(-1))
        s.set_preconditioner(buf)
        assert s.preconditioner_source == 1
        x2, h2 = solve(s, c, dtype)
        buf.release()
        check_run(x2, h2, ref, dtype, "device pointer")
        assert same_bits((x1, h1), (x2, h2)), "the same diagonals from the host and from the device give different bits"
    finally:
        s.close()
    # the systems differ and so do their preconditioners: delta_1 of two systems is percents apart
    assert abs(h[1, 0] - h[1, 1]) / abs(h[1, 0]) > 1e-3


@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_jacobi_parity_unfused(pkg, gpu, dt):
    """CGAMD_UNFUSED: the preconditioned loop keeps its four launches and takes alpha from d.q partials of its own SpMV"""
    dtype = DT[dt]
    lib = pkg._lib.load()
    c = grid_systems(GRIDS[1], "x", is_cplx(dtype))
    s = batched(pkg, gpu[0], c.ip, c.ix, c.vals, dtype, flags=pkg._lib.UNFUSED)
    try:
        s.set_preconditioner("jacobi")
        assert s.preconditioner_source == 2 and lib.cgamd_solver_loop_launches(s.handle) == 4
        x, h = solve(s, c, dtype)
    finally:
        s.close()
    check_run(x, h, grid_ref(c, "jacobi"), dtype, "jacobi, unfused")


# ---- 2. line parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_line_parity_x_y_and_z_lines(pkg, gpu, axis, grid, dt):
    """strides 1, nx and nx ny; 23 x 21 x 17 has an odd row count (a padding row in fp64 / complex64, three in fp32)"""
    dtype = DT[dt]
    lib = pkg._lib.load()
    c = grid_systems(grid, axis, is_cplx(dtype))
    s = batched(pkg, gpu[0], c.ip, c.ix, c.vals, dtype)
    try:
        s.set_preconditioner(("line", c.s))
        assert s.preconditioner_source == 2 and lib.cgamd_solver_loop_launches(s.handle) == 4
        x, h = solve(s, c, dtype)
    finally:
        s.close()
    check_run(x, h, grid_ref(c, "line"), dtype, f"{axis}-lines")
    assert abs(h[1, 0] - h[1, 1]) / abs(h[1, 0]) > 1e-3


# ---- 3. different cuts per system on one pattern, 4. the long form -------------------------------------------------------------------
_CUTS = {}


def cut_systems(n, s, nsys, shared_cuts, own_cuts, cplx):
    """pattern {0, +-1, +-5} and, for s = 7, +-7.  Diagonal 5.5 + U(0, 1), the couplings at distance s -U(0.2, 1), the others -0.8
    (s = 1, where there is no +-7 band: +-5 at -1.6, the same off-diagonal weight outside M, so that the narrow types keep at least
    four history entries above 1e-4 there too); shared_cuts couplings at distance s are zero in every system and own_cuts more at
    places of each system's own (seeds 300 + r).  The zeros stay stored, so that all systems share the pattern."""
    key = (n, s, nsys, shared_cuts, own_cuts, cplx)
    if key in _CUTS:
        return _CUTS[key]
    offs = sorted({0, 1, -1, 5, -5, s, -s})
    P = sp.csr_matrix(sp.diags([np.ones(n - abs(o)) for o in offs], offs, format="csr"))
    P.sort_indices()
    ip, ix = P.indptr.astype(np.int32), P.indices.astype(np.int32)
    rows = np.repeat(np.arange(n), np.diff(ip))
    dist = ix.astype(np.int64) - rows
    shared = np.random.default_rng(299).choice(n - s, size=shared_cuts, replace=False) if shared_cuts else np.zeros(0, int)
    vals, mats = [], []
    for r in range(nsys):
        rng = np.random.default_rng(300 + r)
        diag = 5.5 + rng.uniform(0.0, 1.0, n)
        off = -rng.uniform(0.2, 1.0, n - s)
        off[shared] = 0.0
        if own_cuts:
            off[rng.choice(n - s, size=own_cuts, replace=False)] = 0.0
        v = np.full(len(ix), -0.8 if s > 1 else -1.6)
        v[dist == 0] = diag
        at = np.abs(dist) == s
        v[at] = off[np.minimum(rows, ix)[at]]
        if cplx:
            v = v * (1.0 + 0.05j)
        A = sp.csr_matrix((v, ix, ip), shape=(n, n))
        vals.append(v)
        mats.append(A)
    for A in mats[1:]:                       # one pattern, although the systems' zeros lie at different places
        assert np.array_equal(A.indptr, mats[0].indptr) and np.array_equal(A.indices, mats[0].indices)
    if own_cuts:
        zeros = [set(np.flatnonzero(v == 0)) for v in vals]
        assert zeros[0] != zeros[1] and len(set.intersection(*zeros)) >= 2 * shared_cuts
    rng = np.random.default_rng(11)
    B = rng.standard_normal((nsys, n))
    if cplx:
        B = B * (1.0 + 0.3j * rng.standard_normal((nsys, n)))
    c = types.SimpleNamespace(ip=ip, ix=ix, n=n, vals=vals, mats=mats, B=B, s=s, ref=oracle(mats, [cut(A, s) for A in mats], B, 8))
    _CUTS[key] = c
    return c


@pytest.mark.parametrize("dt", ["f64", "c64"])
@pytest.mark.parametrize("n,s", [(3000, 7), (3001, 1)])
def test_different_cuts_per_system_on_one_pattern(pkg, gpu, n, s, dt):
    """10 couplings cut in every system and 40 more per system: the shared plan has the segments all systems agree on, and a system's
    own zero couplings inside one restart its recurrence by zero factors.  8 iterations"""
    dtype = DT[dt]
    lib = pkg._lib.load()
    c = cut_systems(n, s, NSYS, 10, 40, is_cplx(dtype))
    sv = batched(pkg, gpu[0], c.ip, c.ix, c.vals, dtype)
    try:
        sv.set_preconditioner(("line", s))
        assert sv.preconditioner_source == 2 and lib.cgamd_solver_loop_launches(sv.handle) == 4
        x, h = solve(sv, c, dtype, iters=(8,))
    finally:
        sv.close()
    kept = check_run(x, h, c.ref, dtype, f"own cuts, stride {s}")
    assert kept >= 4, kept


@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_long_form(pkg, gpu, dt):
    """a chain of 3000 rows without a cut is one segment, longer than a chunk of the scan sweep (1024 rows): maps, carry, apply"""
    dtype = DT[dt]
    lib = pkg._lib.load()
    c = cut_systems(3000, 1, 2, 0, 0, is_cplx(dtype))
    sv = batched(pkg, gpu[0], c.ip, c.ix, c.vals, dtype)
    try:
        sv.set_preconditioner(("line", 1))
        assert sv.preconditioner_source == 2 and lib.cgamd_solver_loop_launches(sv.handle) == 6
        V = np.dtype(dtype).itemsize
        matrix = len(c.ix) * (2 * V + 4) + 4 * (c.n + 1)
        assert sv.iter_moved_bytes == sv.iter_bytes(True) == matrix + (13 + 6) * c.n * V * 2
        x, h = solve(sv, c, dtype, iters=(8,))
    finally:
        sv.close()
    check_run(x, h, c.ref, dtype, "long form")


# ---- 5. bits -------------------------------------------------------------------------------------------------------------------------
FORMS = {"jacobi": lambda c: "jacobi", "line": lambda c: ("line", c.s)}


def run(pkg, ctx, c, dtype, form, iters=(ITERS,), flags=0, order=None, remove=False):
    order = list(range(len(c.vals))) if order is None else order
    cc = types.SimpleNamespace(B=c.B[order])
    s = batched(pkg, ctx, c.ip, c.ix, [c.vals[p] for p in order], dtype, flags=flags)
    try:
        if form is not None:
            s.set_preconditioner(form)
        if remove:
            s.set_preconditioner(None)
            assert s.preconditioner_source == 0
        return solve(s, cc, dtype, iters)
    finally:
        s.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_bits_are_stable(pkg, gpu, dt, form):
    dtype = DT[dt]
    ctx = gpu[0]
    c = grid_systems(GRIDS[1], "y", is_cplx(dtype))
    f = FORMS[form](c)
    n = c.n
    x12, h12 = run(pkg, ctx, c, dtype, f)
    assert np.all(np.isfinite(h12.view(np.float64 if dtype == np.float64 else np.float32)))
    assert same_bits(run(pkg, ctx, c, dtype, f), (x12, h12)), "results differ from run to run"
    assert same_bits(run(pkg, ctx, c, dtype, f, iters=(6, 6)), (x12, h12)), "iterate(6) twice differs from iterate(12)"
    assert same_bits(run(pkg, ctx, c, dtype, f, flags=pkg._lib.NO_GRAPH), (x12, h12)), "graph replay differs from plain launches"
    perm = [2, 0, 1]
    xp, hp = run(pkg, ctx, c, dtype, f, order=perm)
    assert np.array_equal(xp.reshape(3, n), x12.reshape(3, n)[perm]), "permuting the batch does not permute x"
    assert np.array_equal(hp, h12[:, perm]), "permuting the batch does not permute the history columns"
    assert not np.array_equal(xp, x12)
    plain = run(pkg, ctx, c, dtype, None)
    assert same_bits(run(pkg, ctx, c, dtype, f, remove=True), plain), "set, then removed: not the bits of a fresh handle"
    assert not same_bits(plain, (x12, h12))


# ---- 6. reload and borrowed values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_reload_rebuilds_the_preconditioner(pkg, gpu, dt, form):
    dtype = DT[dt]
    ctx = gpu[0]
    c = grid_systems(GRIDS[0], "y", is_cplx(dtype))
    c2 = grid_systems(GRIDS[0], "y", is_cplx(dtype), seeds=(200, 201, 202))
    f = FORMS[form](c)
    fresh = run(pkg, ctx, c2, dtype, f)
    s = batched(pkg, ctx, c.ip, c.ix, c.vals, dtype)
    try:
        s.set_preconditioner(f)
        first = solve(s, c, dtype)
        s.reload_matrix(np.concatenate(c2.vals), c.ip, c.ix)
        assert s.preconditioner_source == 2
        again = solve(s, c2, dtype)
    finally:
        s.close()
    assert same_bits(again, fresh), "after reload_matrix: not the bits of a fresh handle set up the same way"
    assert not same_bits(first, fresh)


@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_a_callers_array_survives_reload(pkg, gpu, dt):
    dtype = DT[dt]
    ctx = gpu[0]
    c = grid_systems(GRIDS[0], "y", is_cplx(dtype))
    c2 = grid_systems(GRIDS[0], "y", is_cplx(dtype), seeds=(200, 201, 202))
    m = np.stack([1.0 / A.diagonal() for A in c.mats]).astype(dtype)      # of the FIRST matrices: kept as it is
    fresh = run(pkg, ctx, c2, dtype, m)
    s = batched(pkg, ctx, c.ip, c.ix, c.vals, dtype)
    try:
        s.set_preconditioner(m.reshape(-1))
        solve(s, c, dtype)
        s.reload_matrix(np.concatenate(c2.vals), c.ip, c.ix)
        assert s.preconditioner_source == 1
        again = solve(s, c2, dtype)
    finally:
        s.close()
    assert same_bits(again, fresh)
    assert not same_bits(again, run(pkg, ctx, c2, dtype, "jacobi"))          # ... and not rebuilt from the new matrices


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_borrowed_device_values(pkg, gpu, dt, form):
    """CGAMD_MATRIX_ON_DEVICE: the preconditioner is built from the borrowed values; bits of the owning handle"""
    import torch
    dtype = DT[dt]
    ctx = gpu[0]
    c = grid_systems(GRIDS[1], "y", is_cplx(dtype))
    f = FORMS[form](c)
    own = run(pkg, ctx, c, dtype, f)
    dev = torch.device("cuda", 0)
    tv = torch.from_numpy(np.concatenate(c.vals).astype(dtype)).to(dev)
    tp_ = torch.from_numpy(c.ip).to(dev)
    tc = torch.from_numpy(c.ix).to(dev)
    torch.cuda.synchronize()
    s = pkg.Solver(ctx, c.n, len(c.ix), tv, tp_, tc, NSYS, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype, batched=True)
    try:
        s.set_preconditioner(f)
        assert s.preconditioner_source == 2
        got = solve(s, c, dtype)
    finally:
        s.close()
    assert same_bits(got, own)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def entry_at(c, row, col):
    j = np.flatnonzero(c.ix[c.ip[row]:c.ip[row + 1]] == col)
    assert j.size == 1
    return int(c.ip[row] + j[0])


def test_errors_name_the_system_and_the_row(pkg, gpu):
    dtype = np.float64
    ctx = gpu[0]
    lib, L = pkg._lib.load(), pkg._lib
    c = grid_systems(GRIDS[0], "x", False)
    m = np.stack([1.0 / A.diagonal() for A in c.mats]).astype(dtype)
    # system 1 has no diagonal in row 17 (and row 30 of system 2: the smaller system is named)
    vals = [v.copy() for v in c.vals]
    vals[1][entry_at(c, 17, 17)] = 0.0
    vals[1][entry_at(c, 25, 25)] = 0.0
    vals[2][entry_at(c, 3, 3)] = 0.0
    s = batched(pkg, ctx, c.ip, c.ix, vals, dtype)
    try:
        s.set_preconditioner(m)
        want = solve(s, c, dtype)
        assert lib.cgamd_solver_set_preconditioner_batched_jacobi(s.handle) == L.ERR_INVALID
        msg = lib.cgamd_last_error().decode()
        print("  ", msg)
        assert "system 1" in msg and "row 17" in msg and "diagonal" in msg
        for stride in (0, c.n, -1):
            assert lib.cgamd_solver_set_preconditioner_batched_line(s.handle, stride) == L.ERR_INVALID
            assert b"stride" in lib.cgamd_last_error()
        assert s.preconditioner_source == 1
        assert same_bits(solve(s, c, dtype), want), "a failed call changed the preconditioner in force"
    finally:
        s.close()
    # system 2 has the block [[1, 1], [1, 1]] at rows 40, 41, decoupled from row 39: u_40 = 1, l_41 = 1, u_41 = 1 - 1 = 0
    vals = [v.copy() for v in c.vals]
    for i, j, v in ((40, 40, 1.0), (40, 41, 1.0), (41, 40, 1.0), (41, 41, 1.0), (40, 39, 0.0), (39, 40, 0.0)):
        vals[2][entry_at(c, i, j)] = v
    s = batched(pkg, ctx, c.ip, c.ix, vals, dtype)
    try:
        s.set_preconditioner("jacobi")
        want = solve(s, c, dtype)
        assert lib.cgamd_solver_set_preconditioner_batched_line(s.handle, 1) == L.ERR_INVALID
        msg = lib.cgamd_last_error().decode()
        print("  ", msg)
        assert "zero or non-finite pivot" in msg and "system 2" in msg and "row 41" in msg
        assert s.preconditioner_source == 2
        assert same_bits(solve(s, c, dtype), want), "a failed call changed the preconditioner in force"
        ran = ctypes.c_int(-1)
        assert lib.cgamd_solver_iterate_tol(s.handle, 10, 1e-6, ctypes.byref(ran)) == L.ERR_STATE
        # reload_matrix with matrices the form in force cannot be built from: loaded, the preconditioner removed, the error returned
        bad = [v.copy() for v in c.vals]
        bad[0][entry_at(c, 5, 5)] = 0.0
        with pytest.raises(pkg.CgAmdError, match="system 0 row 5"):
            s.reload_matrix(np.concatenate(bad), c.ip, c.ix)
        assert s.preconditioner_source == 0
    finally:
        s.close()


def test_a_handle_that_is_not_batched_refuses_the_three_entries(pkg, gpu):
    dtype = np.float64
    ctx = gpu[0]
    lib, L = pkg._lib.load(), pkg._lib
    c = grid_systems(GRIDS[0], "x", False)
    b = c.B.reshape(-1)
    s = pkg.Solver(ctx, c.n, len(c.ix), c.vals[0], c.ip, c.ix, NSYS)
    try:
        want = s.solve(b, None, ITERS)
        s.set_rhs(b)
        s.iterate(4)
        m = np.ones(NSYS * c.n, dtype)
        got = {"batched": lib.cgamd_solver_set_preconditioner_batched(s.handle, L.ptr(m), 0),
               "batched_null": lib.cgamd_solver_set_preconditioner_batched(s.handle, None, 0),
               "batched_jacobi": lib.cgamd_solver_set_preconditioner_batched_jacobi(s.handle),
               "batched_line": lib.cgamd_solver_set_preconditioner_batched_line(s.handle, 1)}
        assert got == {k: L.ERR_STATE for k in got}, got
        assert b"cgamd_solver_set_preconditioner_line" in lib.cgamd_last_error()
        assert s.preconditioner_source == 0 and s.iterations_done() == 4
        s.iterate(ITERS - 4)                      # the solve goes on where it was
        assert same_bits((s.x(), s.history()), want)
    finally:
        s.close()


# ---- 8. contract ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("dt", ALL)
def test_contract_accessors_and_byte_models(pkg, gpu, dt, flags):
    dtype = DT[dt]
    lib = pkg._lib.load()
    c = grid_systems(GRIDS[1], "y", is_cplx(dtype))
    n, nnz, V = c.n, len(c.ix), np.dtype(dtype).itemsize
    matrix = nnz * (NSYS * V + 4) + 4 * (n + 1)
    s = batched(pkg, gpu[0], c.ip, c.ix, c.vals, dtype, flags=flags)
    try:
        for form, passes in (("jacobi", 12), (("line", c.s), 14 + 3), (("line", 1), 11 + 3)):
            s.set_preconditioner(form)
            assert s.systems == NSYS and lib.cgamd_solver_layout(s.handle) == 0
            assert lib.cgamd_solver_loop_launches(s.handle) == 4
            assert s.iter_moved_bytes == matrix + passes * n * V * NSYS, form
            assert s.iter_bytes(True) == matrix + passes * n * V * NSYS, form
            assert s.spmv_bytes == s.spmv_moved_bytes == matrix + 2 * n * V * NSYS
            solve(s, c, dtype, iters=(2,))
            assert lib.cgamd_solver_layout(s.handle) == 0 and lib.cgamd_solver_loop_launches(s.handle) == 4
        # the shared-M entry with NULL removes a per-system preconditioner too
        assert lib.cgamd_solver_set_preconditioner(s.handle, None, 0) == pkg._lib.OK and s.preconditioner_source == 0
        assert s.iter_moved_bytes == matrix + (14 if flags & 4 else 10) * n * V * NSYS
        assert lib.cgamd_solver_loop_launches(s.handle) == (8 if flags & 4 else 3)
    finally:
        s.close()


# ---- 9. solve_subdomains -------------------------------------------------------------------------------------------------------------
def test_solve_subdomains_with_a_preconditioner(pkg, gpu, golden):
    """three sub-domain matrices on one pattern, complex64, Jacobi per sub-domain: against three batched-of-one PCG solves"""
    ip, ix, a, b = pattern(golden, True)
    ctx = gpu[0]
    n = len(ip) - 1
    P = [types.SimpleNamespace(indptr=ip, indices=ix, data=scaled(ip, a, ix, 100 + r)) for r in range(3)]
    res = [(b * (1 + 0.25 * r)).reshape(32, 32) for r in range(3)]
    out = pkg.solve_subdomains(ctx, P, res, ITERS, preconditioner="jacobi")
    assert len(out) == 3 and all(o.shape == (32, 32) and o.dtype == np.complex128 for o in out)
    keep = pkg.Solver(ctx, n, len(ix), np.zeros(3 * len(ix), np.complex64), ip, ix, 3, batched=True)
    try:
        out2 = pkg.solve_subdomains(ctx, P, res, ITERS, solver=keep, preconditioner="jacobi")
        assert keep.preconditioner_source == 0, "the caller's handle keeps a preconditioner it did not ask for"
        plain = pkg.solve_subdomains(ctx, P, res, ITERS, solver=keep)
    finally:
        keep.close()
    for r in range(3):
        one = batched(pkg, ctx, ip, ix, [P[r].data], np.complex64)
        try:
            one.set_preconditioner("jacobi")
            x1, _ = one.solve(res[r].ravel().astype(np.complex64), None, ITERS)
        finally:
            one.close()
        rel = np.linalg.norm(out[r].ravel() - x1) / np.linalg.norm(x1)
        print(f"sub-domain {r}: relative difference to a batched-of-one PCG solve {rel:.3g}")
        assert rel < 1e-5
        assert np.array_equal(out2[r], out[r])
        assert not np.array_equal(plain[r], out[r])
