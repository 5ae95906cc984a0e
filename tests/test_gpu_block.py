"""Block CG on the GPU (cgamd_solver_set_block, csrc/block_cg.hip): the right-hand sides of one SPD matrix share one Krylov space.

Systems: the five-point Laplacians on 33 x 29 (957 rows, padded inside the handle) and 64 x 64, s in {2, 4, 9, 16} independent random
right-hand sides (default_rng(11)), float32 and float64.  The reference is tests/block_ref.py (the recurrence in numpy with the
kernels' own orders, itself held to separate CG solves by tests/test_block_ref.py), on the matrix and right-hand sides AS ROUNDED
to the handle's type.

Bounds after 10 block iterations.  The yardstick of float32 is the restatement run in float32 against itself run in float64, row by
row: D_k = max_j |delta_k[j] - delta64_k[j]| / delta64_k[j], and D_X = max_j |x_j - x64_j|_2 / |x64_j|_2; the GPU is within 4 D_k of
the float64 run in every history row and within 4 D_X in X.  float64 is held to what test_gpu_cg.py holds the plain loop to: every
delta_k within 1e-10 relative, X within 1e-9.
Measured D_k (float32, k = 0 .. 10; the smallest and the largest row of every case) and D_X:
    33 x 29  s =  2   D_k 1.3e-08 .. 1.6e-07   D_X 1.3e-07        64 x 64  s =  2   D_k 2.7e-08 .. 3.6e-07   D_X 1.2e-07
    33 x 29  s =  4   D_k 2.7e-08 .. 3.0e-07   D_X 2.0e-07        64 x 64  s =  4   D_k 2.3e-08 .. 6.5e-07   D_X 1.6e-07
    33 x 29  s =  9   D_k 1.9e-08 .. 6.6e-07   D_X 3.1e-07        64 x 64  s =  9   D_k 5.6e-08 .. 4.1e-07   D_X 2.2e-07
    33 x 29  s = 16   D_k 3.2e-08 .. 5.0e-07   D_X 3.7e-07        64 x 64  s = 16   D_k 5.6e-08 .. 7.6e-07   D_X 2.9e-07
(the smallest is row 0 -- one rounding of the history entry -- in every case but 33 x 29 at s = 2, where it is row 1; the rows grow
with k as the recurrence carries its roundings along.  The small rows are below the float32 unit roundoff of 6e-8 that the history
entry itself carries: the GPU meets them because its sums run in the restatement's order, not because the bound is loose -- measured
on the MI355X, its error against the float64 run is D_k itself in every row of every case (ratio 1.0) and D_X in X, and in float64
its history and X equal the restatement's exactly: on these matrices the handle's SpMV adds a row's products in CSR order, as scipy
does.)

Bits: iterate(3); iterate(7) against iterate(10), a captured graph against CGAMD_NO_GRAPH, a second run, iterate_until with
check_every 1 against 8.  Tolerances (float32 1e-4 |b_j|, float64 1e-8 |b_j|): all columns stop in the first iteration in which
each satisfies its own, read off the handle's own history; the count is block_ref's, +-1; solve_block leaves a true residual (float64
on the host) of at most 2 tol |b_j| and, at s >= 4, needs strictly fewer iterations than the slowest column of the same handle's
solve_until.  A duplicated column breaks down in set_rhs (status 2 at iteration 0, X untouched and finite) and solve_block finishes
column by column.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import block_ref as B
import shift_ref as R

pytestmark = pytest.mark.gpu

GRIDS = {"33x29": (33, 29), "64x64": (64, 64)}
BLOCKS = (2, 4, 9, 16)
DTYPES = (np.float32, np.float64)
TOL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-8}
ITERS = 10
CASES = [(g, s, d) for g in GRIDS for s in BLOCKS for d in DTYPES]
IDS = [f"{g}-s{s}-{np.dtype(d).name}" for g, s, d in CASES]

_SYS, _REF = {}, {}


def system(name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _SYS:
        A = sp.csr_matrix(R.laplace2d(*GRIDS[name]).astype(dtype).astype(np.float64))
        A.sort_indices()
        _SYS[key] = A
    return _SYS[key]


def rhs(name, s, dtype):
    """(n, s), as rounded to dtype"""
    n = GRIDS[name][0] * GRIDS[name][1]
    return np.random.default_rng(11).standard_normal((n, s)).astype(dtype)


def ref(name, s, dtype, wide=False, tol=None, x0=None):
    """block_ref.bcg once per case: ITERS iterations (tol None) or to the tolerance; wide: the same right-hand sides in float64"""
    key = (name, s, np.dtype(dtype).name, wide, tol, None if x0 is None else x0.tobytes())
    if key not in _REF:
        b = rhs(name, s, dtype)
        run_in = np.float64 if wide else dtype
        nb = np.linalg.norm(b.astype(np.float64), axis=0)
        _REF[key] = B.bcg(system(name, dtype), b.astype(run_in), tol=None if tol is None else tol * nb, maxit=ITERS if tol is None else 400,
                          dtype=run_in, X0=x0)
    return _REF[key]


def make(pkg, ctx, name, dtype, s, flags=0, **kw):
    A = system(name, dtype)
    return pkg.Solver(ctx, A.shape[0], A.nnz, A.data.astype(dtype), A.indptr, A.indices, s, flags=flags, **kw)


def dev(b):
    """(n, s) -> the handle's RHS-major block"""
    return np.ascontiguousarray(b.T).reshape(-1)


def run(s, b, pieces=(ITERS,), x0=None):
    s.set_rhs(dev(b), None if x0 is None else dev(x0))
    for k in pieces:
        s.iterate(k)
    return s.x().reshape(s.n_rhs, -1).T.copy(), s.history()


def same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int(np.count_nonzero(a != b))} values differ"


def true_residual(name, dtype, b, x):
    """|b_j - A x_j| / |b_j| in float64 on the host"""
    A = system(name, dtype)
    b64, x64 = b.astype(np.float64), x.astype(np.float64)
    return np.linalg.norm(b64 - A @ x64, axis=0) / np.linalg.norm(b64, axis=0)


def yardstick(name, s, dtype):
    narrow, wide = ref(name, s, dtype), ref(name, s, dtype, wide=True)
    h, hw = narrow["history"].astype(np.float64), wide["history"]
    Dk = np.max(np.abs(h - hw) / hw, axis=1)
    DX = np.max(np.linalg.norm(narrow["X"].astype(np.float64) - wide["X"], axis=0) / np.linalg.norm(wide["X"], axis=0))
    return Dk, DX, wide


@pytest.mark.parametrize("name,s,dtype", CASES, ids=IDS)
def test_ten_iterations_against_the_restatement_and_the_bits(pkg, gpu, name, s, dtype):
    ctx, L = gpu[0], pkg._lib
    dtype = np.dtype(dtype)
    b = rhs(name, s, dtype)
    sv = make(pkg, ctx, name, dtype, s)
    ng = make(pkg, ctx, name, dtype, s, flags=L.NO_GRAPH)
    try:
        sv.set_block(True)
        ng.set_block(True)
        assert L.load().cgamd_solver_loop_launches(sv.handle) == 6
        x, h = run(sv, b)
        assert h.shape == (ITERS + 1, s) and sv.iterations_done() == ITERS
        Dk, DX, wide = yardstick(name, s, dtype)
        eh = np.max(np.abs(h.astype(np.float64) - wide["history"]) / wide["history"], axis=1)
        ex = np.max(np.linalg.norm(x.astype(np.float64) - wide["X"], axis=0) / np.linalg.norm(wide["X"], axis=0))
        print(name, s, dtype.name, "D_k", Dk.min(), "..", Dk.max(), "D_X", DX, "| GPU history", eh.max(), "worst ratio", np.max(eh / Dk) if dtype.itemsize == 4 else "-",
              "x", ex)
        if dtype.itemsize == 4:
            assert np.all(eh <= 4 * Dk), (eh, Dk)
            assert ex <= 4 * DX
        else:
            assert eh.max() < 1e-10 and ex < 1e-9
        st = sv.block_status()
        assert (st["on"], st["status"], st["s"]) == (True, 0, s) and st["min_pivot_ratio"] > 0.1
        x2, h2 = run(sv, b)
        same(x2, x, "a second run: x"); same(h2, h, "a second run: history")
        x3, h3 = run(sv, b, pieces=(3, 7))
        same(x3, x, "iterate(3); iterate(7): x"); same(h3, h, "iterate(3); iterate(7): history")
        x4, h4 = run(ng, b)
        same(x4, x, "CGAMD_NO_GRAPH: x"); same(h4, h, "CGAMD_NO_GRAPH: history")
    finally:
        sv.close()
        ng.close()


@pytest.mark.parametrize("name,s,dtype", CASES, ids=IDS)
def test_tolerance_stop_and_solve_block(pkg, gpu, name, s, dtype):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    tol = TOL[dtype]
    b = rhs(name, s, dtype)
    nb = np.linalg.norm(b.astype(np.float64), axis=0)
    sv = make(pkg, ctx, name, dtype, s)
    try:
        sv.set_block(True)
        got = {}
        for ce in (1, 8):
            sv.set_rhs(dev(b))
            its = sv.iterate_until(tol * nb, 400, ce)
            got[ce] = (its.copy(), sv.x().copy(), sv.history())
        its, x, h = got[8]
        assert np.array_equal(got[1][0], its)
        same(got[1][1], x, "check_every 1 against 8: x"); same(got[1][2], h, "check_every 1 against 8: history")
        assert np.all(its == its[0]) and sv.iterations_done() == its[0] and h.shape[0] == its[0] + 1
        # the all-at-once rule, read off the handle's own history
        below = ~(np.sqrt(np.abs(h.astype(np.float64))) >= tol * nb)
        first = int(np.nonzero(np.all(below[1:], axis=1))[0][0]) + 1
        want = ref(name, s, dtype, tol=tol)["iterations"]
        print(name, s, dtype.name, "iterations", int(its[0]), "block_ref", want)
        assert its[0] == first
        assert abs(int(its[0]) - want) <= 1
        with pytest.raises(pkg._lib.CgAmdError):        # the columns have stopped: iterate() asks for set_rhs
            sv.iterate(1)
        # a tolerance per column: the loosest column does not stop the tightest
        tols = tol * nb * np.where(np.arange(s) % 2 == 0, 100.0, 1.0)
        sv.set_rhs(dev(b))
        its2 = sv.iterate_until(tols, 400, 8)
        h2 = sv.history()
        below2 = ~(np.sqrt(np.abs(h2.astype(np.float64))) >= tols)
        assert np.all(its2 == its2[0]) and its2[0] == int(np.nonzero(np.all(below2[1:], axis=1))[0][0]) + 1
        assert np.any(np.all(below2[1:, 0::2], axis=1)[:its2[0] - 1]), "the loose columns alone would have stopped earlier"
        same(h2, h[:its2[0] + 1], "the history up to the earlier stop")
        # solve_block, and the same handle's column-by-column solve
        xb, info = sv.solve_block(dev(b), tol=tol, maxit=400)
        res = true_residual(name, dtype, b, xb.reshape(s, -1).T)
        sv.set_block(False)
        _, its_single, _ = sv.solve_until(dev(b), tol=tol * nb, maxit=400)
        print(name, s, dtype.name, "solve_block", info, "residual / tol", float(np.max(res / tol)), "solve_until", its_single.tolist())
        assert info["path"] == "block" and info["status"] == 0 and info["block_iterations"] == its[0]
        same(xb, x, "solve_block against set_rhs; iterate_until")
        assert np.all(res <= 2 * tol)
        if s >= 4:
            assert info["block_iterations"] < int(its_single.max())
    finally:
        sv.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_duplicate_column_breaks_down_and_solve_block_falls_back(pkg, gpu, dtype):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    tol = TOL[dtype]
    b = rhs("33x29", 4, dtype)
    b[:, 3] = b[:, 1]
    sv = make(pkg, ctx, "33x29", dtype, 4)
    try:
        sv.set_block(True)
        x, h = run(sv, b, pieces=(5,))
        st = sv.block_status()
        print(dtype.name, st)
        assert (st["status"], st["iteration"]) == (2, 0) and st["min_pivot_ratio"] <= 4 * B.EPS[dtype]
        assert not np.any(x) and sv.iterations_done() == 0       # frozen in set_rhs: X is x0, finite
        np.testing.assert_allclose(sv.history()[0].astype(np.float64), np.sum(b.astype(np.float64) ** 2, axis=0), rtol=1e-6)
        sv.set_rhs(dev(b))
        its = sv.iterate_until(tol, 50, 8)                      # ends with the count reached, whatever maxit
        assert np.all(its == 0)
        xb, info = sv.solve_block(dev(b), tol=tol, maxit=400)
        res = true_residual("33x29", dtype, b, xb.reshape(4, -1).T)
        print(dtype.name, info, "residual / tol", float(np.max(res / tol)))
        assert info["path"] == "block+columns" and info["status"] == 2 and info["breakdown_iteration"] == 0
        assert info["block_iterations"] == 0 and np.all(info["column_iterations"] > 0)
        assert np.all(np.isfinite(xb)) and np.all(res <= 2 * tol)
        assert sv.block_status()["on"]                          # block CG stays on: an independent block runs it again
        b2 = rhs("33x29", 4, dtype)
        xb2, info2 = sv.solve_block(dev(b2), tol=tol, maxit=400)
        assert info2["path"] == "block" and np.all(true_residual("33x29", dtype, b2, xb2.reshape(4, -1).T) <= 2 * tol)
    finally:
        sv.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_nonzero_x0(pkg, gpu, dtype):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    s = 4
    b = rhs("33x29", s, dtype)
    x0 = np.random.default_rng(5).standard_normal(b.shape).astype(dtype)
    sv = make(pkg, ctx, "33x29", dtype, s)
    try:
        sv.set_block(True)
        x, h = run(sv, b, x0=x0)
        narrow, wide = ref("33x29", s, dtype, x0=x0), ref("33x29", s, dtype, wide=True, x0=x0)
        hw = wide["history"]
        Dk = np.max(np.abs(narrow["history"].astype(np.float64) - hw) / hw, axis=1)
        eh = np.max(np.abs(h.astype(np.float64) - hw) / hw, axis=1)
        ex = np.max(np.linalg.norm(x.astype(np.float64) - wide["X"], axis=0) / np.linalg.norm(wide["X"], axis=0))
        print(dtype.name, "x0: D_k", Dk, "GPU", eh, "x", ex)
        if dtype.itemsize == 4:
            assert np.all(eh <= 4 * Dk)
        else:
            assert eh.max() < 1e-10 and ex < 1e-9
        xb, info = sv.solve_block(dev(b), x0=dev(x0), tol=TOL[dtype], maxit=400)
        assert info["path"] == "block" and np.all(true_residual("33x29", dtype, b, xb.reshape(s, -1).T) <= 2 * TOL[dtype])
    finally:
        sv.close()


def _plain(s, b, tol, until=True):
    """a plain solve of the handle: 12 iterations, then the per-column stop (until=False: a handle that has none)"""
    s.set_rhs(dev(b))
    s.iterate(12)
    out = [s.x().copy(), s.history()]
    if not until:
        return out
    s.set_rhs(dev(b))
    out += [s.iterate_until(tol, 400, 8).copy(), s.x().copy(), s.history()]
    return out


def _unchanged(a, b, what):
    for u, v in zip(a, b):
        same(np.asarray(u), np.asarray(v), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_turned_off_the_handle_has_the_bits_of_one_that_never_had_it(pkg, gpu, dtype):
    ctx, lib = gpu[0], pkg._lib.load()
    dtype = np.dtype(dtype)
    b = rhs("33x29", 4, dtype)
    tol = TOL[dtype] * np.linalg.norm(b.astype(np.float64), axis=0)
    never, sv = make(pkg, ctx, "33x29", dtype, 4), make(pkg, ctx, "33x29", dtype, 4)
    try:
        want = _plain(never, b, tol)
        sv.set_block(True)
        run(sv, b)
        sv.solve_block(dev(b), tol=TOL[dtype])
        sv.set_block(False)
        assert not sv.block_status()["on"]
        with pytest.raises(pkg._lib.CgAmdError):        # r and d held Q and P: set_rhs comes first
            sv.iterate(1)
        _unchanged(_plain(sv, b, tol), want, "after set_block(False)")
        assert lib.cgamd_solver_loop_launches(sv.handle) == lib.cgamd_solver_loop_launches(never.handle)
        assert sv.iter_moved_bytes == never.iter_moved_bytes and sv.iter_bytes() == never.iter_bytes()
        sv.set_block(True)                              # the byte models of the block loop: 14 passes beside the matrix, the plain loop 10
        V = dtype.itemsize
        assert sv.iter_moved_bytes - never.iter_moved_bytes == 4 * 957 * V * 4
    finally:
        never.close()
        sv.close()


def test_set_block_refuses_what_it_does_not_serve(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    A = system("33x29", np.float64)
    b = rhs("33x29", 4, np.float64)

    def refused(s, block, reason, until=True):
        tol = 1e-4 * np.linalg.norm(np.abs(block).astype(np.float64), axis=0)
        before = _plain(s, block, tol, until)
        assert lib.cgamd_solver_set_block(s.handle, 1) == L.ERR_STATE, reason
        assert reason.encode() in lib.cgamd_last_error(), (reason, lib.cgamd_last_error())
        assert not s.block_status()["on"]
        _unchanged(_plain(s, block, tol, until), before, reason)
        s.close()

    Ac = R.shifted_laplace2d(33, 29, 0.3 + 0.2j)
    for ct in (np.complex64, np.complex128):
        bc = (b + 0.5j * b[::-1]).astype(ct)
        refused(pkg.Solver(ctx, 957, Ac.nnz, Ac.data.astype(ct), Ac.indptr, Ac.indices, 4), bc, "real value types")
    refused(pkg.Solver(ctx, 957, A.nnz, np.tile(A.data, 4), A.indptr, A.indices, 4, batched=True), b, "batched")
    refused(make(pkg, ctx, "33x29", np.float64, 4, flags=L.UNFUSED), b, "CGAMD_UNFUSED", until=False)
    L.check(lib.cgamd_tune(b"spmm_rowmajor", 2))             # fp64 x 16 keeps its right-hand sides interleaved under this knob
    try:
        rm = make(pkg, ctx, "33x29", np.float64, 16)
    finally:
        L.check(lib.cgamd_tune(b"spmm_rowmajor", 1))
    refused(rm, rhs("33x29", 16, np.float64), "row-major", until=False)
    refused(make(pkg, ctx, "33x29", np.float64, 1), b[:, :1], "2 ... 16")
    refused(make(pkg, ctx, "33x29", np.float32, 17), rhs("33x29", 17, np.float32), "2 ... 16")
    pre = make(pkg, ctx, "33x29", np.float64, 4)
    pre.set_preconditioner("jacobi")
    refused(pre, b, "preconditioner")
    sh = make(pkg, ctx, "33x29", np.float64, 4)
    sh.set_shifts([0.5])
    refused(sh, b, "shifts")


def test_what_is_refused_with_block_on(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    dtype = np.dtype(np.float64)
    b = rhs("33x29", 4, dtype)
    sv = make(pkg, ctx, "33x29", dtype, 4)
    try:
        sv.set_block(True)
        sv.enable_projection(2)
        x, hist = run(sv, b)
        h, p, one = sv.handle, L.ptr, np.ones(957)
        its = ctypes.c_int()
        calls = {
            "set_preconditioner": lambda: lib.cgamd_solver_set_preconditioner(h, p(one), 0),
            "set_preconditioner_tridiag": lambda: lib.cgamd_solver_set_preconditioner_tridiag(h, p(one), p(4 * one), p(one), 0),
            "set_preconditioner_tridiag_strided": lambda: lib.cgamd_solver_set_preconditioner_tridiag_strided(h, 33, p(one), p(4 * one), p(one), 0),
            "set_preconditioner_line": lambda: lib.cgamd_solver_set_preconditioner_line(h, 1),
            "set_preconditioner_jacobi": lambda: lib.cgamd_solver_set_preconditioner_jacobi(h),
            "set_preconditioner_multigrid": lambda: lib.cgamd_solver_set_preconditioner_multigrid(h, 33, 29, 1, 0, 0.0, 0),
            "set_preconditioner_amg": lambda: lib.cgamd_solver_set_preconditioner_amg(h, 0, 0.0, 0, 0.0, 0),
            "set_shifts": lambda: lib.cgamd_solver_set_shifts(h, p(np.ones(1)), 1),
            "iterate_tol": lambda: lib.cgamd_solver_iterate_tol(h, 5, 1e-3, ctypes.byref(its)),
            "replace_residual": lambda: lib.cgamd_solver_replace_residual(h, sv.vector("q")),
        }
        for who, call in calls.items():
            assert call() == L.ERR_STATE, who
            assert b"block CG is on" in lib.cgamd_last_error(), (who, lib.cgamd_last_error())
            same(sv.x().reshape(4, -1).T, x, who + ": x"); same(sv.history(), hist, who + ": history")
            assert sv.block_status()["on"] and sv.iterations_done() == ITERS
        sv.iterate(2)                                   # and it goes on
        # removal of a preconditioner that is not there stays served, and the projected start only chooses x0
        L.check(lib.cgamd_solver_set_preconditioner(h, None, 0))
        tol = 1e-8 * np.linalg.norm(b, axis=0)
        for _ in range(2):
            sv.set_rhs_projected(dev(b))
            its_p = sv.iterate_until(tol, 400, 8)
            xp = sv.x().reshape(4, -1).T
            sv.projection_update()
            assert sv.block_status()["status"] == 0 and np.all(true_residual("33x29", dtype, b, xp) <= 2e-8)
        print("projected restart of the same right-hand sides: iterations", its_p.tolist())
    finally:
        sv.close()


def test_mixed_solve_refuses_a_handle_with_block_on(pkg, gpu):
    ctx, L = gpu[0], pkg._lib
    A = system("33x29", np.float64)
    b = rhs("33x29", 4, np.float64)
    m = pkg.MixedSolver(ctx, A.shape[0], A.nnz, A.data, A.indptr, A.indices, 4)
    try:
        x0, info0 = m.solve(dev(b), tol=1e-9)
        for h in (m.inner, m.outer):
            h.set_block(True)
            with pytest.raises(L.CgAmdError) as e:
                m.solve(dev(b), tol=1e-9)
            assert e.value.status == L.ERR_STATE and "block CG is on" in str(e.value)
            h.set_block(False)
        x1, info1 = m.solve(dev(b), tol=1e-9)
        same(x1, x0, "the mixed solve after set_block(False) on both handles")
        assert np.array_equal(info1.iterations, info0.iterations)
    finally:
        m.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_refresh_values_keeps_block_cg(pkg, gpu, dtype):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    s, tol = 4, TOL[np.dtype(dtype)]
    A = system("33x29", dtype)
    b = rhs("33x29", s, dtype)
    sv = make(pkg, ctx, "33x29", dtype, s)
    fresh = pkg.Solver(ctx, A.shape[0], A.nnz, (1.5 * A.data).astype(dtype), A.indptr, A.indices, s)
    try:
        sv.set_block(True)
        run(sv, b)
        sv.refresh_values((1.5 * A.data).astype(dtype))
        assert sv.block_status()["on"]
        x, info = sv.solve_block(dev(b), tol=tol, maxit=400)
        res = np.linalg.norm(b.astype(np.float64) - 1.5 * (A @ x.reshape(s, -1).T.astype(np.float64)), axis=0) / np.linalg.norm(b.astype(np.float64), axis=0)
        assert info["path"] == "block" and np.all(res <= 2 * tol)
        fresh.set_block(True)
        xf, info_f = fresh.solve_block(dev(b), tol=tol, maxit=400)
        same(x, xf, "refreshed against a handle created with the new values")
        assert info_f["block_iterations"] == info["block_iterations"]
    finally:
        sv.close()
        fresh.close()
