"""The line-preconditioner sweeps z = M^-1 r as an operation of their own, element by element: the fused scan sweep
(pcg_tri_kernel MODE 0), its three-launch long form (MODE 1, pcg_tri_carry_kernel, MODE 2) and the one-thread-per-line strided
walk (pcg_tri_strided_kernel), every value type.  After set_rhs the handle holds r = b in "r" and z0 = M^-1 b in "d" (UPD =
false); after iterate(k) it holds r_k in "r" and z_k = M^-1 r_k in "q" (UPD = true, in place).  Both are read back and compared
per segment with the extended-precision solve of the very inputs the device was given (tridiag_pcg.thomas_ext / check_sweep:
e(z) <= 4 max(e(sequential sweep in the type), 4 eps)).  Chains keep a relative diagonal shift of at least 1e-2 over
|lower| + |upper|; the one shift-0 case is measured and printed, not asserted."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cg_numpy
import tridiag_pcg as tp

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


def rows_per_thread(dtype):
    return 32 // np.dtype(dtype).itemsize                 # R: 8 / 4 / 4 / 2


def chunk_rows(dtype):
    return 256 * rows_per_thread(dtype)                   # C: 2048 / 1024 / 1024 / 512


def walk_rows(dtype):
    return 4 if np.dtype(dtype).itemsize == 16 else 8     # U of the strided walk


def tols(dtype):
    return (1e-9, 1e-10) if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else (1e-4, 1e-4)


def chain(rng, n, dtype, stride=1, shift=0.1, extra=0.0):
    """M's three arrays rounded to the value type: couplings -U(0.2, 1) (symmetric), diagonal (1 + shift)(|lower| + |upper|)
    + extra; complex types: every entry with a phase of its own in +-0.3 (complex symmetric, damped)"""
    cplx = np.dtype(dtype).kind == "c"
    off = -rng.uniform(0.2, 1.0, n - stride)
    if cplx:
        off = off * np.exp(1j * rng.uniform(-0.3, 0.3, n - stride))
    lower, upper = np.zeros(n, off.dtype), np.zeros(n, off.dtype)
    lower[stride:], upper[:n - stride] = off, off
    diag = (1.0 + shift) * (np.abs(lower) + np.abs(upper)) + extra
    if cplx:
        diag = diag * np.exp(1j * rng.uniform(-0.3, 0.3, n))
    return lower.astype(dtype), diag.astype(dtype), upper.astype(dtype)


def cut(lower, upper, rows, stride=1):
    rows = np.asarray(rows, dtype=np.int64)
    lower[rows] = 0
    upper[rows - stride] = 0


def rhs(rng, nrhs, n, dtype):
    b = rng.standard_normal((nrhs, n))
    if np.dtype(dtype).kind == "c":
        b = b + 1j * rng.standard_normal((nrhs, n))
    return b.astype(dtype)


def matrix(lower, diag, upper, stride, far=None):
    """A: M itself, plus (far = (distance, value)) a symmetric coupling that M leaves out"""
    n = diag.size
    d, o = [lower[stride:], diag, upper[:n - stride]], [-stride, 0, stride]
    if far is not None:
        d += [np.full(n - far[0], far[1], diag.dtype)] * 2
        o += [-far[0], far[0]]
    A = sp.csr_matrix(sp.diags(d, o, format="csr", dtype=diag.dtype))
    A.sort_indices()
    return A


def read(pkg, ctx, s, which):
    """one of the handle's vectors as (n_rhs, ld)"""
    ctx.synchronize()
    out = np.empty(s.n_rhs * s.ld, dtype=s.dtype)
    pkg._lib.check(pkg._lib.load().cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), ctypes.c_void_p(s.vector(which)), out.nbytes))
    return out.reshape(s.n_rhs, s.ld)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run_case(pkg, gpu, label, lower, diag, upper, dtype, nrhs, launches, stride=1, far=None, A=None, B=None, iterate=0,
             assert_sweep=True):
    """set_rhs on a handle with M = (lower, diag, upper) at `stride`, then: the launch count, "r" = b bit for bit, z0 in "d" and
    not in "q", zero padding rows of z0, history[0] against the extended b.b, z0 through check_sweep.  iterate > 0: that many
    iterations, then "q" against the exact solve of the device's own "r", and "r" against the restated PCG element by element.
    Returns (z0, z_ref, the bound check_sweep held z0 to)."""
    ctx, _, _ = gpu
    lib = pkg._lib.load()
    dtype = np.dtype(dtype)
    n = diag.size
    if A is None:
        A = matrix(lower, diag, upper, stride, far)
    if B is None:
        B = rhs(np.random.default_rng(1), nrhs, n, dtype)
    s = pkg.Solver(ctx, n, A.nnz, A.data.astype(dtype), A.indptr.astype(np.int32), A.indices.astype(np.int32), nrhs)
    try:
        pkg._lib.check(lib.cgamd_solver_set_preconditioner_tridiag_strided(s.handle, stride, pkg._lib.ptr(lower), pkg._lib.ptr(diag),
                                                                           pkg._lib.ptr(upper), 0))
        assert lib.cgamd_solver_loop_launches(s.handle) == launches, (label, lib.cgamd_solver_loop_launches(s.handle))
        s.set_rhs(B.reshape(-1))
        ld = s.ld
        assert ld >= n and s.vector("d") != s.vector("q")
        r0, z0, q0 = read(pkg, ctx, s, "r"), read(pkg, ctx, s, "d"), read(pkg, ctx, s, "q")
        assert same_bits(r0[:, :n], B), label                              # UPD = false leaves r = b alone
        assert not np.any(q0[:, :n]), label                                # z0 went to d's storage; q still holds A x0 = 0
        if ld != n:
            assert not np.any(z0[:, n:]), (label, "padding rows of z")
        ext = np.clongdouble if dtype.kind == "c" else np.longdouble
        bb = np.sum(B.astype(ext) ** 2, axis=1)
        h0 = s.history()[0]
        herr = np.max(np.abs(h0 - bb) / np.abs(bb))
        print(f"  {label} {dtype.name}: n {n}, ld {ld}, launches {launches}, history[0] err {float(herr):.3e} (< {tols(dtype)[1]:g})")
        assert herr < tols(dtype)[1], (label, herr)
        segs = tp.segments(lower, diag, upper, dtype, stride)
        z_ref = tp.thomas_ext(lower, diag, upper, B, stride)
        z_seq = tp.sweep_in_type(lower, diag, upper, B, dtype, stride)
        bound = None
        if assert_sweep:
            figures = tp.check_sweep(z0[:, :n], z_ref, z_seq, segs, dtype, label + " set_rhs")
            bound = max(4.0 * max(e_seq, 4.0 * float(np.finfo(dtype).eps)) for _, e_seq in figures)
        else:
            for r in range(nrhs):
                e_dev, e_seq = tp.sweep_error(z0[r, :n], z_ref[r], segs), tp.sweep_error(z_seq[r], z_ref[r], segs)
                print(f"  sweep {label} (measured, not asserted) {dtype.name} rhs {r}: e(z) {e_dev:.3e}, e(z_seq) {e_seq:.3e}, "
                      f"ratio {e_dev / e_seq:.2f}")
                assert np.isfinite(e_dev)
        if iterate:
            s.iterate(iterate)
            rk, zk = read(pkg, ctx, s, "r")[:, :n], read(pkg, ctx, s, "q")[:, :n]
            tp.check_sweep(zk, tp.thomas_ext(lower, diag, upper, rk, stride), tp.sweep_in_type(lower, diag, upper, rk, dtype, stride),
                           segs, dtype, f"{label} iterate({iterate})")
            M = matrix(lower, diag, upper, stride)
            lu = spla.splu(sp.csc_matrix(M.astype(complex)))
            for r in range(nrhs):
                _, _, _, want = tp.pcg_sparse(A.astype(complex), B[r].astype(complex), M, tol=0.0, maxit=iterate, history=True,
                                              solve=lu.solve, residual=True)
                rerr = np.max(np.abs(rk[r] - want)) / np.max(np.abs(want))
                print(f"  {label} {dtype.name} rhs {r}: r_{iterate} element-wise err {rerr:.3e} (< {tols(dtype)[0]:g}), "
                      f"max|r_{iterate}| / max|b| {np.max(np.abs(want)) / np.max(np.abs(B[r])):.2e}")
                assert rerr < tols(dtype)[0], (label, r, rerr)
        return z0[:, :n], z_ref, bound
    finally:
        s.close()


# ---- stride 1, fused form ------------------------------------------------------------------------------------------------------

def mixed_segments(rng, dtype, total):
    """segment lengths drawn from {1, 2, R-1, R, R+1, 64R-1, 64R, 64R+1, C-R} in random order, every one at least once, `total`
    rows or a little more, an odd row count"""
    R, C = rows_per_thread(dtype), chunk_rows(dtype)
    pool = [1, 2, R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, C - R]
    lengths = list(rng.permutation(pool))
    while sum(lengths) < total:
        lengths.append(int(rng.choice(pool)))
    lengths = [int(v) for v in rng.permutation(lengths)]
    if sum(lengths) % 2 == 0:
        lengths.append(1)
    return lengths


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_mixed_segment_lengths(pkg, gpu, dtype):
    """about 40 C rows of segments of 1 row to C - R rows, so chunks begin off multiples of R and threads straddle chunk starts;
    odd size (padding rows except in complex128), 3 right-hand sides"""
    rng = np.random.default_rng(21)
    lengths = mixed_segments(rng, dtype, 40 * chunk_rows(dtype))
    n = sum(lengths)
    assert n % 2 == 1
    lower, diag, upper = chain(rng, n, dtype)
    cut(lower, upper, np.cumsum(lengths)[:-1])
    assert tp.segments(lower, diag, upper, dtype)[:, 1].tolist() == lengths
    run_case(pkg, gpu, "fused mixed", lower, diag, upper, dtype, 3, 4)


def exact_chunk_segment(dtype, lead):
    """segments of `lead`, C and 5 R + 1 rows (every part a chain of its own: no coupling across its ends); the C-row segment has
    the same entries and the same right-hand side whatever `lead` is"""
    R, C = rows_per_thread(dtype), chunk_rows(dtype)
    rng = np.random.default_rng(31)
    parts = [chain(rng, m, dtype) + (rhs(rng, 1, m, dtype),) for m in (C, lead, 5 * R + 1)]
    lower, diag, upper, B = (np.concatenate([parts[1][k], parts[0][k], parts[2][k]], axis=-1) for k in range(4))
    return lower, diag, upper, B


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_of_exactly_one_chunk_fused_and_long_form(pkg, gpu, dtype):
    """a segment of exactly C rows is fused when it begins on a multiple of R and takes the long form when it begins one row
    later (tri_plan); the same segment gives the same answer through both"""
    R, C = rows_per_thread(dtype), chunk_rows(dtype)
    out = []
    for lead, launches in ((3 * R, 4), (3 * R + 1, 6)):
        lower, diag, upper, B = exact_chunk_segment(dtype, lead)
        assert tp.segments(lower, diag, upper, dtype).tolist() == [[0, lead, 1], [lead, C, 1], [lead + C, 5 * R + 1, 1]]
        z, z_ref, bound = run_case(pkg, gpu, f"{'fused' if launches == 4 else 'long'} exactly C rows from row {lead}", lower, diag, upper, dtype, 1,
                                      launches, B=B)
        out.append((z[0, lead:lead + C], z_ref[0, lead:lead + C], bound))
    # the segment's exact solve is the same in both; each form is within its bound of it, so they are within the sum of each other
    (za, ra, ba), (zb, rb, bb) = out
    assert np.array_equal(ra, rb)
    diff = float(np.max(np.abs(za.astype(ra.dtype) - zb)) / np.max(np.abs(ra)))
    print(f"  {np.dtype(dtype).name}: fused against long form on the C-row segment {diff:.3e} (<= {ba + bb:.3e})")
    assert diff <= ba + bb


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_one_sided_zeros_do_not_cut(pkg, gpu, dtype):
    """an unsymmetric M with lower[i] = 0 but upper[i - 1] != 0 at 60 random rows and the reverse at 60 others: no cut there (the
    segment rule needs both), and z is still the exact solve; two-sided cuts every R to C - R rows keep the form fused"""
    R, C = rows_per_thread(dtype), chunk_rows(dtype)
    rng = np.random.default_rng(41)
    lengths = [int(v) for v in rng.integers(R, C - R + 1, size=14)]
    if sum(lengths) % 2 == 0:
        lengths[-1] -= 1
    n = sum(lengths)
    lower, diag, upper = chain(rng, n, dtype)
    starts = np.cumsum(lengths)[:-1]
    cut(lower, upper, starts)
    free = np.setdiff1d(np.arange(1, n), starts)
    rows = rng.choice(free, size=120, replace=False)
    lower[rows[:60]] = 0
    upper[rows[60:] - 1] = 0
    assert np.all(upper[rows[:60] - 1] != 0) and np.all(lower[rows[60:]] != 0)
    assert tp.segments(lower, diag, upper, dtype)[:, 0].tolist() == [0] + starts.tolist()
    run_case(pkg, gpu, "fused one-sided zeros", lower, diag, upper, dtype, 3, 4)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_fused_helmholtz_htrid(pkg, gpu, dtype):
    """the reference driver's own use: Htrid (the entries with |i - j| < 10) of helmFE_var(200, 12, C = 1, rho = 0.15), 200 grid
    lines, indefinite and damped; A is the Helmholtz matrix itself"""
    N = 200
    ip, ix, da = cg_numpy.helm_fe_var(N, 12.0, np.ones((N - 1, N - 1)), 0.15, N, N)
    A = sp.csr_matrix((da.astype(dtype), ix, ip), shape=(N * N, N * N))
    M = tp.band(A, 10)
    n = N * N
    lower, diag, upper = np.zeros(n, dtype), M.diagonal(0).astype(dtype), np.zeros(n, dtype)
    lower[1:], upper[:-1] = M.diagonal(-1), M.diagonal(1)
    segs = tp.segments(lower, diag, upper, dtype)
    assert len(segs) == N and np.all(segs[:, 1] == N)
    run_case(pkg, gpu, "fused Htrid", lower, diag, upper, dtype, 2, 4, A=A)


# ---- stride 1, long form -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("size", ["C+1", "2C", "2C+1", "200001"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_long_form_one_chain(pkg, gpu, dtype, size, nrhs):
    """one chain of C + 1, 2 C, 2 C + 1 and 200 001 rows (the odd sizes: padding rows), every instantiation, distinct right-hand
    sides through the per-RHS chunk maps; shift 1e-2 on the long chain"""
    C = chunk_rows(dtype)
    n = {"C+1": C + 1, "2C": 2 * C, "2C+1": 2 * C + 1, "200001": 200_001}[size]
    lower, diag, upper = chain(np.random.default_rng(51), n, dtype, shift=1e-2 if n > 3 * C else 0.1)
    run_case(pkg, gpu, f"long {size}", lower, diag, upper, dtype, nrhs, 6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_form_random_cuts(pkg, gpu, dtype):
    """60 C + 1 rows with 100 random cuts: segments of a few rows to several chunks, chunk edges anywhere inside them"""
    C = chunk_rows(dtype)
    rng = np.random.default_rng(61)
    n = 60 * C + 1
    lower, diag, upper = chain(rng, n, dtype)
    cut(lower, upper, rng.choice(np.arange(1, n), size=100, replace=False))
    segs = tp.segments(lower, diag, upper, dtype)
    assert len(segs) == 101 and segs[:, 1].max() > C
    run_case(pkg, gpu, "long random cuts", lower, diag, upper, dtype, 1, 6)


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_long_form_more_chunks_than_work_groups(pkg, gpu, dtype):
    """one chain of 1025 C + 3 rows: 1026 chunks on the 1024-work-group grid, so two work-groups take a second chunk (LDS reused
    across chunks in MODE 1) and the carry walk is 1026 maps long"""
    n = 1025 * chunk_rows(dtype) + 3
    lower, diag, upper = chain(np.random.default_rng(71), n, dtype)
    run_case(pkg, gpu, "long 1025 C + 3", lower, diag, upper, dtype, 1, 6)


# ---- strided -------------------------------------------------------------------------------------------------------------------

def grid_lines(rng, nx, ny, nz, axis, dtype, extra=0.0):
    """line preconditioner of an nx x ny x nz grid (x fastest) along y (stride nx) or z (stride nx ny)"""
    n = nx * ny * nz
    stride = nx if axis == "y" else nx * ny
    lower, diag, upper = chain(rng, n, dtype, stride, extra=extra)
    if axis == "y":                                                       # a y-line ends where its plane does
        i = np.arange(stride, n)
        cut(lower, upper, i[(i // nx) % ny == 0], stride)
    return lower, diag, upper, stride


@pytest.mark.parametrize("axis", ["y", "z"])
@pytest.mark.parametrize("nz", ["U-1", "U", "U+1", "2U", "2U+1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_grid_lines_around_the_step(pkg, gpu, dtype, nz, axis):
    """13 x 11 x nz grids, z-lines (stride 143) of U - 1 to 2 U + 1 rows, U the rows per step of the walk, and y-lines (stride 13,
    11 rows, nz planes of them); 3 right-hand sides"""
    U = walk_rows(dtype)
    nz = {"U-1": U - 1, "U": U, "U+1": U + 1, "2U": 2 * U, "2U+1": 2 * U + 1}[nz]
    lower, diag, upper, stride = grid_lines(np.random.default_rng(81), 13, 11, nz, axis, dtype)
    segs = tp.segments(lower, diag, upper, dtype, stride)
    assert len(segs) == (143 if axis == "z" else 13 * nz) and np.all(segs[:, 1] == (nz if axis == "z" else 11))
    run_case(pkg, gpu, f"strided 13x11x{nz} {axis}-lines", lower, diag, upper, dtype, 3, 4, stride=stride)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_unequal_chains_random_cuts(pkg, gpu, dtype):
    """20 011 rows at stride 37 (size % stride = 31: chains of 541 and 540 rows) with 2000 random cuts: segments of one row to
    dozens, every length around U, lanes of a wave with different lengths; 3 right-hand sides"""
    rng = np.random.default_rng(91)
    n, stride = 20_011, 37
    lower, diag, upper = chain(rng, n, dtype, stride)
    cut(lower, upper, rng.choice(np.arange(stride, n), size=2000, replace=False), stride)
    segs = tp.segments(lower, diag, upper, dtype, stride)
    U = walk_rows(dtype)
    assert len(segs) == stride + 2000 and set(range(1, 2 * U + 2)) <= set(segs[:, 1].tolist())
    run_case(pkg, gpu, "strided unequal chains", lower, diag, upper, dtype, 3, 4, stride=stride)


def test_strided_more_segments_than_threads(pkg, gpu):
    """600 x 500 x 3 z-lines in fp64: 300 000 segments on a grid of 1024 work-groups of 256 threads, so the segment loop wraps"""
    lower, diag, upper, stride = grid_lines(np.random.default_rng(101), 600, 500, 3, "z", np.float64)
    assert stride == 300_000 > 1024 * 256
    run_case(pkg, gpu, "strided 600x500x3 z-lines", lower, diag, upper, np.float64, 1, 4, stride=stride)


# ---- after iterate(3): UPD = true, z in place over q, r updated in the kernel ------------------------------------------------------

@pytest.mark.parametrize("form", ["fused", "long", "strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_after_three_iterations(pkg, gpu, dtype, form):
    """A = M plus a symmetric coupling of -0.3 that M leaves out (the diagonal raised by 0.6), 2 right-hand sides"""
    R, C, U = rows_per_thread(dtype), chunk_rows(dtype), walk_rows(dtype)
    rng = np.random.default_rng(111)
    if form == "fused":
        lengths = mixed_segments(rng, dtype, 6 * C)
        lower, diag, upper = chain(rng, sum(lengths), dtype, extra=0.6)
        cut(lower, upper, np.cumsum(lengths)[:-1])
        stride, launches, far = 1, 4, (37, -0.3)
    elif form == "long":
        lower, diag, upper = chain(rng, 2 * C + 1, dtype, extra=0.6)
        stride, launches, far = 1, 6, (37, -0.3)
    else:
        lower, diag, upper, stride = grid_lines(rng, 13, 11, 2 * U + 1, "z", dtype, extra=0.6)
        launches, far = 4, (1, -0.3)
    run_case(pkg, gpu, f"{form} UPD", lower, diag, upper, dtype, 2, launches, stride=stride, far=far, iterate=3)


# ---- measured, not asserted ------------------------------------------------------------------------------------------------------

def test_shift_zero_laplacian_is_measured_not_asserted(pkg, gpu):
    """the pure 1-D Laplacian (-1, 2, -1), 50 000 rows, fp32, long form: composing affine maps across an ill-conditioned chain
    loses more than walking it (a CPU restatement of the scan order gave 30x the sequential error), which is a property of the
    form and no indexing fault -- the figures are printed for DESIGN.md and nothing rests on them"""
    n = 50_000
    lower, diag, upper = -np.ones(n, np.float32), 2 * np.ones(n, np.float32), -np.ones(n, np.float32)
    run_case(pkg, gpu, "shift 0 Laplacian", lower, diag, upper, np.float32, 1, 6, assert_sweep=False)
