"""CGAMD_HERMITIAN handles on the GPU: CG with conjugated inner products (csrc/hermitian.hip) against its host restatement herm_ref.cg.

Tolerances are the project's own for solver-against-host comparisons (test_gpu_kernels.py): delta_k relative error 1e-10 in complex128
and 1e-4 in complex64; x relative error 1e-9 and 1e-4.  On these systems a numpy complex64 run of the restatement stays within 2.3e-6
of the complex128 one over 12 iterations, with delta_12 / delta_0 between 6e-8 and 9e-7, so all 13 history rows are compared and none
is masked.  alpha and beta are quotients of two such sums, so they are held to twice the delta bound.

The two smallest systems, n = 1 and n = 2, are solved exactly after n iterations (CG ends there; the next alpha is 0 / 0), so they run n
iterations, not 12, and their last history row -- rounding noise around zero on the device and in numpy alike -- is compared as
|delta_n| <= (64 eps)^2 delta_0 instead of relatively; x is also held to numpy.linalg.solve there.

The unflagged handle's stall (test_the_flag_makes_it_converge) is measured as the issue's table measures it, min_k ||b - A x_k|| / ||b||
over the 40 rows k = 0 .. 39 (numpy: never below 0.35), held to the issue's bound of 0.1.  The history of an unflagged handle is the
UNCONJUGATED r.r, which is no norm: sqrt|delta_k / delta_0| dips to 0.080 (complex128) / 0.075 (complex64) in numpy on this very
right-hand side while the true residual stays above 0.35, so that quotient is printed, not asserted.

Every figure is printed before it is asserted."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import herm_ref as H

pytestmark = pytest.mark.gpu

DT = {"c64": np.complex64, "c128": np.complex128}
ITERS = 12


def tols(dtype):
    """(history, x) relative bounds"""
    return (1e-10, 1e-9) if np.dtype(dtype) == np.complex128 else (1e-4, 1e-4)


# ---- systems, right-hand sides and reference runs: made once ----------------------------------------------------------------------
_SYS, _REF = {}, {}


def system(name):
    if name not in _SYS:
        _SYS[name] = {"n1": lambda: sp.csr_matrix(np.array([[2.5 + 0j]])), "n2": lambda: H.chain(2),
                      "7x5": lambda: H.magnetic(7, 5, 0.13, 0.05), "33x29": lambda: H.magnetic(33, 29, 0.13, 0.05),
                      "33x29b": lambda: H.magnetic(33, 29, 0.29, 0.05), "64x64": lambda: H.magnetic(64, 64, 0.1, 0.01),
                      "chain": lambda: H.chain(70001), "scaled": lambda: scaled("33x29", 11), "scaledb": lambda: scaled("33x29b", 12)}[name]()
    return _SYS[name]


def scaled(name, seed):
    """B = D A D with D = diag(exp(u)), u uniform in [-1.5, 1.5]: Hermitian positive definite, badly scaled, diag(B) real"""
    A = system(name)
    D = sp.diags(np.exp(np.random.default_rng(seed).uniform(-1.5, 1.5, A.shape[0])))
    B = sp.csr_matrix(D @ A @ D)
    B.sort_indices()
    return B


def rhs(n, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)


def ref(name, seed, dtype, iters=ITERS, jacobi=False, tol=None):
    """herm_ref.cg on system `name` with the right-hand side of `seed` AS ROUNDED to dtype, values rounded to dtype as well"""
    key = (name, seed, np.dtype(dtype).name, iters, jacobi, tol)
    if key not in _REF:
        A = system(name).astype(dtype).astype(np.complex128)
        m = 1.0 / A.diagonal().real if jacobi else None
        _REF[key] = H.cg(A, rhs(A.shape[0], seed, dtype), iters, m=m, tol=tol)
    return _REF[key]


def make(pkg, ctx, A, dtype, n_rhs=1, flags=0, hermitian=True, batched=False, values=None):
    vals = np.asarray(A.data if values is None else values).astype(dtype)
    return pkg.Solver(ctx, A.shape[0], A.nnz, vals, A.indptr, A.indices, n_rhs, flags=flags, batched=batched, hermitian=hermitian)


def run(s, b, iters=ITERS):
    s.set_rhs(b)
    s.iterate(iters)
    return s.x(), s.history()


def check_history_shape(h):
    """imaginary parts exactly +0, real parts >= 0"""
    assert np.all(h.imag == 0) and not np.signbit(h.imag).any()
    assert np.all(h.real >= 0)


def check_column(label, x, h, r, want, dtype, exact_after=None):
    """column r of a run against one herm_ref result; exact_after = n of a system CG solves exactly in n iterations"""
    ht, xt = tols(dtype)
    eps = np.finfo(dtype).eps
    n = want["x"].size
    ho, rows = want["history"], len(want["history"])
    got = h[:rows, r].real
    rel = rows if exact_after is None else min(rows, exact_after)
    herr = np.max(np.abs(got[:rel] - ho[:rel]) / ho[:rel])
    xerr = np.linalg.norm(x[r * n:(r + 1) * n] - want["x"]) / np.linalg.norm(want["x"])
    print(f"  {label} {np.dtype(dtype).name} column {r}: {rel} history rows, err {herr:.3e} (< {ht:g}); x err {xerr:.3e} (< {xt:g}); "
          f"delta_last / delta_0 {ho[-1] / ho[0]:.3e}")
    assert herr < ht and xerr < xt
    assert np.all(np.abs(got[rel:]) <= (64 * eps) ** 2 * ho[0]) and np.all(np.abs(ho[rel:]) <= (64 * eps) ** 2 * ho[0])
    if exact_after is None:
        assert np.all(ho > (64 * eps) ** 2 * ho[0])        # nothing compared is rounding noise


@pytest.fixture
def tune(pkg):
    """tune(key, value) before a handle is created (a handle keeps the configuration it was created under); the defaults of struct
    Tuning are put back afterwards"""
    defaults = {"vec_grid": 0, "pad_rows": 1, "index_codes_min_mb": 32, "dev.row_codes_min_mb": 32, "spmm_rowmajor": 1, "resident": 1,
                "two_launch": 1}
    lib = pkg._lib.load()
    touched = []

    def put(key, value):
        assert key in defaults
        touched.append(key)
        pkg._lib.check(lib.cgamd_tune(key.encode(), int(value)))
    yield put
    for key in touched:
        pkg._lib.check(lib.cgamd_tune(key.encode(), defaults[key]))


# ---- 1. the flag is what makes it converge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
def test_the_flag_makes_it_converge(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    A = system("33x29")
    A_t = A.astype(dtype).astype(np.complex128)
    b = rhs(957, 1, dtype)
    iters, bound = (20, 1e-5) if dt == "c128" else (14, 1e-3)
    s = make(pkg, ctx, A, dtype)
    assert s.hermitian == 1 and s.ld == (957 if dt == "c128" else 958)
    x, h = run(s, b, iters)
    s.close()
    res = np.linalg.norm(b.astype(np.complex128) - A_t @ x.astype(np.complex128)) / np.linalg.norm(b)
    u = make(pkg, ctx, A, dtype, hermitian=False)
    assert u.hermitian == 0
    u.set_rhs(b)
    true = [1.0]                # row 0: x0 = 0
    for _ in range(39):
        u.iterate(1)
        true.append(np.linalg.norm(b.astype(np.complex128) - A_t @ u.x().astype(np.complex128)) / np.linalg.norm(b))
    hu = u.history()
    u.close()
    stall, unconj = min(true), np.min(np.sqrt(np.abs(hu[:, 0])) / np.sqrt(np.abs(hu[0, 0])))
    print(f"  {dt}: flagged ||b - A x|| / ||b|| after {iters} iterations {res:.3e} (< {bound:g}); unflagged min ||b - A x_k|| / ||b|| over "
          f"{len(true)} rows {stall:.3f} (> 0.1); its min sqrt|delta_k / delta_0| {unconj:.3f} (no norm: numpy gives 0.080 / 0.075)")
    assert len(hu) == 40 and len(true) == 40
    assert res < bound
    assert stall > 0.1
    check_history_shape(h)


# ---- 2. parity with the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", ["n1", "n2", "7x5", "33x29", "64x64"])
def test_parity(pkg, gpu, name, dt):
    ctx, dtype = gpu[0], DT[dt]
    A = system(name)
    n = A.shape[0]
    iters = min(ITERS, n) if n <= 2 else ITERS
    want = ref(name, 3, dtype, iters)
    s = make(pkg, ctx, A, dtype)
    x, h = run(s, rhs(n, 3, dtype), iters)
    alpha, beta = s.hermitian_scalars()
    assert pkg._lib.load().cgamd_solver_loop_launches(s.handle) == 4
    s.close()
    assert h.shape == (iters + 1, 1)
    check_history_shape(h)
    check_column(name, x, h, 0, want, dtype, exact_after=n if n <= 2 else None)
    assert alpha.imag[0] == 0 and beta.imag[0] == 0
    if n > 2:
        ht = tols(dtype)[0]
        aerr, berr = abs(alpha[0].real - want["alpha"][-1]) / want["alpha"][-1], abs(beta[0].real - want["beta"][-1]) / want["beta"][-1]
        print(f"  {name} {dt}: alpha err {aerr:.3e}, beta err {berr:.3e} (< {2 * ht:g})")
        assert aerr < 2 * ht and berr < 2 * ht
    else:
        exact = np.linalg.solve(A.astype(dtype).astype(np.complex128).toarray(), rhs(n, 3, dtype).astype(np.complex128))
        assert np.linalg.norm(x - exact) / np.linalg.norm(exact) < tols(dtype)[1]


@pytest.mark.parametrize("dt,pad", [("c64", 1), ("c64", 0), ("c128", 1)])
def test_parity_on_a_long_chain_with_two_work_groups(pkg, gpu, tune, dt, pad):
    """70 001 rows on a vector grid of two work-groups: every vector kernel takes its grid-stride loop; complex64 without the
    appended row (pad_rows 0) also takes the scalar tail behind the 16-byte packs"""
    ctx, dtype = gpu[0], DT[dt]
    A = system("chain")
    n = A.shape[0]
    want = ref("chain", 3, dtype)
    tune("vec_grid", 2)
    tune("pad_rows", pad)
    s = make(pkg, ctx, A, dtype)
    assert s.ld == (n + 1 if (dt == "c64" and pad) else n)
    x, h = run(s, rhs(n, 3, dtype))
    alpha, beta = s.hermitian_scalars()
    s.close()
    check_history_shape(h)
    check_column(f"chain pad={pad}", x, h, 0, want, dtype)
    assert alpha.imag[0] == 0 and beta.imag[0] == 0


# ---- 3. cuts and flags leave the bits alone --------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


@pytest.mark.parametrize("dt", list(DT))
def test_cuts_and_flags_keep_the_bits(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    A = system("33x29")
    b = rhs(957, 4, dtype)
    s = make(pkg, ctx, A, dtype)
    x, h = run(s, b)
    s.set_rhs(b)
    s.iterate(5)
    s.iterate(7)
    assert np.array_equal(s.x(), x) and np.array_equal(s.history(), h)
    s.close()
    g = make(pkg, ctx, A, dtype, flags=pkg._lib.NO_GRAPH)
    xg, hg = run(g, b)
    assert g.graph_captures == 0
    g.close()
    assert np.array_equal(xg, x) and np.array_equal(hg, h)
    ip, ix, da = dev(A.indptr.astype(np.int32)), dev(A.indices.astype(np.int32)), dev(A.data.astype(dtype))
    d = pkg.Solver(ctx, 957, A.nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype, hermitian=True)
    assert d.hermitian == 1
    xd, hd = run(d, b)
    d.close()
    assert np.array_equal(xd, x) and np.array_equal(hd, h)


# ---- 4. several right-hand sides and batched handles -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
def test_three_right_hand_sides(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    A = system("33x29")
    s = make(pkg, ctx, A, dtype, n_rhs=3)
    x, h = run(s, np.concatenate([rhs(957, 5 + r, dtype) for r in range(3)]))
    alpha, beta = s.hermitian_scalars()
    s.close()
    check_history_shape(h)
    assert np.all(alpha.imag == 0) and np.all(beta.imag == 0)
    for r in range(3):
        check_column("nRHS 3", x, h, r, ref("33x29", 5 + r, dtype), dtype)


@pytest.mark.parametrize("dt", list(DT))
def test_batched_two_systems(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    A, B = system("33x29"), system("33x29b")
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    s = make(pkg, ctx, A, dtype, n_rhs=2, batched=True, values=np.concatenate([A.data, B.data]))
    assert s.hermitian == 1 and s.systems == 2
    x, h = run(s, np.concatenate([rhs(957, 8, dtype), rhs(957, 9, dtype)]))
    s.close()
    check_history_shape(h)
    check_column("batched", x, h, 0, ref("33x29", 8, dtype), dtype)
    check_column("batched", x, h, 1, ref("33x29b", 9, dtype), dtype)


def test_32_right_hand_sides_keep_the_rhs_major_layout(pkg, gpu, tune):
    """complex64 x 32 is a width the matrix-core path takes (spmm_rowmajor 2: for every supported type); the flagged handle does not"""
    ctx, dtype = gpu[0], np.complex64
    A = system("64x64")
    lib = pkg._lib.load()
    tune("spmm_rowmajor", 2)
    b = np.concatenate([rhs(4096, 40 + r, dtype) for r in range(32)])
    u = make(pkg, ctx, A, dtype, n_rhs=32, hermitian=False)
    u.set_rhs(b)
    print(f"  unflagged layout {lib.cgamd_solver_layout(u.handle)}")
    u.close()
    s = make(pkg, ctx, A, dtype, n_rhs=32)
    x, h = run(s, b)
    assert lib.cgamd_solver_layout(s.handle) == 0 and lib.cgamd_solver_loop_launches(s.handle) == 4
    s.close()
    check_history_shape(h)
    for r in range(32):
        check_column("nRHS 32", x, h, r, ref("64x64", 40 + r, dtype), dtype)


# ---- 5. the coded SpMV forms serve the handle ------------------------------------------------------------------------------------
def test_coded_spmv_forms(pkg, gpu, tune):
    ctx, dtype = gpu[0], np.complex64
    A = system("64x64")
    assert len(np.unique(A.data.astype(dtype))) == 11 and np.diff(A.indptr).max() == 5
    b = rhs(4096, 6, dtype)
    plain = make(pkg, ctx, A, dtype)
    assert plain.index_codes == 0 and plain.value_codes == 0
    x, h = run(plain, b)
    plain.close()
    tune("index_codes_min_mb", 0)
    tune("dev.row_codes_min_mb", 0)
    s = make(pkg, ctx, A, dtype)
    assert s.index_codes > 0 and s.value_codes == 11
    xc, hc = run(s, b)
    form = s.last_spmv_form()
    print(f"  coded form: {form}")
    s.close()
    assert form["family"] in ("vc", "vcp", "rowcode") and form["value_codes"] >= 1 and form["fused"] == 1
    assert np.array_equal(hc, h) and np.array_equal(xc, x)
    check_column("coded", xc, hc, 0, ref("64x64", 6, dtype), dtype)


# ---- 6. tolerance stop -----------------------------------------------------------------------------------------------------------
def test_tolerance_stop(pkg, gpu):
    ctx, dtype = gpu[0], np.complex128
    A = system("33x29")
    bs = [rhs(957, 20 + r) for r in range(3)]
    b = np.concatenate(bs)
    tol = np.array([1e-4, 1e-8, 1e-2]) * [np.linalg.norm(v) for v in bs]
    want = [ref("33x29", 20 + r, dtype, iters=100, tol=float(tol[r])) for r in range(3)]
    s = make(pkg, ctx, A, dtype, n_rhs=3)
    x, its, h = s.solve_until(b, tol=tol, maxit=100)
    print(f"  iterations {its.tolist()}, the restatement's {[w['its'] for w in want]}")
    assert its.tolist() == [w["its"] for w in want]
    assert 12 <= its[0] <= 16 and 25 <= its[1] <= 29          # (about 14 and 27)
    check_history_shape(h)
    assert len(h) == its.max() + 1
    with pytest.raises(pkg._lib.CgAmdError) as e:
        s.iterate(1)
    assert e.value.status == pkg._lib.ERR_STATE
    for r in range(3):
        k = int(its[r])
        check_column("until", x, h, r, want[r], dtype)
        assert np.all(h[k:, r] == h[k, r])                      # the frozen rows repeat
        assert np.sqrt(h[k, r].real) < tol[r] <= np.sqrt(h[k - 1, r].real)
        s.set_rhs(b)
        s.iterate(k)
        assert np.array_equal(s.x()[r * 957:(r + 1) * 957], x[r * 957:(r + 1) * 957])
    s.close()


# ---- 7. Jacobi -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["jacobi", "array"])
def test_jacobi(pkg, gpu, how):
    ctx, dtype = gpu[0], np.complex128
    B = system("scaled")
    b = rhs(957, 13)
    tol = 1e-8 * np.linalg.norm(b)
    want = ref("scaled", 13, dtype, jacobi=True)
    want_its = ref("scaled", 13, dtype, iters=400, jacobi=True, tol=tol)["its"]
    M = "jacobi" if how == "jacobi" else (1.0 / B.diagonal().real).astype(dtype)
    s = make(pkg, ctx, B, dtype)
    s.set_preconditioner(M)
    x, h = run(s, b)
    check_history_shape(h)
    check_column(f"Jacobi ({how})", x, h, 0, want, dtype)
    assert pkg._lib.load().cgamd_solver_loop_launches(s.handle) == 4
    xu, its, _ = s.solve_until(b, tol=tol, maxit=400)
    xp, last = s.pcg(b, M=M, tol=tol, maxit=400)
    s.set_preconditioner(None)
    _, plain, _ = s.solve_until(b, tol=tol, maxit=400)
    print(f"  iterations to 1e-8 ||b||: Jacobi {int(its[0])} (the restatement {want_its}), pcg() {last + 1}, without {int(plain[0])}")
    assert abs(int(its[0]) - want_its) <= 1 and int(its[0]) <= 40 and last + 1 == int(its[0])
    assert int(plain[0]) > 100
    assert np.array_equal(xp, xu)           # pcg() leaves x at the iteration the device-side stop froze it in
    with pytest.raises(pkg._lib.CgAmdError) as e:
        s.pcg(b, M=("line", 1), tol=tol, maxit=10)
    assert e.value.status == pkg._lib.ERR_STATE
    s.close()


@pytest.mark.parametrize("how", ["jacobi", "array"])
def test_batched_jacobi(pkg, gpu, how):
    ctx, dtype = gpu[0], np.complex128
    B0, B1 = system("scaled"), system("scaledb")
    s = make(pkg, ctx, B0, dtype, n_rhs=2, batched=True, values=np.concatenate([B0.data, B1.data]))
    s.set_preconditioner("jacobi" if how == "jacobi" else np.concatenate([1.0 / B0.diagonal().real, 1.0 / B1.diagonal().real]).astype(dtype))
    b = np.concatenate([rhs(957, 13), rhs(957, 14)])
    x, h = run(s, b)
    check_history_shape(h)
    check_column("batched Jacobi", x, h, 0, ref("scaled", 13, dtype, jacobi=True), dtype)
    check_column("batched Jacobi", x, h, 1, ref("scaledb", 14, dtype, jacobi=True), dtype)
    tol = 1e-8 * np.array([np.linalg.norm(b[:957]), np.linalg.norm(b[957:])])
    want = [ref(nm, sd, dtype, iters=400, jacobi=True, tol=float(t))["its"] for nm, sd, t in (("scaled", 13, tol[0]), ("scaledb", 14, tol[1]))]
    _, its, _ = s.solve_until(b, tol=tol, maxit=400)
    print(f"  batched Jacobi iterations {its.tolist()}, the restatement's {want}")
    assert all(abs(int(i) - w) <= 1 and int(i) <= 40 for i, w in zip(its, want))
    s.close()


# ---- 8. refresh ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [None, "jacobi"])
def test_refresh_values_in_place(pkg, gpu, pre):
    import torch
    ctx, dtype = gpu[0], np.complex128
    A = system("33x29")
    b = rhs(957, 15)
    ip, ix, da = dev(A.indptr.astype(np.int32)), dev(A.indices.astype(np.int32)), dev(A.data.astype(dtype))
    s = pkg.Solver(ctx, 957, A.nnz, da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype, hermitian=True)
    if pre:
        s.set_preconditioner(pre)
    x_old, h_old = run(s, b)
    da.mul_(2.0)
    torch.cuda.synchronize()
    s.refresh_values()
    assert s.hermitian == 1 and s.preconditioner_source == (2 if pre else 0)
    x_new, h_new = run(s, b)
    s.close()
    check_column(f"refresh ({pre})", x_old, h_old, 0, ref("33x29", 15, dtype, jacobi=bool(pre)), dtype)
    assert np.array_equal(h_new, h_old)
    assert np.array_equal(2 * x_new, x_old)         # powers of two are exact


def test_reload_matrix(pkg, gpu):
    ctx, dtype = gpu[0], np.complex128
    A, B = system("33x29"), system("33x29b")
    s = make(pkg, ctx, A, dtype)
    s.set_preconditioner("jacobi")
    run(s, rhs(957, 15))
    s.reload_matrix(B.data, B.indptr, B.indices)
    x, h = run(s, rhs(957, 16))
    assert s.hermitian == 1 and s.preconditioner_source == 2
    s.close()
    check_column("reload", x, h, 0, ref("33x29b", 16, dtype, jacobi=True), dtype)


# ---- 9. contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_real_types_ignore_the_flag(pkg, gpu, dtype):
    import cg_numpy
    ctx = gpu[0]
    ip, ix, da = cg_numpy.poisson2d(31)
    n = 31 * 31
    b = np.linspace(1.0, 2.0, n).astype(dtype)
    lib = pkg._lib.load()
    out = []
    for flag in (False, True):
        s = pkg.Solver(ctx, n, len(ix), da.astype(dtype), ip, ix, 1, hermitian=flag)
        assert s.hermitian == 0
        out.append(run(s, b) + (lib.cgamd_solver_loop_launches(s.handle), s.iter_moved_bytes))
        s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2:] == out[1][2:]
    unfused = []
    for flag in (False, True):      # with CGAMD_UNFUSED too: refused on the complex types only
        s = pkg.Solver(ctx, n, len(ix), da.astype(dtype), ip, ix, 1, flags=pkg._lib.UNFUSED, hermitian=flag)
        unfused.append(run(s, b))
        s.close()
    assert np.array_equal(unfused[0][0], unfused[1][0]) and np.array_equal(unfused[0][1], unfused[1][1])


@pytest.mark.parametrize("dt", list(DT))
def test_contract(pkg, gpu, dt):
    ctx, dtype, L = gpu[0], DT[dt], pkg._lib
    lib, ptr = L.load(), L.ptr
    A = system("33x29")
    n, V = 957, np.dtype(dtype).itemsize
    for batched in (False, True):
        with pytest.raises(L.CgAmdError) as e:
            make(pkg, ctx, A, dtype, flags=L.UNFUSED, batched=batched)
        assert e.value.status == L.ERR_INVALID and "CGAMD_UNFUSED" in str(e.value)
    b = np.concatenate([rhs(n, 17 + r, dtype) for r in range(3)])
    s = make(pkg, ctx, A, dtype, n_rhs=3)
    u = make(pkg, ctx, A, dtype, n_rhs=3, hermitian=False)
    assert lib.cgamd_solver_loop_launches(s.handle) == 4 and lib.cgamd_solver_x_lag(s.handle) == 1 and lib.cgamd_solver_layout(s.handle) == 0
    assert s.iter_moved_bytes == u.iter_moved_bytes + 2 * n * V * 3
    assert s.iter_bytes(True) == s.spmv_bytes + 10 * n * V * 3
    assert s.spmv_moved_bytes == u.spmv_moved_bytes
    u.close()
    x, h = run(s, b)
    # not served: refused with the reason, the handle untouched
    one = np.ones(n, dtype)
    its = ctypes.c_int(-7)
    refused = {"tridiag": lib.cgamd_solver_set_preconditioner_tridiag(s.handle, ptr(one), ptr(one), ptr(one), 0),
               "strided": lib.cgamd_solver_set_preconditioner_tridiag_strided(s.handle, 33, ptr(one), ptr(one), ptr(one), 0),
               "line": lib.cgamd_solver_set_preconditioner_line(s.handle, 1),
               "iterate_tol": lib.cgamd_solver_iterate_tol(s.handle, 10, 1e-3, ctypes.byref(its))}
    assert b"CGAMD_HERMITIAN" in lib.cgamd_last_error()
    assert all(v == L.ERR_STATE for v in refused.values()), refused
    assert its.value == -7 and s.preconditioner_source == 0 and s.iterations_done() == ITERS
    assert np.array_equal(s.x(), x) and np.array_equal(s.history(), h)
    out = (ctypes.c_int * 11)()
    assert lib.cgamd_solver_step_plan(s.handle, out, 11) == -L.ERR_INVALID
    cnt = ctypes.c_longlong()
    assert lib.cgamd_solver_step_state(s.handle, 2, ptr(one), n, ctypes.byref(cnt)) == L.ERR_INVALID
    x2, h2 = run(s, b)
    assert np.array_equal(x2, x) and np.array_equal(h2, h)
    s.set_preconditioner("jacobi")
    assert s.iter_moved_bytes == s.spmv_moved_bytes + 12 * n * V * 3 and lib.cgamd_solver_loop_launches(s.handle) == 4
    s.close()
    g = make(pkg, ctx, A, dtype, flags=L.NO_GRAPH)
    assert lib.cgamd_solver_loop_launches(g.handle) == 4 and lib.cgamd_solver_x_lag(g.handle) == 1
    g.close()
    sb = make(pkg, ctx, A, dtype, n_rhs=2, batched=True, values=np.concatenate([A.data, A.data]))
    assert lib.cgamd_solver_set_preconditioner_batched_line(sb.handle, 1) == L.ERR_STATE
    sb.close()
    un = make(pkg, ctx, A, dtype, hermitian=False)
    assert lib.cgamd_solver_hermitian_scalars(un.handle, None, None) == L.ERR_STATE
    un.close()


def test_development_spmv_entry_stays_unconjugated(pkg, gpu):
    ctx, dtype = gpu[0], np.complex128
    A = system("33x29")
    v = rhs(957, 18)
    s = make(pkg, ctx, A, dtype)
    import torch
    xd, yd = dev(v), dev(np.zeros(957, dtype))
    torch.cuda.synchronize()
    s.spmv(xd, yd, fused_dot=True)
    ctx.synchronize()
    got = s.dot_partials().sum()
    s.close()
    want = v @ (A @ v)
    assert abs(got - want) / abs(want) < 1e-12 and abs(want.imag) > 1e-3 * abs(want)


# ---- 10. the command-line front end ----------------------------------------------------------------------------------------------
def test_cli_hermitian(pkg, gpu, tmp_path):
    A = system("7x5").tocoo()
    low = A.row >= A.col
    path, out = tmp_path / "herm.mtx", tmp_path / "hist.bin"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex hermitian\n")
        f.write(f"35 35 {int(low.sum())}\n")
        for i, j, v in zip(A.row[low], A.col[low], A.data[low]):
            f.write(f"{i + 1} {j + 1} {float(v.real)!r} {float(v.imag)!r}\n")
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "oclcgex")
    r = subprocess.run([exe, str(path), "1", "1", "12", "--double", "--hermitian", "--quiet", "--history", str(out)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    h = np.fromfile(out, dtype=np.float64).reshape(13, 2)
    want = H.cg(system("7x5"), np.full(35, 5.0), 12)["history"]
    err = np.max(np.abs(h[:, 0] - want) / want)
    print(f"  oclcgex --hermitian: 13 delta_k, err {err:.3e} (< 1e-10)")
    assert err < 1e-10 and np.all(h[:, 1] == 0)
    r = subprocess.run([exe, str(path), "1", "1", "12", "--double", "--quiet", "--history", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    plain = np.fromfile(out, dtype=np.float64).reshape(13, 2)
    assert np.max(np.abs(plain[:, 0] - want) / want) > 1e-3         # the default stays the unconjugated recurrence
