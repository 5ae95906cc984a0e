"""Multi-shift CG on the GPU (cgamd_solver_set_shifts, csrc/shifts.hip): all (A + sigma_j I) x_j = b on the SpMV of A x = b.

Systems: the 33 x 29 five-point Laplacian (float32 / float64, shifts 0.05, 0.7, 6) and L - (0.3 + 0.2i) I (complex64 / complex128,
complex symmetric, unconjugated dots, shifts 0.05 + 0.1i, 0.7 - 0.3i, 6 + i), 30 iterations; a 7 x 5 system with three right-hand
sides; n = 1.  The reference is tests/shift_ref.py (the ratio form in numpy, itself held to separate CG solves by
tests/test_shift_ref.py), run in float64 / complex128 on the matrix, right-hand side and shifts AS ROUNDED to the handle's type.

Bounds.  x_j: the project's solver-against-host tolerances (test_gpu_hermitian.py::tols, from test_gpu_kernels.py), 1e-9 for float64 /
complex128 and 1e-4 for float32 / complex64, relative to max|x_j|.  zeta: the same two numbers, relative to the largest |zeta_k^j| of
the column compared (k = 0 .. 30; at least 1, row 0) -- the normalisation of x.  A numpy run of the restatement in the value type
stays within 2.8e-7 (float32) and 1.8e-6 (complex64) of the wide one in x_j and within 5.2e-8 / 2.1e-6 in zeta on these right-hand
sides.  (The complex system is indefinite, and zeta carries the rounding of every alpha_k, beta_k before it: per entry, relative
to |zeta_k| itself -- 5e-19 in the last row of the largest shift -- numpy's own complex64 run is off by up to 5.2e-5 here and by up
to 4.4e-4 on other right-hand sides, which is why the bound is not stated per entry; the per-entry figure is printed.)
What the scalar kernel computes is held much tighter, in test_scalar_step_follows_the_recurrence: driven by the DEVICE's own
alpha_k, beta_k (read back after every iteration), the restated recurrence must give the device's theta and zeta to 1e-12 relative --
12 steps of a dozen double operations each, 1.1e-16 apiece, and the two complex divisions (Smith's on the device, numpy's on the
host) agree to a few ulps.

Bits.  With shifts set the seed's x and history are array_equal to the same handle without shifts; iterate(7); iterate(23),
iterate(30), CGAMD_NO_GRAPH and a second run give the same x_j and zeta; a column frozen by iterate_until keeps, for every shift, the
bits of iterate(its_r).  sigma = 0 returns the seed's x array_equal on the real types (every factor is exactly 1); complex division
does not promise that, so the complex types are held to the tolerance.

Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import shift_ref as M

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
ALL = list(DT)
ITERS = 30
REAL_SHIFTS, CPLX_SHIFTS = (0.05, 0.7, 6.0), (0.05 + 0.1j, 0.7 - 0.3j, 6 + 1j)


def tol(dtype):
    return 1e-9 if np.dtype(dtype).itemsize // (2 if np.dtype(dtype).kind == "c" else 1) == 8 else 1e-4


def shifts_of(dtype):
    return np.asarray(CPLX_SHIFTS if np.dtype(dtype).kind == "c" else REAL_SHIFTS, dtype=dtype)


# ---- systems, right-hand sides and reference runs: made once -------------------------------------------------------------------------
_SYS, _REF = {}, {}


def system(name, dtype):
    """CSR matrix in the accumulator type with the values as rounded to dtype"""
    dtype = np.dtype(dtype)
    key = (name, dtype.name)
    if key not in _SYS:
        if name == "n1":
            A = sp.csr_matrix(np.array([[4.0 - (0.3 + 0.2j)]])) if dtype.kind == "c" else sp.csr_matrix(np.array([[4.0]]))
        else:
            nx, ny = {"33x29": (33, 29), "7x5": (7, 5)}[name]
            A = M.shifted_laplace2d(nx, ny, 0.3 + 0.2j) if dtype.kind == "c" else M.laplace2d(nx, ny)
        A = sp.csr_matrix(A.astype(dtype).astype(M.acc_type(dtype)))
        A.sort_indices()
        _SYS[key] = A
    return _SYS[key]


def rhs(n, seed, dtype, nrhs=1):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((nrhs, n))
    if np.dtype(dtype).kind == "c":
        b = b + 1j * rng.standard_normal((nrhs, n))
    return b.astype(dtype)


def ref(name, dtype, seed, nrhs=1, iters=ITERS, sigmas=None):
    """shift_ref.mscg per right-hand side, in the accumulator type"""
    dtype = np.dtype(dtype)
    sig = shifts_of(dtype) if sigmas is None else np.asarray(sigmas, dtype=dtype)
    key = (name, dtype.name, seed, nrhs, iters, sig.tobytes())
    if key not in _REF:
        A = system(name, dtype)
        B = rhs(A.shape[0], seed, dtype, nrhs)
        _REF[key] = [M.mscg(A, B[r].astype(M.acc_type(dtype)), sig.astype(M.acc_type(dtype)), iters) for r in range(nrhs)]
    return _REF[key]


def make(pkg, ctx, name, dtype, nrhs=1, flags=0, **kw):
    A = system(name, dtype)
    return pkg.Solver(ctx, A.shape[0], A.nnz, A.data.astype(dtype), A.indptr, A.indices, nrhs, flags=flags, **kw)


def run(s, b, iters=ITERS, pieces=None):
    s.set_rhs(b)
    for k in (pieces or (iters,)):
        s.iterate(k)
    out = {"x": s.x().reshape(s.n_rhs, -1), "h": s.history()}
    if s.shifts():
        out["xs"], out["zeta"] = s.x_shifted(), s.shift_history()
    return out


def same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int(np.count_nonzero(a != b))} values differ"


def check_against_ref(label, got, want, dtype):
    """x_j and zeta of every column against shift_ref, in the bounds of the module docstring"""
    t = tol(dtype)
    for r, w in enumerate(want):
        for j in range(w["xs"].shape[0]):
            xerr = np.max(np.abs(got["xs"][j, r] - w["xs"][j])) / np.max(np.abs(w["xs"][j]))
            zcol, zref = got["zeta"][:, j, r], w["zeta"][:, j]
            zerr = np.max(np.abs(zcol - zref)) / np.max(np.abs(zref))
            entry = np.max(np.abs(zcol - zref) / np.abs(zref))
            print(f"  {label} {np.dtype(dtype).name} column {r} shift {j}: x_j err {xerr:.3e}, zeta err {zerr:.3e} (< {t:g}); zeta per entry "
                  f"{entry:.3e}, |zeta_last| {abs(zref[-1]):.3e}")
            assert xerr < t and zerr < t


# ---- 1. seed bits and accuracy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
def test_seed_keeps_its_bits_and_the_shifted_solutions_match_the_host(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    for name, nrhs, iters, seed in (("33x29", 1, ITERS, 5), ("7x5", 3, 12, 6), ("n1", 1, 1, 7)):
        A = system(name, dtype)
        b = rhs(A.shape[0], seed, dtype, nrhs)
        plain, s = make(pkg, ctx, name, dtype, nrhs), make(pkg, ctx, name, dtype, nrhs)
        try:
            assert s.shifts() == 0
            s.set_shifts(shifts_of(dtype))
            assert s.shifts() == 3 and plain.shifts() == 0
            want_seed, got = run(plain, b, iters), run(s, b, iters)
            same(got["x"], want_seed["x"], f"seed x {name}")
            same(got["h"], want_seed["h"], f"seed history {name}")
            assert got["xs"].shape == (3, nrhs, A.shape[0]) and got["zeta"].shape == (iters + 1, 3, nrhs)
            assert np.all(got["zeta"][0] == 1)
            check_against_ref(name, got, ref(name, dtype, seed, nrhs, iters), dtype)
            if name == "n1":        # one iteration solves a 1 x 1 system: x_j = b / (a + sigma_j)
                exact = b[0, 0].astype(M.acc_type(dtype)) / (A[0, 0] + shifts_of(dtype).astype(M.acc_type(dtype)))
                err = np.max(np.abs(got["xs"][:, 0, 0] - exact) / np.abs(exact))
                print(f"  n1 {dt}: against b / (a + sigma) {err:.3e}")
                assert err < tol(dtype)
        finally:
            plain.close()
            s.close()


# ---- 2. the scalar step, driven by the device's own alpha and beta ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
def test_scalar_step_follows_the_recurrence(pkg, gpu, dt):
    ctx, dtype = gpu[0], np.dtype(DT[dt])
    ct, eps = M.acc_type(dtype), np.finfo(dtype).eps
    sig = shifts_of(dtype)
    s = make(pkg, ctx, "7x5", dtype, 3)
    try:
        s.set_shifts(sig)
        s.set_rhs(rhs(35, 8, dtype, 3))
        th, ze = np.ones((3, 3), ct), np.ones((3, 3), ct)
        ap, bp = np.ones(3, ct), np.zeros(3, ct)
        worst = 0.0
        for k in range(12):
            s.iterate(1)
            al, be = s.step_state("alpha").astype(ct), s.step_state("beta").astype(ct)
            th = M.theta_step(al[None], ap[None], bp[None], th, sig.astype(ct)[:, None])
            ze = ze * th
            dth, dze = s.shift_scalars("theta"), s.shift_scalars("zeta")
            worst = max(worst, np.max(np.abs(dth - th) / np.abs(th)), np.max(np.abs(dze - ze) / np.abs(ze)))
            # alpha_j, beta_j and the history row: the device's own theta and zeta, rounded once
            aj, bj = s.shift_scalars("alpha"), s.shift_scalars("beta")
            assert np.max(np.abs(aj - al[None] * dth) / np.abs(al[None] * dth)) <= 2 * eps
            assert np.max(np.abs(bj - be[None] * dth * dth) / np.abs(be[None] * dth * dth)) <= 4 * eps
            same(s.shift_history()[k + 1], dze.astype(dtype), f"history row {k + 1}")
            ap, bp = al, be
        print(f"  {dt}: theta and zeta against the recurrence on the device's alpha, beta: {worst:.3e} (< 1e-12)")
        assert worst < 1e-12
    finally:
        s.close()


# ---- 3. sigma = 0 is the seed --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
def test_zero_shift_returns_the_seed(pkg, gpu, dt):
    ctx, dtype = gpu[0], np.dtype(DT[dt])
    s = make(pkg, ctx, "33x29", dtype)
    try:
        s.set_shifts(np.asarray([0.7, 0.0], dtype=dtype))
        got = run(s, rhs(957, 5, dtype))
        if dtype.kind != "c":
            same(got["xs"][1], got["x"], "x of sigma = 0")
            assert np.all(got["zeta"][:, 1] == 1)
        err = np.max(np.abs(got["xs"][1] - got["x"])) / np.max(np.abs(got["x"]))
        print(f"  {dt}: x of sigma = 0 against the seed's {err:.3e}")
        assert err < tol(dtype)
    finally:
        s.close()


# ---- 4. the same bits however the iterations are asked for ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
def test_bits_do_not_depend_on_the_call_pattern(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    b = rhs(957, 5, dtype, 2)
    runs = {}
    for label, flags, pieces in (("30", 0, (30,)), ("7 + 23", 0, (7, 23)), ("no graph", pkg._lib.NO_GRAPH, (30,)), ("ones", 0, (1,) * 30)):
        s = make(pkg, ctx, "33x29", dtype, 2, flags)
        try:
            s.set_shifts(shifts_of(dtype))
            runs[label] = run(s, b, pieces=pieces)
            if label == "30":
                runs["again"] = run(s, b)
        finally:
            s.close()
    for label, got in runs.items():
        for key in ("x", "h", "xs", "zeta"):
            same(got[key], runs["30"][key], f"{key} of '{label}'")


# ---- 5. tolerance stop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
def test_iterate_until_freezes_every_shift_with_its_column(pkg, gpu, dt):
    ctx, dtype = gpu[0], DT[dt]
    b = rhs(957, 9, dtype, 3)
    s = make(pkg, ctx, "33x29", dtype, 3)
    try:
        s.set_shifts(shifts_of(dtype))
        s.set_rhs(b)
        norm0 = np.sqrt(np.abs(np.sum(b.astype(M.acc_type(dtype)) ** 2, axis=1)))
        its = s.iterate_until(norm0 * np.array([0.3, 0.05, 0.005]), 200, check_every=5)
        x, h, xs, zeta = s.x().reshape(3, -1), s.history(), s.x_shifted(), s.shift_history()
        print(f"  {dt}: stopped after {its.tolist()} iterations")
        assert len(set(its.tolist())) == 3 and its.max() < 200
        assert zeta.shape[0] == its.max() + 1
        for r in range(3):
            s.set_rhs(b)
            s.iterate(int(its[r]))
            same(s.x().reshape(3, -1)[r], x[r], f"x column {r}")
            same(s.x_shifted()[:, r], xs[:, r], f"x_j column {r}")
            zr = s.shift_history()
            same(zr[:, :, r], zeta[:its[r] + 1, :, r], f"zeta column {r}")
            same(zeta[its[r]:, :, r], np.broadcast_to(zeta[its[r], :, r], zeta[its[r]:, :, r].shape).copy(), f"zeta column {r} repeats its last entry")
            same(s.history()[:, r], h[:its[r] + 1, r], f"history column {r}")
    finally:
        s.close()


# ---- 6. contract ---------------------------------------------------------------------------------------------------------------------------
def _state(s):
    out = [s.x().copy(), s.history().copy(), s.preconditioner_source, s.shifts()]
    if s.shifts():
        out += [s.x_shifted().copy(), s.shift_history().copy()]
    return out


def _unchanged(s, before, what):
    for a, b in zip(_state(s), before):
        if isinstance(a, np.ndarray):
            same(a, b, what)
        else:
            assert a == b, what


def test_set_shifts_refuses_what_it_does_not_serve(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    sig = np.asarray(REAL_SHIFTS)
    A = system("33x29", np.float64)
    b = rhs(957, 5, np.float64)[0]

    def refused(s, rhs_block, reason, layout=0):
        s.set_rhs(rhs_block)
        assert lib.cgamd_solver_layout(s.handle) == layout
        s.iterate(5)
        before = _state(s)
        assert lib.cgamd_solver_set_shifts(s.handle, L.ptr(sig.astype(s.dtype)), 3) == L.ERR_STATE, reason
        assert reason.encode() in lib.cgamd_last_error(), (reason, lib.cgamd_last_error())
        _unchanged(s, before, reason)
        s.iterate(3)                                # and it goes on
        s.close()

    refused(pkg.Solver(ctx, 957, A.nnz, np.tile(A.data, 2), A.indptr, A.indices, 2, batched=True), np.tile(b, 2), "batched")
    Ac = system("33x29", np.complex128)
    refused(pkg.Solver(ctx, 957, Ac.nnz, Ac.data, Ac.indptr, Ac.indices, 1, hermitian=True), rhs(957, 5, np.complex128)[0], "CGAMD_HERMITIAN")
    refused(make(pkg, ctx, "33x29", np.float64, flags=L.UNFUSED), b, "CGAMD_UNFUSED")
    L.check(lib.cgamd_tune(b"spmm_rowmajor", 2))             # fp64 x 16 keeps its right-hand sides interleaved under this knob
    try:
        rm = make(pkg, ctx, "33x29", np.float64, 16)
    finally:
        L.check(lib.cgamd_tune(b"spmm_rowmajor", 1))
    refused(rm, np.tile(b, 16), "row-major", layout=1)
    pre = make(pkg, ctx, "33x29", np.float64)
    pre.set_preconditioner("jacobi")
    refused(pre, b, "preconditioner")
    # a real handle created with the Hermitian flag runs the plain recurrence and is served
    s = make(pkg, ctx, "33x29", np.float64, hermitian=True)
    try:
        s.set_shifts(sig)
        check_against_ref("hermitian flag on a real type", run(s, b), ref("33x29", np.float64, 5), np.float64)
    finally:
        s.close()


def test_what_is_refused_with_shifts_in_force(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    dtype = np.dtype(np.float64)
    b = rhs(957, 5, dtype)[0]
    s = make(pkg, ctx, "33x29", dtype)
    try:
        s.set_shifts(shifts_of(dtype))
        s.enable_projection(2)
        got = run(s, b, 10)
        before = _state(s)
        h, p, one = s.handle, L.ptr, np.ones(957)
        its = ctypes.c_int()
        bad = np.array([1.0, np.inf])
        calls = {
            "set_preconditioner": (lambda: lib.cgamd_solver_set_preconditioner(h, p(one), 0), L.ERR_STATE),
            "set_preconditioner_tridiag": (lambda: lib.cgamd_solver_set_preconditioner_tridiag(h, p(one), p(4 * one), p(one), 0), L.ERR_STATE),
            "set_preconditioner_tridiag_strided": (lambda: lib.cgamd_solver_set_preconditioner_tridiag_strided(h, 33, p(one), p(4 * one), p(one), 0), L.ERR_STATE),
            "set_preconditioner_line": (lambda: lib.cgamd_solver_set_preconditioner_line(h, 1), L.ERR_STATE),
            "set_preconditioner_jacobi": (lambda: lib.cgamd_solver_set_preconditioner_jacobi(h), L.ERR_STATE),
            "set_preconditioner_multigrid": (lambda: lib.cgamd_solver_set_preconditioner_multigrid(h, 33, 29, 1, 0, 0.0, 0), L.ERR_STATE),
            "set_preconditioner_amg": (lambda: lib.cgamd_solver_set_preconditioner_amg(h, 0, 0.0, 0, 0.0, 0), L.ERR_STATE),
            "iterate_tol": (lambda: lib.cgamd_solver_iterate_tol(h, 5, 1e-3, ctypes.byref(its)), L.ERR_STATE),
            "replace_residual": (lambda: lib.cgamd_solver_replace_residual(h, s.vector("q")), L.ERR_STATE),
            "set_rhs_projected": (lambda: lib.cgamd_solver_set_rhs_projected(h, p(b), 0), L.ERR_STATE),
            "set_rhs": (lambda: lib.cgamd_solver_set_rhs(h, p(b), p(one), 0), L.ERR_INVALID),
            "set_shifts: nShifts": (lambda: lib.cgamd_solver_set_shifts(h, p(np.ones(17)), 17), L.ERR_INVALID),
            "set_shifts: shift 1 is not finite": (lambda: lib.cgamd_solver_set_shifts(h, p(bad), 2), L.ERR_INVALID),
        }
        for who, (call, status) in calls.items():
            assert call() == status, who
            assert who.split(":")[0].encode() in lib.cgamd_last_error() and who.split(": ")[-1].encode() in lib.cgamd_last_error(), (who, lib.cgamd_last_error())
            _unchanged(s, before, who)
        assert lib.cgamd_solver_get_x_shifted(h, 3, p(one), 0) == L.ERR_INVALID
        s.iterate(20)                               # the solve goes on where it was
        # removing a preconditioner that is not there stays served, and so does every plain call
        s.set_preconditioner(None)
        assert s.shifts() == 3
        check_against_ref("after the refusals", run(s, b), ref("33x29", dtype, 5), dtype)
        same(got["xs"], run(s, b, 10)["xs"], "the first ten iterations again")
    finally:
        s.close()


@pytest.mark.parametrize("dt", ("f32", "c128"))
def test_removal_refresh_and_the_models(pkg, gpu, dt):
    ctx, lib, dtype = gpu[0], pkg._lib.load(), np.dtype(DT[dt])
    b = rhs(957, 5, dtype)[0]
    A = system("33x29", dtype)
    plain, s = make(pkg, ctx, "33x29", dtype), make(pkg, ctx, "33x29", dtype)
    try:
        want = run(plain, b)
        launches, moved, counted = lib.cgamd_solver_loop_launches(s.handle), s.iter_moved_bytes, s.iter_bytes(True)
        s.set_rhs(b)
        per_launched = []
        for S in (1, 3, 16):
            s.set_shifts(np.linspace(0.1, 2.0, S).astype(dtype))
            grown = (4 * S + 1) * 957 * dtype.itemsize
            per_launched.append(lib.cgamd_solver_loop_launches(s.handle))
            # (a handle whose iterate() runs a resident loop reports the launched loop's bytes with and without shifts)
            assert s.iter_moved_bytes == moved + grown and s.iter_bytes(True) == counted + grown, S
        print(f"  {dt}: launches per iteration {launches} without shifts, {per_launched} with 1, 3, 16")
        assert len(set(per_launched)) == 1 and per_launched[0] in (5, 6) and per_launched[0] >= launches + 2
        # the next call must be set_rhs
        assert lib.cgamd_solver_iterate(s.handle, 1) == pkg._lib.ERR_STATE
        # refresh_values keeps the shifts: the same solve on 2 A has x_j(2 A, 2 sigma) = x_j(A, sigma) / 2
        s.set_shifts(2 * shifts_of(dtype))
        s.refresh_values((2 * A.data).astype(dtype))
        assert s.shifts() == 3
        got = run(s, b)
        w = ref("33x29", dtype, 5)[0]
        for j in range(3):
            err = np.max(np.abs(2 * got["xs"][j, 0] - w["xs"][j])) / np.max(np.abs(w["xs"][j]))
            print(f"  {dt}: after refresh_values, shift {j}: {err:.3e}")
            assert err < tol(dtype)
        # removal: the bits of a handle that never had shifts
        s.refresh_values(A.data.astype(dtype))
        s.set_shifts(None)
        assert s.shifts() == 0 and lib.cgamd_solver_loop_launches(s.handle) == launches and s.iter_moved_bytes == moved
        assert lib.cgamd_solver_iterate(s.handle, 1) == pkg._lib.ERR_STATE
        got = run(s, b)
        same(got["x"], want["x"], "x after removal")
        same(got["h"], want["h"], "history after removal")
        assert lib.cgamd_solver_get_x_shifted(s.handle, 0, pkg._lib.ptr(np.ones(957, dtype)), 0) == pkg._lib.ERR_STATE
        s.set_shifts([])                            # removing what is not there is served, and changes nothing
        s.iterate(1)
    finally:
        plain.close()
        s.close()


# ---- 7. other SpMV forms -------------------------------------------------------------------------------------------------------------------
FORM_DEFAULTS = {"resident": 1, "index_codes_min_mb": 32, "dev.row_codes_min_mb": 32, "dev.long_row_bytes": 0}


@pytest.fixture
def tuned(pkg):
    lib = pkg._lib.load()

    def put(**kv):
        for k, v in kv.items():
            k = k.replace("dev_", "dev.")
            assert k in FORM_DEFAULTS, k
            pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))
    yield put
    for k, v in FORM_DEFAULTS.items():
        pkg._lib.check(lib.cgamd_tune(k.encode(), v))


@pytest.mark.parametrize("form", ("value_coded", "long_rows"))
def test_coded_and_split_handles_agree_with_the_plain_one(pkg, gpu, tuned, form):
    ctx, dtype = gpu[0], np.dtype(np.float64)
    b = rhs(957, 5, dtype)[0]
    plain = make(pkg, ctx, "33x29", dtype)
    if form == "value_coded":
        tuned(resident=0, index_codes_min_mb=0, dev_row_codes_min_mb=0)
    else:
        tuned(resident=0, dev_long_row_bytes=64)
    other, unshifted = (make(pkg, ctx, "33x29", dtype, long_rows=form == "long_rows") for _ in range(2))
    try:
        if form == "value_coded":
            print(f"  value codes {other.value_codes}, row codes {other.row_codes}")
            assert other.value_codes > 0
        else:
            print(f"  long rows {other.long_rows}")
            assert other.long_rows["heavy_blocks"] > 0
        plain.set_shifts(shifts_of(dtype))
        other.set_shifts(shifts_of(dtype))
        want, got, seed = run(plain, b), run(other, b), run(unshifted, b)
        same(got["x"], seed["x"], f"seed x of the {form} handle")
        same(got["h"], seed["h"], f"seed history of the {form} handle")
        check_against_ref(form, got, ref("33x29", dtype, 5), dtype)
        err = np.max(np.abs(got["xs"] - want["xs"])) / np.max(np.abs(want["xs"]))
        print(f"  {form}: x_j against the plain handle's {err:.3e}, bit-equal: {got['xs'].tobytes() == want['xs'].tobytes()}")
        assert err < tol(dtype)
    finally:
        for s in (plain, other, unshifted):
            s.close()


# ---- 8. the residual of a shifted system is zeta r -----------------------------------------------------------------------------------------
def test_true_residual_is_zeta_times_the_seeds(pkg, gpu):
    """float64, 30 iterations, sigma in {0.05, 0.7}: both residuals are still far above rounding (4.6e-2 and 4.5e-7 in numpy, 1.5e-3
    and 1.5e-8 of ||b||), so ||b - (A + sigma_j) x_j|| must match |zeta_30^j| sqrt(delta_30) to 1e-6 relative"""
    ctx, dtype = gpu[0], np.dtype(np.float64)
    A = system("33x29", dtype)
    b = rhs(957, 5, dtype)[0]
    s = make(pkg, ctx, "33x29", dtype)
    try:
        s.set_shifts([0.05, 0.7])
        got = run(s, b)
        for j, sigma in enumerate((0.05, 0.7)):
            true = np.linalg.norm(b - (A @ got["xs"][j, 0] + sigma * got["xs"][j, 0]))
            claimed = abs(got["zeta"][-1, j, 0]) * np.sqrt(got["h"][-1, 0])
            print(f"  sigma {sigma}: ||b - (A + sigma) x_j|| {true:.6e}, |zeta| sqrt(delta) {claimed:.6e}, relative to ||b|| {true / np.linalg.norm(b):.3e}")
            assert abs(true - claimed) <= 1e-6 * true
    finally:
        s.close()


# ---- 9. the convenience call ---------------------------------------------------------------------------------------------------------------
def test_solve_shifted(pkg, gpu):
    ctx, dtype = gpu[0], np.dtype(np.float64)
    b = rhs(957, 5, dtype)[0]
    A = system("33x29", dtype)
    s = make(pkg, ctx, "33x29", dtype)
    try:
        x, xs, its = s.solve_shifted(b, REAL_SHIFTS, iterations=ITERS)
        assert its.tolist() == [ITERS] and xs.shape == (3, 1, 957) and x.shape == (957,)
        check_against_ref("solve_shifted", {"xs": xs, "zeta": s.shift_history()}, ref("33x29", dtype, 5), dtype)
        x, xs, its = s.solve_shifted(b, REAL_SHIFTS, tol=1e-9 * np.linalg.norm(b), maxit=500)
        print(f"  to 1e-9 ||b||: {its.tolist()} iterations")
        assert 0 < its[0] < 500
        for j, sigma in enumerate(REAL_SHIFTS):     # positive shifts of a positive-definite matrix converge with the seed
            res = np.linalg.norm(b - (A @ xs[j, 0] + sigma * xs[j, 0])) / np.linalg.norm(b)
            print(f"  sigma {sigma}: true residual {res:.3e}")
            assert res < 1e-8
    finally:
        s.close()
