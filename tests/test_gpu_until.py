"""cgamd_solver_iterate_until / Solver.iterate_until / solve_until / solve_subdomains(tol=): the per-right-hand-side tolerance stop of
the launched loops, decided on the device.

The yardstick is never the new code: it is the SAME handle's fixed-iteration run, `set_rhs; iterate(maxit); history()`.  From that
history (taken to float64 / complex128, as the device takes it) the expected stopping iteration of column r is the first row k >= 1
with not (sqrt|delta_k[r]| >= tol_r); the expected x column comes from `set_rhs; iterate(its_r)`; the expected history column is the
fixed-count one down to row its_r and repeats that entry below.  Everything is compared bit for bit (np.array_equal, NaN positions
equal), for check_every in {1, 3, 8} and for until(a); until(b) against until(a + b).

Tolerances are placed BETWEEN two values of the yardstick history (the geometric mean of a new record low of the column's norm and
the record before it, at least 3 % apart), so no decision hangs on the last bits of sqrt / hypot.  Every multi-right-hand-side case
carries scaled copies 10^-r b under one tolerance (stops in different iterations), one that never stops (maxit reached; where the
system is so small that CG ends by itself the rule says where), an all-zero column (delta_1 = NaN: it stops in iteration 1 and must
not disturb its neighbours) and, from five columns on, a non-zero one that stops in iteration 1; `flip` puts the zero column first,
so right-hand side 0 -- the one that advances the iteration counter -- is the earliest stopper.

Shapes are the smallest that reach each path, the thresholds read from the code: alpha is folded into the r update up to
kFoldAlphaMax = 2048 d.q partials (one per 256 rows: 524 288 rows) and cg_alpha is a launch of its own beyond (740 x 740 = 547 600
rows, 2140 partials); cg_alpha2 takes over at 16 384 partials (2048 x 2048 = 4 194 304 rows).  The partial count of every handle is
asserted (cgamd_solver_dot_partials), so a case cannot silently run another kernel than it names."""
import ctypes
import types

import numpy as np
import pytest
import scipy.sparse as sp

import cg_numpy

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
CHUNKS = (1, 3, 8)


def wide(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


# ---- systems (host CSR in the wide type), made once ------------------------------------------------------------------------------------
_SYS = {}


def chain(n, far=0.0):
    """1-D chain, diag 2.5 (+ 2 far), -1 at distance 1 and -far at distance 3: SPD, rows of 1 to 5 entries"""
    diags, offs = [np.full(n, 2.5 + 2 * far)], [0]
    if n > 1:
        diags += [np.full(n - 1, -1.0)] * 2
        offs += [-1, 1]
    if far and n > 3:
        diags += [np.full(n - 3, -far)] * 2
        offs += [-3, 3]
    A = sp.diags(diags, offs, format="csr")
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def system(kind):
    if kind not in _SYS:
        if kind.startswith("chain"):
            _SYS[kind] = chain(int(kind[5:]))
        elif kind.startswith("far"):
            _SYS[kind] = chain(int(kind[3:]), far=0.7)
        elif kind.startswith("poisson"):
            _SYS[kind] = cg_numpy.poisson2d(int(kind[7:]))
        elif kind.startswith("helm"):
            N = int(kind[4:])
            _SYS[kind] = cg_numpy.helm_fe_var(N, 12.0, np.ones((N - 1, N - 1)), 0.15, N, N)
        else:
            raise ValueError(kind)
    return _SYS[kind]


def values(kind, dtype):
    ip, ix, da = system(kind)
    if np.dtype(dtype).kind == "c" and not np.iscomplexobj(da):
        da = da * (1.0 + 0.05j)                     # complex symmetric: the unconjugated recurrence has something to do
    return ip, ix, np.asarray(da).astype(dtype)


def apply_matrix(kind, dtype, u):
    """A u in the wide type, A as values(kind, dtype) gives it (the 5-point stencil on the grid: no host matrix for the large ones)"""
    if kind.startswith("poisson"):
        N = int(kind[7:])
        g = u.reshape(N, N)
        y = 4.0 * g
        y[1:, :] -= g[:-1, :]
        y[:-1, :] -= g[1:, :]
        y[:, 1:] -= g[:, :-1]
        y[:, :-1] -= g[:, 1:]
        return y.reshape(-1) * ((1.0 + 0.05j) if np.dtype(dtype).kind == "c" else 1.0)
    ip, ix, da = values(kind, wide(dtype))
    return sp.csr_matrix((da, ix, ip), shape=(len(ip) - 1,) * 2) @ u


def rhs_block(kind, nrhs, dtype, flip=False, seed=7):
    """(B (nrhs, n), roles): columns 0 .. nrhs - 2 are 10^-r b, the last one is zero; one column: b alone.  Roles: "scaled" columns
    share one tolerance (column 0, the unscaled copy, stops about two thirds of the way; the smaller copies earlier), "never" never
    stops, "first" stops in iteration 1 (five columns and more; with three the zero column is the one that stops there)"""
    rng = np.random.default_rng(seed)
    n = len(system(kind)[0]) - 1 if not kind.startswith("poisson") else int(kind[7:]) ** 2
    u = rng.uniform(0.5, 1.5, n)
    if np.dtype(dtype).kind == "c":
        u = u * (1.0 + 0.3j * rng.standard_normal(n))
    b = apply_matrix(kind, dtype, u)                 # b = A u: the residual norm falls from the first iteration on
    if nrhs == 1:
        return b[None, :].astype(dtype), ["b"]
    B = np.stack([b * 10.0 ** -r for r in range(nrhs - 1)] + [np.zeros_like(b)])
    roles = ["scaled"] * (nrhs - 1) + ["zero"]
    roles[1] = "never"
    if nrhs >= 5:
        roles[nrhs - 2] = "first"
    if flip:
        B, roles = B[::-1], roles[::-1]
    return np.ascontiguousarray(B).astype(dtype), roles


# ---- the rule, restated on the yardstick history ---------------------------------------------------------------------------------------
def norms_of(h):
    return np.sqrt(np.abs(h.astype(wide(h.dtype))))


def tol_between_records(norms, upto):
    """a tolerance between a record low of norms[1:upto + 1] and the record before it (>= 3 % apart): the latest such pair"""
    best, low = None, np.inf
    for j in range(1, min(upto, len(norms) - 1) + 1):
        v = norms[j]
        if not np.isfinite(v) or v == 0:
            break
        if np.isfinite(low) and v < 0.97 * low:
            best = float(np.sqrt(v * low))
        low = min(low, v)
    return best


def tolerances(H, roles, maxit):
    """one tolerance per column from the yardstick history H (maxit + 1, nrhs)"""
    N = norms_of(H)
    big = int(np.argmax(N[0]))                      # the unscaled copy: it stops last under the common tolerance
    common = tol_between_records(N[:, big], max(2, 2 * maxit // 3))
    if common is None:                              # (a system so small that CG ends at once)
        common = 2.0 * float(N[1, big]) if np.isfinite(N[1, big]) and N[1, big] > 0 else 1.0
    tol = np.full(len(roles), common)
    for r, role in enumerate(roles):
        if role == "first":
            tol[r] = 2.0 * N[1, r] if np.isfinite(N[1, r]) and N[1, r] > 0 else 1.0
        elif role == "never":
            tol[r] = 1e-200
        elif role == "zero":
            tol[r] = 1e-3
    return tol


def expected_its(H, tol, maxit):
    N = norms_of(H)
    its = np.full(H.shape[1], maxit, dtype=np.int64)
    for r in range(H.shape[1]):
        hit = np.nonzero(~(N[1:, r] >= tol[r]))[0]
        if hit.size:
            its[r] = int(hit[0]) + 1
    return its


def expected_history(H, its):
    top = int(its.max())
    E = H[:top + 1].copy()
    for r, k in enumerate(its):
        E[k + 1:, r] = H[k, r]
    return E


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def partials(pkg, s):
    """d.q partials per right-hand side of the handle's SpMV (the count alone: the output buffer is too small on purpose)"""
    per, probe = ctypes.c_int(), np.empty(1, np.complex128)
    pkg._lib.load().cgamd_solver_dot_partials(s.handle, pkg._lib.ptr(probe), 0, ctypes.byref(per))
    return per.value


def check_until(s, B, roles, maxit, tol=None, split=None, want_paths=True):
    """all the assertions of a case on the handle s; returns (its, tol)"""
    nrhs, n = B.shape
    b = B.reshape(-1)
    s.set_rhs(b)
    s.iterate(maxit)
    H, Xfull = s.history(), s.x().reshape(nrhs, n)
    assert H.shape == (maxit + 1, nrhs)
    if tol is None:
        tol = tolerances(H, roles, maxit)
    its = expected_its(H, tol, maxit)
    X = np.empty_like(Xfull)
    for k in sorted(set(its.tolist())):
        if k == maxit:
            xk = Xfull
        else:
            s.set_rhs(b)
            s.iterate(k)
            xk = s.x().reshape(nrhs, n)
        X[its == k] = xk[its == k]
    E = expected_history(H, its)
    print(f"  n={n} x {nrhs} {B.dtype.name}: maxit {maxit}, tol {np.array2string(tol, precision=3)}, expected iterations {its.tolist()}")
    if want_paths and nrhs > 1:
        assert len(set(its.tolist())) >= 2, "the case does not stop its columns in different iterations"
        assert its[roles.index("zero")] == 1 and np.all(np.isnan(X[roles.index("zero")]))
        assert "first" not in roles or its[roles.index("first")] == 1
    for ce in CHUNKS:
        s.set_rhs(b)
        got = s.iterate_until(tol, maxit, check_every=ce)
        assert got.tolist() == its.tolist(), (ce, got.tolist(), its.tolist())
        assert s.iterations_done() == int(its.max())
        x, h = s.x().reshape(nrhs, n), s.history()
        for r in range(nrhs):
            assert same(x[r], X[r]), (ce, r, "x")
        assert same(h, E), (ce, "history")
        if np.any(its < maxit):                     # a right-hand side has stopped: the columns are at different iterations
            with pytest.raises(RuntimeError, match="iterate_until"):
                s.iterate(1)
    a = split if split is not None else max(1, maxit // 3)
    s.set_rhs(b)
    first = s.iterate_until(tol, a)
    assert first.tolist() == np.minimum(its, a).tolist()
    got = s.iterate_until(tol, maxit - a)
    assert got.tolist() == its.tolist(), ("split", a, got.tolist(), its.tolist())
    assert s.iterate_until(tol, 0).tolist() == its.tolist()          # maxIterations == 0: the current counts, at once
    x, h = s.x().reshape(nrhs, n), s.history()
    for r in range(nrhs):
        assert same(x[r], X[r]), ("split", a, r)
    assert same(h, E), ("split", a)
    return its, tol


def solver(pkg, ctx, kind, dtype, nrhs, flags=0):
    ip, ix, da = values(kind, dtype)
    return pkg.Solver(ctx, len(ip) - 1, len(ix), da, ip, ix, nrhs, flags=flags), len(ip) - 1


# ---- plain CG: sizes, types, widths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 3, 9])
@pytest.mark.parametrize("dt", list(DT))
def test_poisson24_every_type_and_width(pkg, gpu, dt, nrhs):
    s, n = solver(pkg, gpu[0], "poisson24", DT[dt], nrhs)
    try:
        assert partials(pkg, s) <= 2048                       # alpha folded into the r update
        B, roles = rhs_block("poisson24", nrhs, DT[dt], flip=(nrhs == 9))
        check_until(s, B, roles, 80 if nrhs == 9 else 30)
    finally:
        s.close()


@pytest.mark.parametrize("kind,dt,nrhs,maxit", [("chain1", "f64", 3, 4), ("chain3", "f32", 3, 6), ("chain257", "f64", 5, 20),
                                                ("chain257", "c128", 1, 20), ("poisson23", "c64", 5, 24), ("poisson23", "c64", 1, 24)])
def test_tails_and_padded_rows(pkg, gpu, kind, dt, nrhs, maxit):
    """n = 1, 3, 257 and 23 x 23 = 529: scalar tails, and systems carried with empty rows appended (cgamd_solver_ld > size)"""
    s, n = solver(pkg, gpu[0], kind, DT[dt], nrhs)
    try:
        B, roles = rhs_block(kind, nrhs, DT[dt])
        check_until(s, B, roles, maxit, want_paths=n > 3)
    finally:
        s.close()


@pytest.mark.parametrize("nrhs,flip", [(1, False), (5, True)])
def test_300x300_fp64_several_work_groups(pkg, gpu, nrhs, flip):
    """90 000 rows: several work-groups per right-hand side, and a handle whose iterate() runs the chip-wide resident loop -- the
    yardstick comes from that loop, iterate_until from the launched one"""
    s, n = solver(pkg, gpu[0], "poisson300", np.float64, nrhs)
    try:
        assert pkg._lib.load().cgamd_solver_loop_launches(s.handle) == 1
        B, roles = rhs_block("poisson300", nrhs, np.float64, flip=flip)
        check_until(s, B, roles, 24)
    finally:
        s.close()


def test_as_prec_shape_16384_rows_x9_complex64(pkg, gpu):
    s, n = solver(pkg, gpu[0], "helm128", np.complex64, 9)
    try:
        B, roles = rhs_block("helm128", 9, np.complex64, flip=True)
        check_until(s, B, roles, 40)
    finally:
        s.close()


def _device_poisson(pkg, ctx, N, dtype, nrhs):
    ip, ix, da = pkg.generators.poisson2d(ctx, N, dtype=dtype)
    s = pkg.Solver(ctx, N * N, int(ix.numel()), da, ip, ix, nrhs, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
    return s, (ip, ix, da)


def test_above_the_fold_limit_cg_alpha_in_its_own_launch_borrowed_matrix(pkg, gpu):
    """740 x 740 generated on the device and borrowed (CGAMD_MATRIX_ON_DEVICE): 2140 d.q partials > kFoldAlphaMax, four launches"""
    s, keep = _device_poisson(pkg, gpu[0], 740, np.float64, 3)
    try:
        assert 2048 < partials(pkg, s) < 16384
        B, roles = rhs_block("poisson740", 3, np.float64, flip=True)
        check_until(s, B, roles, 12)
    finally:
        s.close()


def test_cg_alpha2_the_two_level_alpha_step(pkg, gpu):
    """2048 x 2048 = 4 194 304 rows, fp32: 16 384 d.q partials, the threshold of cg_alpha2 (kAlphaParts work-groups per right-hand
    side and a ticket: all of them must take the same branch)"""
    s, keep = _device_poisson(pkg, gpu[0], 2048, np.float32, 3)
    try:
        assert partials(pkg, s) >= 16384
        B, roles = rhs_block("poisson2048", 3, np.float32, flip=True)
        check_until(s, B, roles, 6, split=2)
    finally:
        s.close()


def test_no_graph(pkg, gpu):
    s, n = solver(pkg, gpu[0], "poisson24", np.float64, 5, flags=pkg._lib.NO_GRAPH)
    try:
        B, roles = rhs_block("poisson24", 5, np.float64)
        check_until(s, B, roles, 30)
    finally:
        s.close()


def test_after_iterate_calls_and_under_a_smaller_tolerance(pkg, gpu):
    """iterate(5); iterate_until(...) goes on from iteration 5 (earlier iterations are not examined again) and leaves the bits of
    fixed-count runs; a column that has stopped stays stopped when a later call brings a smaller tolerance"""
    s, n = solver(pkg, gpu[0], "poisson24", np.float64, 3)
    try:
        B, roles = rhs_block("poisson24", 3, np.float64)          # b, 0.1 b, 0
        b = B.reshape(-1)

        def x_after(k):
            s.set_rhs(b)
            s.iterate(k)
            return s.x().reshape(3, n)

        s.set_rhs(b)
        s.iterate(30)
        H, X30 = s.history(), s.x().reshape(3, n)
        t0 = tol_between_records(norms_of(H)[:, 0], 10)
        tol = np.array([t0, 1e-200, 1e-3])
        k0 = int(expected_its(H, tol, 30)[0])
        assert 5 < k0 <= 10
        s.set_rhs(b)
        s.iterate(5)
        its = s.iterate_until(tol, 25, check_every=3)
        assert its.tolist() == [k0, 30, 6]              # the zero column is NaN from iteration 1 on: the first iteration examined stops it
        x = s.x().reshape(3, n)
        assert same(x[0], x_after(k0)[0]) and same(x[1], X30[1])
        s.set_rhs(b)
        assert s.iterate_until(tol, 12).tolist() == [k0, 12, 1]
        assert s.iterate_until(tol * 1e-3, 18).tolist() == [k0, 30, 1]
        x = s.x().reshape(3, n)
        assert same(x[0], x_after(k0)[0]) and same(x[1], X30[1])
    finally:
        s.close()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "no_graph"])
@pytest.mark.parametrize("pre", [None, "jacobi"])
def test_iterate_goes_on_after_an_iterate_until_that_stopped_nothing(pkg, gpu, pre, graph):
    """set_rhs; iterate_until(tol, 7, check_every=3); iterate(9) leaves the bits of set_rhs; iterate(16) on the same handle: two
    replayed chunks and one iteration of plain guarded launches, then a plain iterate on the handle still in the three-launch loop
    iterate_until put it in (its graphs captured anew there).  Three right-hand sides that all stay active (the scaled copies, no
    zero column: that one stops by the NaN rule and the handle then refuses iterate)."""
    s, n = solver(pkg, gpu[0], "poisson24", np.float64, 3, flags=0 if graph else pkg._lib.NO_GRAPH)
    try:
        if pre is not None:
            s.set_preconditioner(pre)
        b = np.ascontiguousarray(rhs_block("poisson24", 4, np.float64)[0][:3]).reshape(-1)      # b, 0.1 b, 0.01 b
        s.set_rhs(b)
        s.iterate(16)
        X, H = s.x().copy(), s.history().copy()
        assert H.shape == (17, 3) and s.iterations_done() == 16 and np.all(np.isfinite(H))
        s.set_rhs(b)
        assert s.iterate_until(np.full(3, 1e-200), 7, check_every=3).tolist() == [7, 7, 7]
        s.iterate(9)
        assert s.iterations_done() == 16
        assert same(s.x(), X), "x"
        assert same(s.history(), H), "history"
    finally:
        s.close()


# ---- preconditioned handles --------------------------------------------------------------------------------------------------------------
def test_diagonal_pcg(pkg, gpu):
    s, n = solver(pkg, gpu[0], "poisson24", np.float64, 5)
    try:
        s.set_preconditioner(np.random.default_rng(3).uniform(0.15, 0.35, n))
        B, roles = rhs_block("poisson24", 5, np.float64, flip=True)
        check_until(s, B, roles, 30)
    finally:
        s.close()


def test_diagonal_pcg_complex64_x9_jacobi_from_the_matrix(pkg, gpu):
    s, n = solver(pkg, gpu[0], "helm24", np.complex64, 9)
    try:
        s.set_preconditioner("jacobi")
        B, roles = rhs_block("helm24", 9, np.complex64)
        check_until(s, B, roles, 30)
    finally:
        s.close()


@pytest.mark.parametrize("kind,dt,stride,launches,maxit", [("poisson24", "f64", 1, 4, 20), ("poisson24", "c64", 1, 4, 20),
                                                           ("far3000", "f64", 1, 6, 12), ("poisson24", "f64", 24, 4, 20),
                                                           ("poisson23", "c128", 23, 4, 20)])
def test_line_preconditioner_short_long_and_strided(pkg, gpu, kind, dt, stride, launches, maxit):
    """("line", 1) on 24-row grid lines (one sweep launch), on a 3 000-row chain (longer than a work-group's chunk: the three-launch
    sweep, six launches per iteration) and ("line", nx) (one thread per line)"""
    s, n = solver(pkg, gpu[0], kind, DT[dt], 5)
    try:
        s.set_preconditioner(("line", stride))
        assert pkg._lib.load().cgamd_solver_loop_launches(s.handle) == launches
        B, roles = rhs_block(kind, 5, DT[dt], flip=(dt == "f64"))
        check_until(s, B, roles, maxit)
    finally:
        s.close()


# ---- batched handles: A_r = c_r A + s_r I ------------------------------------------------------------------------------------------------
def batched_solver(pkg, ctx, dtype, flags=0):
    ip, ix, da = values("poisson24", dtype)
    n = len(ip) - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    eye = (rows == ix).astype(da.dtype)
    vals = np.concatenate([c * da + sh * eye for c, sh in ((1.0, 0.0), (1.5, 0.5), (0.7, 2.0))]).astype(dtype)
    return pkg.Solver(ctx, n, len(ix), vals, ip, ix, 3, flags=flags, batched=True), n


@pytest.mark.parametrize("pre", [None, "jacobi", ("line", 1), ("line", 24)])
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_batched_handles(pkg, gpu, dt, pre):
    s, n = batched_solver(pkg, gpu[0], DT[dt])
    try:
        s.set_preconditioner(pre)
        B, roles = rhs_block("poisson24", 3, DT[dt], flip=(pre is None))
        check_until(s, B, roles, 24)
    finally:
        s.close()


def test_solve_until_and_solve_subdomains(pkg, gpu):
    """the Python entries: solve_until on a batched handle; solve_subdomains(tol=) stops every sub-domain on its own and returns
    the counts; tol=None is the fixed-count solve, unchanged"""
    ctx = gpu[0]
    s, n = batched_solver(pkg, ctx, np.complex64)
    try:
        B, roles = rhs_block("poisson24", 3, np.complex64)
        b = B.reshape(-1)
        s.set_rhs(b)
        s.iterate(24)
        tol = tolerances(s.history(), roles, 24)
        its = expected_its(s.history(), tol, 24)
        x, got, h = s.solve_until(b, tol=tol, maxit=24)
        assert got.tolist() == its.tolist() and h.shape == (int(its.max()) + 1, 3)
    finally:
        s.close()
    ip, ix, da = values("poisson24", np.complex64)
    A = types.SimpleNamespace(indptr=ip, indices=ix, data=da)
    res = [B[0], B[1]]
    fixed = pkg.solve_subdomains(ctx, A, res, 24)
    s2 = pkg.Solver(ctx, n, len(ix), da, ip, ix, 2)
    try:
        s2.set_rhs(np.concatenate(res))
        s2.iterate(24)
        assert same(np.concatenate(fixed).astype(np.complex64), s2.x())
        t2 = tolerances(s2.history(), ["scaled", "scaled"], 24)
        want = expected_its(s2.history(), t2, 24)
        out, got = pkg.solve_subdomains(ctx, A, res, 24, tol=t2[0], return_iterations=True, solver=s2)
        assert got.tolist() == want.tolist() and want[1] < want[0]
        for p, k in enumerate(want):
            s2.set_rhs(np.concatenate(res))
            s2.iterate(int(k))
            assert same(out[p].astype(np.complex64), s2.x().reshape(2, n)[p])
    finally:
        s2.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _until_status(pkg, s, maxit, tol):
    t, its = np.asarray(tol, np.float64), np.zeros(s.n_rhs, np.intc)
    return pkg._lib.load().cgamd_solver_iterate_until(s.handle, maxit, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), t.size, 8,
                                                      its.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))


def test_row_major_and_unfused_handles_are_refused_with_their_state_intact(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    ip, ix, da = values("poisson24", np.float64)
    n = len(ip) - 1
    b = np.tile(np.linspace(1.0, 2.0, n), 16)
    L.check(lib.cgamd_tune(b"spmm_rowmajor", 2))             # fp64 x 16 keeps its right-hand sides interleaved under this knob
    try:
        rm = pkg.Solver(ctx, n, len(ix), da, ip, ix, 16)
    finally:
        L.check(lib.cgamd_tune(b"spmm_rowmajor", 1))
    un = pkg.Solver(ctx, n, len(ix), da, ip, ix, 16, flags=L.UNFUSED)
    try:
        for s, layout in ((rm, 1), (un, 0)):
            assert _until_status(pkg, s, 5, [1e-3]) == L.ERR_STATE      # no set_rhs yet
            s.set_rhs(b)
            assert lib.cgamd_solver_layout(s.handle) == layout
            s.iterate(10)
            want = (s.x().copy(), s.history().copy())
            s.set_rhs(b)
            s.iterate(4)
            assert _until_status(pkg, s, 5, [1e-3]) == L.ERR_STATE
            assert _until_status(pkg, s, 5, np.full(16, 1e-3)) == L.ERR_STATE
            assert s.iterations_done() == 4
            s.iterate(6)
            assert same(s.x(), want[0]) and same(s.history(), want[1])
    finally:
        rm.close()
        un.close()


def test_argument_checks_on_a_live_handle_and_iterate_after_a_stop(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    s, n = solver(pkg, ctx, "poisson24", np.float64, 3)
    try:
        B, roles = rhs_block("poisson24", 3, np.float64)
        b = B.reshape(-1)
        s.set_rhs(b)
        assert _until_status(pkg, s, 5, [1e-3, 1e-3]) == L.ERR_INVALID          # nTol = 2 of 3
        assert _until_status(pkg, s, 5, [1e-3, 0.0, 1e-3]) == L.ERR_INVALID
        assert _until_status(pkg, s, 5, [float("nan")]) == L.ERR_INVALID
        s.iterate(3)                                                              # the refused calls left the handle alone
        its = s.iterate_until([1e-200, 1e-200, 1e-3], 4)
        assert its.tolist() == [7, 7, 4]
        spmv_ms, iter_ms, run = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        assert lib.cgamd_solver_iterate(s.handle, 1) == L.ERR_STATE
        assert lib.cgamd_solver_iterate_timed(s.handle, 1, ctypes.byref(spmv_ms), ctypes.byref(iter_ms)) == L.ERR_STATE
        assert s.iterate_until(1e-200, 2).tolist() == [9, 9, 4]                   # iterate_until itself goes on
        s.set_rhs(b)
        assert lib.cgamd_solver_iterate(s.handle, 1) == L.OK                      # until set_rhs
        one, _ = solver(pkg, ctx, "poisson24", np.float64, 1)
        try:
            one.set_rhs(B[0])
            assert one.iterate_until(2.0 * float(np.sqrt(abs(one.history()[0, 0]))), 5).tolist() == [1]
            assert lib.cgamd_solver_iterate_tol(one.handle, 5, 1e-3, ctypes.byref(run)) == L.ERR_STATE
        finally:
            one.close()
    finally:
        s.close()


# ---- oracle cross-check: the stopping iteration only ---------------------------------------------------------------------------------
ORACLE_M = {"f32": 1e-3, "c64": 1e-3, "f64": 1e-9, "c128": 1e-9}       # ten times the delta_k tolerance test_gpu_cg grants the type


def oracle_case(kind, cplx, nrhs, maxit):
    """per column: b, a tolerance at the geometric mean of two consecutive oracle norms that the ORACLE ALONE meets with margin
    (1 + m) for the loosest m, and the iteration cg_numpy.cg_tol stops in"""
    ip, ix, da = system(kind)
    n = len(ip) - 1
    da = np.asarray(da).astype(np.complex128) if cplx or np.iscomplexobj(da) else np.asarray(da, np.float64)
    rng = np.random.default_rng(5)
    cols = []
    for r in range(nrhs):
        b = rng.uniform(0.5, 1.5, n) * 10.0 ** -r
        if np.iscomplexobj(da):
            b = b * (1.0 + 0.3j * rng.standard_normal(n))
        _, _, ho = cg_numpy.pcg_diag(ip, ix, da, b.astype(complex), None, tol=0.0, maxit=maxit, history=True)
        no = np.sqrt(np.abs(ho))
        pick = None
        for k in range(maxit - 2 - 3 * r, 1, -1):            # later columns stop earlier
            tol = np.sqrt(no[k] * no[k - 1])
            if np.all(no[1:k] > tol * 1.01) and no[k] < tol / 1.01:
                pick = (k, tol)
                break
        assert pick, (kind, r)
        _, it = cg_numpy.cg_tol(ip, ix, da, b.astype(complex), tol=pick[1])
        assert it == pick[0]
        cols.append((b, pick[1], it))
    return ip, ix, da, cols


@pytest.mark.parametrize("kind,maxit,dt", [("poisson24", 40, "f32"), ("poisson24", 40, "f64"), ("poisson24", 40, "c64"),
                                           ("poisson24", 40, "c128"), ("helm64", 40, "c64"), ("helm64", 40, "c128")])
def test_stopping_iteration_against_the_numpy_oracle(pkg, gpu, kind, maxit, dt):
    dtype = DT[dt]
    ip, ix, da, cols = oracle_case(kind, np.dtype(dtype).kind == "c", 3, maxit)
    m = ORACLE_M[dt]
    for b, tol, it in cols:                                   # the condition, on the oracle alone
        _, _, ho = cg_numpy.pcg_diag(ip, ix, da, b.astype(complex), None, tol=0.0, maxit=it, history=True)
        no = np.sqrt(np.abs(ho))
        assert np.all(no[1:it] > tol * (1 + m)) and no[it] < tol / (1 + m)
    s = pkg.Solver(gpu[0], len(ip) - 1, len(ix), da.astype(dtype), ip, ix, 3)
    try:
        s.set_rhs(np.concatenate([c[0] for c in cols]).astype(dtype))
        its = s.iterate_until([c[1] for c in cols], maxit)
        assert its.tolist() == [c[2] for c in cols]
    finally:
        s.close()
