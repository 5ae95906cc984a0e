"""MixedSolver / cgamd_mixed_solve: the CG recurrence in float32 / complex64, x and the true residual in float64 / complex128, joined by
residual replacement with the search direction kept.

Every claim is checked on the HOST's residual r = b - A x in the wide type.  b is standard normal with seed 3 and tol = 1e-10 sqrt|b.b|.
The slack of a comparison is the rounding bound of one residual evaluation, || 8 eps (|A| |x| + |b|) ||_2 -- rows of at most 7 entries,
each product and each sum within eps: derived here, not chosen.

The iteration caps (1.3 x the fp64 handle's count; 2.0 x for the complex Helmholtz system) are conditions, not measurements: they keep a
broken replacement -- one that loses the direction and so restarts the Krylov space -- from passing as "converged eventually".  The
numpy restatement (tests/mixed_ref.py) gives 1.00 - 1.17 and 1.53 - 1.61 on these inputs.

The second half pins the solve's bookkeeping, which a self-correcting scheme hides from a residual check: the mask and the freeze
(columns that finish segments apart), columns done at the start, a non-finite column, one segment against the accumulate rule, and
the segment cap with the budget.  The kernels themselves are held bit for bit in tests/test_gpu_mixed_kernels.py."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import mixed_kernel_ref
import mixed_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SYSTEMS = {"33x29": (33, 29), "64x64": (64, 64), "40x30x20": (40, 30, 20)}
_CSR = {}


def system(name):
    if name not in _CSR:
        _CSR[name] = mixed_ref._stencil(SYSTEMS[name])
    return _CSR[name]


def rhs(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)


def udot_norm(v):
    """sqrt|v.v|, the unconjugated measure of the stop"""
    return float(np.sqrt(abs(np.sum(v * v))))


def host_residual(csr, b, x):
    """(sqrt|r.r| of r = b - A x on the host, the rounding bound of that evaluation)"""
    ip, ix, da = csr
    A = sp.csr_matrix((da, ix, ip), shape=(len(ip) - 1,) * 2)
    r = b - A @ x
    slack = float(np.linalg.norm(8 * EPS * (abs(A) @ np.abs(x) + np.abs(b))))
    return udot_norm(r), slack


def mixed(pkg, ctx, csr, nrhs=1, **kw):
    ip, ix, da = csr
    return pkg.MixedSolver(ctx, len(ip) - 1, len(da), da, ip, ix, nrhs, **kw)


def hi_count(pkg, ctx, csr, b, tol, pre=None, maxit=4000):
    """iterations of a handle of the wide type, stopped on the device at the same tolerance"""
    ip, ix, da = csr
    s = pkg.Solver(ctx, len(ip) - 1, len(da), da, ip, ix, 1)
    if pre is not None:
        s.set_preconditioner(pre)
    _, its, _ = s.solve_until(b, tol=tol, maxit=maxit)
    s.close()
    return int(its[0])


@pytest.fixture(scope="module", params=sorted(SYSTEMS))
def solved(request, pkg, gpu):
    """one mixed solve and one fp64 solve per system, shared by the tests below"""
    ctx = gpu[0]
    csr = system(request.param)
    n = len(csr[0]) - 1
    b = rhs(n)
    tol = 1e-10 * udot_norm(b)
    m = mixed(pkg, ctx, csr)
    x, info = m.solve(b, tol=tol, maxit=4000)
    m.close()
    return dict(name=request.param, csr=csr, b=b, tol=tol, x=x, info=info, k64=hi_count(pkg, ctx, csr, b, tol))


def test_reaches_the_tolerance_on_the_true_residual(solved):
    c = solved
    res, slack = host_residual(c["csr"], c["b"], c["x"])
    print(f"  {c['name']}: host residual {res:.3e} tol {c['tol']:.3e} slack {slack:.1e} resnorm {c['info'].resnorm[0]:.3e} "
          f"iterations {c['info'].iterations[0]} replacements {c['info'].replacements} fp64 {c['k64']}")
    assert c["info"].status.tolist() == [0]
    assert res <= c["tol"] + slack
    assert abs(c["info"].resnorm[0] - res) <= slack


def test_fp32_alone_stalls(pkg, gpu):
    """what the feature is for: the float32 handle with the same tolerance ends far above it (the host's run: >= 2.9e-6 ||b||)"""
    ctx = gpu[0]
    ip, ix, da = csr = system("33x29")
    b = rhs(len(ip) - 1)
    tol = 1e-10 * udot_norm(b)
    s = pkg.Solver(ctx, len(ip) - 1, len(da), da.astype(np.float32), ip, ix, 1)
    x, its, _ = s.solve_until(b.astype(np.float32), tol=tol, maxit=600)
    s.close()
    res, _ = host_residual(csr, b, x.astype(np.float64))
    assert res > 100 * tol, (res, tol, its)


def test_iteration_cap(solved):
    c = solved
    assert int(c["info"].iterations[0]) <= 1.3 * c["k64"], (c["name"], c["info"], c["k64"])


def test_iteration_cap_with_jacobi_on_a_rescaled_matrix(pkg, gpu):
    """64 x 64 rescaled by a random positive diagonal, D A D: Jacobi on the inner handle (and on the fp64 handle it is held against)"""
    ctx = gpu[0]
    ip, ix, da = system("64x64")
    n = len(ip) - 1
    dg = np.exp(np.random.default_rng(5).uniform(-1.5, 1.5, n))
    A = sp.csr_matrix((da, ix, ip), shape=(n, n))
    S = (sp.diags(dg) @ A @ sp.diags(dg)).tocsr()
    S.sort_indices()
    csr = (S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))
    b = rhs(n)
    tol = 1e-10 * udot_norm(b)
    m = mixed(pkg, ctx, csr)
    m.inner.set_preconditioner("jacobi")
    x, info = m.solve(b, tol=tol, maxit=6000)
    m.close()
    k64 = hi_count(pkg, ctx, csr, b, tol, pre="jacobi", maxit=6000)
    res, slack = host_residual(csr, b, x)
    print(f"  jacobi: iterations {info.iterations[0]} replacements {info.replacements} fp64 {k64} residual {res:.3e} tol {tol:.3e}")
    assert info.status.tolist() == [0] and res <= tol + slack
    assert int(info.iterations[0]) <= 1.3 * k64, (info, k64)


def test_scales_per_right_hand_side(pkg, gpu):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    B = np.stack([b, 1.3 * 2.0 ** 20 * b, 0.7 * 2.0 ** -20 * b])
    norms = np.array([np.linalg.norm(v) for v in B])
    frac = np.log2(norms) - np.floor(np.log2(norms))
    assert np.all((frac > 1e-6) & (frac < 1 - 1e-6)), "a column's norm is a power of two within 1e-6: the expected scale would hang on rounding"
    tol = np.array([1e-10 * udot_norm(v) for v in B])
    m = mixed(pkg, ctx, csr, nrhs=3)
    x, info = m.solve(B.reshape(-1), tol=tol, maxit=4000)
    m.close()
    assert info.status.tolist() == [0, 0, 0]
    for k in range(3):
        res, slack = host_residual(csr, B[k], x.reshape(3, n)[k])
        assert res <= tol[k] + slack and abs(info.resnorm[k] - res) <= slack, (k, res, tol[k], slack)
    assert info.scales.tolist() == [2.0 ** np.floor(np.log2(v)) for v in norms]      # x0 = 0: the first residual is b


def test_bits_do_not_depend_on_the_run_or_on_check_every(pkg, gpu):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    B = np.stack([rhs(n), rhs(n, 4) * 1e3])
    tol = np.array([1e-10 * udot_norm(v) for v in B])
    m = mixed(pkg, ctx, csr, nrhs=2)
    runs = [m.solve(B.reshape(-1), tol=tol, maxit=4000, check_every=ce) for ce in (8, 8, 3)]
    m.close()
    x0, i0 = runs[0]
    assert i0.status.tolist() == [0, 0]
    for x, info in runs[1:]:
        assert x.tobytes() == x0.tobytes()
        assert info.iterations.tolist() == i0.iterations.tolist() and info.replacements == i0.replacements
        assert info.resnorm.tobytes() == i0.resnorm.tobytes()


def test_initial_guess(pkg, gpu):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    tol = 1e-10 * udot_norm(b)
    m = mixed(pkg, ctx, csr)
    guess = np.random.default_rng(8).standard_normal(n)
    x, info = m.solve(b, x0=guess, tol=tol, maxit=4000)
    res, slack = host_residual(csr, b, x)
    assert info.status.tolist() == [0] and res <= tol + slack and info.iterations[0] > 0
    # a guess that already meets the tolerance comes back as it is
    x2, info2 = m.solve(b, x0=x, tol=2 * (tol + slack), maxit=4000)
    m.close()
    assert info2.status.tolist() == [0] and info2.iterations.tolist() == [0] and info2.replacements == 0
    assert x2.tobytes() == x.tobytes()


def test_complex_helmholtz_from_the_device_generator(pkg, gpu):
    """helm_fe_var(32, omega 12, rho 0.15) in complex128, generated on the device and borrowed (MATRIX_ON_DEVICE), b = rhsA(32, 12)"""
    ctx, L = gpu[0], pkg._lib
    N = 32
    indptr, indices, data = pkg.generators.helm_fe_var(ctx, N, 12.0, None, 0.15, dtype=np.complex128)
    b = pkg.generators.rhsA(ctx, N, 12.0, dtype=np.complex128).cpu().numpy()
    csr = (indptr.cpu().numpy(), indices.cpu().numpy(), data.cpu().numpy())
    n, nnz = N * N, int(data.numel())
    tol = 1e-10 * udot_norm(b)
    m = pkg.MixedSolver(ctx, n, nnz, data, indptr, indices, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.complex128)
    assert m.inner.dtype == np.complex64 and m.outer.dtype == np.complex128
    x, info = m.solve(b, tol=tol, maxit=4000)
    m.close()
    s = pkg.Solver(ctx, n, nnz, data, indptr, indices, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.complex128)
    _, its, _ = s.solve_until(b, tol=tol, maxit=4000)
    s.close()
    res, slack = host_residual(csr, b, x)
    print(f"  helm_fe_var(32): iterations {info.iterations[0]} replacements {info.replacements} complex128 {int(its[0])} residual {res:.3e} tol {tol:.3e}")
    assert info.status.tolist() == [0] and res <= tol + slack and abs(info.resnorm[0] - res) <= slack
    assert int(info.iterations[0]) <= 2.0 * int(its[0]), (info, its)


def test_budget(pkg, gpu):
    ctx = gpu[0]
    csr = system("64x64")
    n = len(csr[0]) - 1
    b = rhs(n)
    m = mixed(pkg, ctx, csr)
    x, info = m.solve(b, tol=1e-10 * udot_norm(b), maxit=20)
    m.close()
    res, slack = host_residual(csr, b, x)
    assert info.status.tolist() == [1] and int(info.iterations[0]) <= 20
    assert np.all(np.isfinite(x)) and abs(info.resnorm[0] - res) <= slack


# ---- the solve's bookkeeping: masks, frozen columns, segments and the budget (33 x 29, b of seed 3) -------------------------------------
def check_column(csr, b, x, tol, info, k):
    """the host residual check of this file on column k"""
    res, slack = host_residual(csr, b, x)
    assert info.status[k] == 0 and res <= tol + slack and abs(info.resnorm[k] - res) <= slack, (k, info, res, tol, slack)


def test_columns_that_finish_segments_apart_keep_the_bits_of_their_own_solve(pkg, gpu):
    """V: the same b in three columns with tolerances 1e-10, 1e-4, 1e-7 ||b||; U_k: tolerance k in all three.  A stopped column is
    frozen at its stopping iteration, a finished one is masked out of the accumulation, and a segment's threshold depends on the
    column's own history only: column k of V is column k of U_k, in every bit"""
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    B = np.tile(b, 3)
    tols = np.array([1e-10, 1e-4, 1e-7]) * udot_norm(b)
    m = mixed(pkg, ctx, csr, nrhs=3)
    xv, V = m.solve(B, tol=tols, maxit=4000)
    # the header's step 4 on V's last segment, read from the inner handle (maxit 0: the counts as they stand): the two columns that
    # were finished before it stopped after one iteration, the open one ran on
    last = m.inner.iterate_until(1.0, 0)
    print(f"  the inner handle's counts of V's last segment: {last.tolist()}")
    assert last[1] == 1 and last[2] == 1 and last[0] > 1 and last[0] == m.inner.iterations_done()
    U = [m.solve(B, tol=np.full(3, t), maxit=4000) for t in tols]
    m.close()
    print(f"  V: {V}")
    for k, (_, u) in enumerate(U):
        print(f"  U_{k}: {u}")
    # not vacuous: the columns of V finish in different segments, so the mask of its later accumulations is partly clear
    assert len(set(V.iterations.tolist())) == 3, V
    assert V.replacements > U[1][1].replacements, (V, U[1][1])
    xv = xv.reshape(3, n)
    for k, (xu, u) in enumerate(U):
        xu = xu.reshape(3, n)
        assert xv[k].tobytes() == xu[k].tobytes(), k
        assert V.iterations[k] == u.iterations[k] and V.status[k] == u.status[k] == 0 and V.scales[k] == u.scales[k], (k, V, u)
        assert V.resnorm[k:k + 1].tobytes() == u.resnorm[k:k + 1].tobytes(), (k, V, u)
        check_column(csr, b, xv[k], tols[k], V, k)


def test_columns_done_at_the_start_beside_an_open_one(pkg, gpu):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    tol = 1e-10 * udot_norm(b)
    m1 = mixed(pkg, ctx, csr)
    solved_x, info1 = m1.solve(b, tol=tol, maxit=4000)
    m1.close()
    _, slack = host_residual(csr, b, solved_x)
    assert info1.status.tolist() == [0]
    B = np.stack([b, np.zeros(n), b])
    X0 = np.stack([np.zeros(n), np.zeros(n), solved_x])
    tols = np.array([tol, tol, 2 * (tol + slack)])
    m = mixed(pkg, ctx, csr, nrhs=3)
    x, info = m.solve(B.reshape(-1), x0=X0.reshape(-1), tol=tols, maxit=4000)
    m.close()
    print(f"  {info}")
    x = x.reshape(3, n)
    assert info.status.tolist() == [0, 0, 0] and info.iterations[1] == 0 and info.iterations[2] == 0 and info.iterations[0] > 0
    assert x[1].tobytes() == X0[1].tobytes() and x[2].tobytes() == X0[2].tobytes()
    assert info.resnorm[1] == 0.0
    check_column(csr, b, x[0], tol, info, 0)


def test_a_non_finite_column_beside_converging_ones(pkg, gpu):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    B = np.stack([rhs(n), rhs(n), rhs(n, 4)])
    B[1, 311] = np.inf
    X0 = np.stack([np.zeros(n), np.random.default_rng(8).standard_normal(n), np.zeros(n)])
    tols = np.array([1e-10 * udot_norm(B[0]), 1e-10 * udot_norm(B[0]), 1e-10 * udot_norm(B[2])])
    m = mixed(pkg, ctx, csr, nrhs=3)
    x, info = m.solve(B.reshape(-1), x0=X0.reshape(-1), tol=tols, maxit=4000)
    m.close()
    print(f"  {info}")
    x = x.reshape(3, n)
    assert info.status.tolist() == [0, 2, 0] and info.iterations[1] == 0 and not np.isfinite(info.resnorm[1])
    assert x[1].tobytes() == X0[1].tobytes()
    for k in (0, 2):
        check_column(csr, B[k], x[k], tols[k], info, k)


def one_segment(pkg, m, n, nrhs, b, x0, tol):
    """maxit = 5 and delta = 1e-30: one segment, which ends at its cap.  What the solve returns is then x0 with the inner handle's x
    added by the rule of the accumulate kernel (tests/mixed_kernel_ref.py), on the real lanes, in every bit"""
    x, info = m.solve(b, x0=x0, tol=tol, maxit=5, delta=1e-30)
    assert info.replacements == 1 and info.iterations.tolist() == [5] * nrhs and info.status.tolist() == [1] * nrhs, info
    x_lo = m.inner.x()
    assert x_lo.dtype == (np.complex64 if x.dtype.kind == "c" else np.float32) and np.all(np.isfinite(x_lo.view(np.float32))) and np.any(x_lo != 0)
    lanes = lambda a, t: np.ascontiguousarray(a).view(t).reshape(nrhs, -1)
    want = mixed_kernel_ref.accumulate(lanes(np.asarray(x0, dtype=x.dtype), np.float64), lanes(x_lo, np.float32), info.scales, [1] * nrhs)
    assert lanes(x, np.float64).tobytes() == want.tobytes(), info
    assert x.tobytes() != np.asarray(x0, dtype=x.dtype).tobytes()


@pytest.mark.parametrize("nrhs", [1, 3])
def test_one_segment_is_x0_plus_the_scaled_inner_x(pkg, gpu, nrhs):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    B = np.concatenate([b * f for f in (1.0, 2.0 ** 11 * 1.1, 2.0 ** -9 * 0.9)[:nrhs]])
    x0 = np.random.default_rng(11).standard_normal(n * nrhs)
    m = mixed(pkg, ctx, csr, nrhs=nrhs)
    one_segment(pkg, m, n, nrhs, B, x0, 1e-10 * udot_norm(b) * 2.0 ** -9)
    m.close()


def test_one_segment_complex(pkg, gpu):
    """the same on helm_fe_var(16) in complex128"""
    ctx, L = gpu[0], pkg._lib
    N = 16
    indptr, indices, data = pkg.generators.helm_fe_var(ctx, N, 12.0, None, 0.15, dtype=np.complex128)
    b = pkg.generators.rhsA(ctx, N, 12.0, dtype=np.complex128).cpu().numpy()
    rng = np.random.default_rng(12)
    x0 = 1e-3 * (rng.standard_normal(N * N) + 1j * rng.standard_normal(N * N))
    m = pkg.MixedSolver(ctx, N * N, int(data.numel()), data, indptr, indices, 1, flags=L.MATRIX_ON_DEVICE, dtype=np.complex128)
    one_segment(pkg, m, N * N, 1, b, x0, 1e-12 * udot_norm(b))
    m.close()


def test_segments_and_the_budget(pkg, gpu):
    """delta = 1e-30 and a tolerance out of reach: a segment ends only at its cap.  max_segment = 7 and maxit = 40: segments of
    7, 7, 7, 7, 7 and 5 iterations -- the budget is the sum of the inner handle's counts"""
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    m = mixed(pkg, ctx, csr)
    runs = [m.solve(b, tol=1e-30 * udot_norm(b), maxit=40, delta=1e-30, max_segment=7, check_every=ce) for ce in (1, 3, 8)]
    m.close()
    x, info = runs[0]
    print(f"  {info}")
    assert info.status.tolist() == [1] and info.iterations.tolist() == [40] and info.replacements == -(-40 // 7)
    res, slack = host_residual(csr, b, x)
    assert abs(info.resnorm[0] - res) <= slack, (info, res, slack)
    for x2, i2 in runs[1:]:
        assert x2.tobytes() == x.tobytes() and i2.resnorm.tobytes() == info.resnorm.tobytes()
        assert i2.iterations.tolist() == [40] and i2.replacements == info.replacements and i2.status.tolist() == [1]


def test_a_line_preconditioner_on_the_inner_handle_is_refused(pkg, gpu):
    ctx = gpu[0]
    csr = system("33x29")
    n = len(csr[0]) - 1
    b = rhs(n)
    m = mixed(pkg, ctx, csr)
    m.inner.set_preconditioner(("line", 1))
    lib = pkg._lib.load()
    x = np.full(n, 0.25)
    keep = x.copy()
    import ctypes
    tol, its, st, res, repl = np.array([1e-8]), np.zeros(1, np.intc), np.zeros(1, np.intc), np.zeros(1), ctypes.c_int(0)
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rc = lib.cgamd_mixed_solve(m.handle, pkg._lib.ptr(b), pkg._lib.ptr(x), 0, tol.ctypes.data_as(pd), 1, 100, 0.1, 0, 8, its.ctypes.data_as(pi),
                               res.ctypes.data_as(pd), st.ctypes.data_as(pi), ctypes.byref(repl))
    assert rc == pkg._lib.ERR_STATE and b"replace_residual" in lib.cgamd_last_error()
    assert x.tobytes() == keep.tobytes()
    with pytest.raises(pkg.CgAmdError) as e:
        m.solve(b, tol=1e-8)
    assert e.value.status == pkg._lib.ERR_STATE
    m.inner.set_preconditioner(None)                # and the handle serves again
    x, info = m.solve(b, tol=1e-8 * udot_norm(b), maxit=2000)
    m.close()
    assert info.status.tolist() == [0]


def test_cli_mixed(pkg, gpu, tmp_path):
    """oclcgex --double --mixed --tol T on a small symmetric Matrix-Market file prints a true residual below T ||b||"""
    ip, ix, da = mixed_ref.poisson2d_rect(13, 11)
    n = len(ip) - 1
    A = sp.csr_matrix((da, ix, ip), shape=(n, n))
    low = sp.tril(A).tocoo()
    p = str(tmp_path / "poisson13x11.mtx")
    pkg.mmio.mmwrite(p, n, low.row, low.col, low.data, "real", "symmetric")
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "oclcgex")
    T = 1e-10
    r = subprocess.run([exe, p, "2", "0", "500", "--double", "--mixed", "--tol", str(T)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("rhs ")]
    assert len(lines) == 2 and any(ln.startswith("replacements ") for ln in r.stdout.splitlines())
    for k, w in enumerate(lines):           # rhs R: iterations I status S true residual E tolerance E
        its, status, res, tol = int(w[3]), int(w[5]), float(w[8]), float(w[10])
        assert status == 0 and its > 0 and res < T * 5.0 * (k + 1) * np.sqrt(n) * (1 + 1e-12) and tol == pytest.approx(T * 5.0 * (k + 1) * np.sqrt(n))
