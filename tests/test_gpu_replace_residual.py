"""cgamd_solver_replace_residual / Solver.replace_residual: a running handle takes a new residual and keeps its search direction.

The system is the 5-point Poisson matrix on 33 x 29: 957 rows, which are no whole number of 16-byte packs in fp32 (960), fp64 and
complex64 (958), so those handles carry padding rows (a complex128 value is a pack of its own: 957).  The complex types run it times
(1 + 0.05i), complex symmetric.

"d stays as it is" is checked bit for bit.  A handle that has just iterated on its two-launch or a resident loop (this small system
without a preconditioner) holds the direction of its last iteration in the other of its two buffers and leaves d = beta d + r to the
next SpMV launch; the entry completes that step with the old residual, as cgamd_solver_iterate_until does, into the one buffer the
launched loop keeps.  The test tells the two cases apart by the address cgamd_solver_vector(2) names before and after the call (7
iterations: an odd count, so the addresses differ exactly when that step was still owed) and expects either the snapshot itself or
beta * snapshot + r_old, formed on the host with one rounding per operation as the kernel forms it."""
import numpy as np
import pytest

import mixed_ref

pytestmark = pytest.mark.gpu

NX, NY = 33, 29
N = NX * NY
DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}


def wide(dtype):
    return np.dtype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64)


_CSR = mixed_ref.poisson2d_rect(NX, NY)


def matrix(dtype):
    ip, ix, da = _CSR
    if np.dtype(dtype).kind == "c":
        da = da * (1.0 + 0.05j)
    return ip, ix, da.astype(dtype)


def block(seed, nrhs, dtype, scale=1.0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((nrhs, N))
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal((nrhs, N))
    return np.ascontiguousarray(scale * v).astype(dtype)


def make(pkg, ctx, dtype, nrhs, pre=False, flags=0, **kw):
    ip, ix, da = matrix(dtype)
    s = pkg.Solver(ctx, N, len(da), da, ip, ix, nrhs, flags=flags, **kw)
    if pre:
        s.set_preconditioner("jacobi")
    return s


def read(pkg, ctx, s, which):
    """one of the handle's vectors as (n_rhs, ld), padding rows included"""
    ctx.synchronize()
    out = np.empty((s.n_rhs, s.ld), dtype=s.dtype)
    pkg._lib.check(pkg._lib.load().cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), pkg._lib.ptr(int(s.vector(which))), out.nbytes))
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def aypx_host(beta, d, r):
    """beta[r] * d + r with one rounding per operation in the handle's type; complex: (a.x y.x - a.y y.y, a.x y.y + a.y y.x)"""
    if d.dtype.kind != "c":
        return beta[:, None] * d + r
    real = np.float32 if d.dtype == np.complex64 else np.float64
    ax, ay = beta.real.astype(real)[:, None], beta.imag.astype(real)[:, None]
    yx, yy = d.real.astype(real), d.imag.astype(real)
    out = np.empty_like(d)
    out.real = (ax * yx - ay * yy) + r.real
    out.imag = (ax * yy + ay * yx) + r.imag
    return out


CASES = [(t, nrhs, pre) for t in DT for nrhs in (1, 3) for pre in (False, True)]
IDS = [f"{t}-x{nrhs}-{'jacobi' if pre else 'plain'}" for t, nrhs, pre in CASES]


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def replaced(request, pkg, gpu):
    """set_rhs(b); iterate(7); replace_residual(r_new) -- with everything the tests below compare, read once"""
    ctx = gpu[0]
    t, nrhs, pre = request.param
    dtype = np.dtype(DT[t])
    s = make(pkg, ctx, dtype, nrhs, pre)
    b, r_new = block(3, nrhs, dtype), block(11, nrhs, dtype, 1e-3)
    s.set_rhs(b.reshape(-1))
    s.iterate(7)
    at0, d0, r0, beta = int(s.vector("d")), read(pkg, ctx, s, "d"), read(pkg, ctx, s, "r"), s.step_state("beta")
    buf = pkg.DeviceBuffer(ctx, hostbuf=r_new.reshape(-1))
    s.replace_residual(buf)
    ctx.synchronize()
    buf.release()
    fresh = make(pkg, ctx, dtype, nrhs, pre)
    fresh.set_rhs(r_new.reshape(-1))
    out = dict(s=s, dtype=dtype, nrhs=nrhs, pre=pre, r_new=r_new, at0=at0, d0=d0, r0=r0, beta=beta, at1=int(s.vector("d")),
               x=read(pkg, ctx, s, "x"), r=read(pkg, ctx, s, "r"), d=read(pkg, ctx, s, "d"), iters=s.iterations_done(), hist=s.history(),
               delta=s.step_state("delta"), fresh_hist=fresh.history(), fresh_delta=fresh.step_state("delta"))
    fresh.close()
    yield out
    s.close()


def test_state_after_the_call_bit_for_bit(replaced):
    c = replaced
    assert not c["x"].any() and same_bits(c["x"], np.zeros_like(c["x"]))
    assert same_bits(np.ascontiguousarray(c["r"][:, :N]), c["r_new"])
    per_pack = 16 // c["dtype"].itemsize                             # 957 rows: 960 in fp32, 958 in fp64 / complex64, 957 in complex128
    assert c["r"].shape[1] == -(-N // per_pack) * per_pack and not c["r"][:, N:].any()
    if c["at1"] == c["at0"]:
        assert same_bits(c["d"], c["d0"])
    else:       # the two-launch convention: d = beta d + r of the last iteration was still owed (module docstring)
        assert same_bits(c["d"], aypx_host(c["beta"], c["d0"], c["r0"]))
    assert c["iters"] == 0
    assert c["hist"].shape == (1, c["nrhs"]) and same_bits(c["hist"], c["fresh_hist"][:1])
    assert same_bits(c["delta"], c["fresh_delta"])


def test_the_recurrence_continues_from_the_kept_direction(pkg, gpu, replaced):
    """10 more iterations against a numpy continuation from (0, r_new, d read back) in the wide type.  Tolerances: the project's own
    (SURVEY 8c): fp64 / complex128 delta_k rtol 1e-10 and x rel 1e-9; fp32 / complex64 delta_k rtol 1e-4"""
    c, ctx = replaced, gpu[0]
    s, w = c["s"], wide(c["dtype"])
    s.iterate(10)
    hist, x = s.history(), s.x().reshape(c["nrhs"], N)
    ip, ix, da = matrix(c["dtype"])
    da = da.astype(w)
    diag = da[[int(np.nonzero(ix[ip[i]:ip[i + 1]] == i)[0][0]) + ip[i] for i in range(N)]]
    m = (1.0 / diag).astype(c["dtype"]).astype(w) if c["pre"] else None
    narrow = c["dtype"] in (np.dtype(np.float32), np.dtype(np.complex64))
    for k in range(c["nrhs"]):
        r, d, xs = c["r_new"][k].astype(w), c["d"][k, :N].astype(w), np.zeros(N, w)
        z = r if m is None else m * r
        rho, want = np.sum(r * z), [np.sum(r * r)]
        for _ in range(10):
            q = mixed_ref.csr_matvec(ip, ix, da, d)
            alpha = rho / np.sum(d * q)
            xs, r = xs + alpha * d, r - alpha * q
            z = r if m is None else m * r
            rho_new = np.sum(r * z)
            want.append(np.sum(r * r))
            d, rho = z + (rho_new / rho) * d, rho_new
        np.testing.assert_allclose(hist[:, k].astype(w), np.array(want), rtol=1e-4 if narrow else 1e-10)
        if not narrow:
            assert np.linalg.norm(x[k] - xs) <= 1e-9 * np.linalg.norm(xs)


@pytest.mark.parametrize("t", sorted(DT))
def test_the_stop_record_is_cleared(pkg, gpu, t):
    ctx = gpu[0]
    dtype = np.dtype(DT[t])
    s = make(pkg, ctx, dtype, 3)
    b = block(3, 3, dtype)
    s.set_rhs(b.reshape(-1))
    its = s.iterate_until(1e30, 50)                 # every column stops in its first iteration
    assert its.tolist() == [1, 1, 1]
    with pytest.raises(pkg.CgAmdError) as e:
        s.iterate(1)
    assert e.value.status == pkg._lib.ERR_STATE
    s.replace_residual(block(11, 3, dtype).reshape(-1))
    its = s.iterate_until(1e-30, 5)
    assert its.tolist() == [5, 5, 5] and s.iterations_done() == 5
    s.iterate_until(1e30, 5)
    s.replace_residual(block(12, 3, dtype).reshape(-1))
    s.iterate(2)                                    # returns OK again
    assert s.iterations_done() == 2 and s.history().shape == (3, 3)
    s.close()


def _refused(pkg, ctx, s, b, status):
    """the call is refused with `status`, x and the history keep their bits"""
    x0, h0 = s.x(), s.history()
    buf = pkg.DeviceBuffer(ctx, hostbuf=b.reshape(-1))
    with pytest.raises(pkg.CgAmdError) as e:
        s.replace_residual(buf)
    assert e.value.status == status
    assert same_bits(s.x(), x0) and same_bits(s.history(), h0)
    buf.release()


def test_refusals_leave_the_handle_untouched(pkg, gpu):
    ctx, L = gpu[0], pkg._lib
    lib = L.load()
    # a tridiagonal (line) preconditioner
    s = make(pkg, ctx, np.float64, 1)
    s.set_preconditioner(("line", 1))
    s.set_rhs(block(3, 1, np.float64).reshape(-1))
    s.iterate(3)
    _refused(pkg, ctx, s, block(11, 1, np.float64), L.ERR_STATE)
    s.close()
    # CGAMD_HERMITIAN on a complex type (the real Poisson matrix is Hermitian positive definite)
    ip, ix, da = _CSR
    s = pkg.Solver(ctx, N, len(da), da.astype(np.complex64), ip, ix, 1, hermitian=True)
    assert s.hermitian == 1
    s.set_rhs(block(3, 1, np.complex64).reshape(-1))
    s.iterate(3)
    _refused(pkg, ctx, s, block(11, 1, np.complex64), L.ERR_STATE)
    s.close()
    # a batched handle
    s = pkg.Solver(ctx, N, len(da), np.concatenate([da, 1.5 * da]), ip, ix, 2, batched=True)
    s.set_rhs(block(3, 2, np.float64).reshape(-1))
    s.iterate(3)
    _refused(pkg, ctx, s, block(11, 2, np.float64), L.ERR_STATE)
    s.close()
    # CGAMD_UNFUSED
    s = make(pkg, ctx, np.float32, 1, flags=L.UNFUSED)
    s.set_rhs(block(3, 1, np.float32).reshape(-1))
    s.iterate(3)
    _refused(pkg, ctx, s, block(11, 1, np.float32), L.ERR_STATE)
    s.close()
    # 16 right-hand sides in fp64, kept row-major (the layout is taken for every supported width with spmm_rowmajor = 2)
    L.check(lib.cgamd_tune(b"spmm_rowmajor", 2))
    try:
        s = make(pkg, ctx, np.float64, 16)
    finally:
        L.check(lib.cgamd_tune(b"spmm_rowmajor", 1))
    s.set_rhs(block(3, 16, np.float64).reshape(-1))
    assert lib.cgamd_solver_layout(s.handle) == 1
    s.iterate(3)
    _refused(pkg, ctx, s, block(11, 16, np.float64), L.ERR_STATE)
    s.close()
    # before set_rhs
    s = make(pkg, ctx, np.float64, 1)
    buf = pkg.DeviceBuffer(ctx, hostbuf=block(11, 1, np.float64).reshape(-1))
    with pytest.raises(pkg.CgAmdError) as e:
        s.replace_residual(buf)
    assert e.value.status == L.ERR_STATE
    # NULL
    s.set_rhs(block(3, 1, np.float64).reshape(-1))
    with pytest.raises(pkg.CgAmdError) as e:
        s.replace_residual(None)
    assert e.value.status == L.ERR_INVALID
    assert lib.cgamd_solver_replace_residual(None, L.ptr(buf)) == L.ERR_INVALID
    buf.release()
    s.close()
