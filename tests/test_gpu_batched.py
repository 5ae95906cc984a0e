"""The batched handle on the GPU (cgamd_solver_create_batched, csrc/batched.hip): nSystems matrices on one pattern, right-hand side r
solved with matrix r.

Systems on one pattern are made by symmetric scaling, a_r[j] = a[j] * s[row(j)] * s[col(j)] with s drawn per system from
uniform(0.8, 1.25): symmetry and the pattern stay, and delta_k of two such systems differs by 1-5 % from k = 1 on, far outside
every tolerance below -- a kernel that reads the wrong system's values cannot pass.

Tolerances are the project's (tests/test_gpu_cg.py), over k while delta_k / delta_0 > 1e-4:
  * fp64 / complex128 against the C oracle (oracle/cg_oracle, sequential sums, one system at a time): delta_k rtol 1e-10 for
    k <= 40, ||x - x_o|| / ||x_o|| < 1e-8 after 50 iterations;
  * fp32 / complex64 against the oracle in the wide type: delta_k rtol 1e-4 for k <= 30.  The cap of 30 comes from the reference alone:
    the oracle run in the narrow type against itself in the wide type on these inputs (seeds 100-108) stays at or below 2.6e-6 (fp32)
    and 1.5e-5 (complex64) up to k = 30, while seed 101 in fp32 leaves 1e-4 at k = 38; in the wide types the same comparison gives
    at most 1e-13 up to k = 40.
SpMV rows are held bit for bit to the host restatement (tests/spmv_ref.py: stored order from +0, one rounding per operation) and to
its textbook bound; nothing here is tuned to a device result."""
import ctypes

import numpy as np
import pytest

import cg_numpy
import cg_oracle
import spmv_ref as R
from conftest import rand_csr, rand_vec

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
ALL = list(DT)
NSYS = 3


def scaled(ip, a, ix, seed):
    """a[j] * s[row(j)] * s[col(j)], s = default_rng(seed).uniform(0.8, 1.25, n), in a's (wide) type"""
    n = len(ip) - 1
    s = np.random.default_rng(seed).uniform(0.8, 1.25, n)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(ip, dtype=np.int64)))
    return a * s[rows] * s[np.asarray(ix)]


def batched(pkg, ctx, ip, ix, vals, dtype, flags=0):
    """one batched handle on the systems `vals` (a list of value arrays on the pattern ip / ix)"""
    stack = np.concatenate([np.asarray(v) for v in vals]).astype(dtype)
    return pkg.Solver(ctx, len(ip) - 1, len(ix), stack, ip, ix, len(vals), flags=flags, batched=True)


def nan_like(count, dtype):
    v = np.full(count, np.nan, dtype=dtype)
    if np.dtype(dtype).kind == "c":
        v = (v + 1j * v).astype(dtype)
    return v


def device_spmv(pkg, ctx, s, x, n, nsys, dtype, fused=False):
    """s.spmv on device buffers with the caller's stride n; y prefilled with NaN -> (y (nsys, n), form)"""
    import torch
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(dev)
    yd = torch.from_numpy(nan_like(nsys * n, dtype)).to(dev)
    torch.cuda.synchronize()
    s.spmv(xd, yd, fused_dot=fused)
    form = s.last_spmv_form()
    ctx.synchronize()
    return yd.cpu().numpy().reshape(nsys, n), form


# ---- 1. SpMV, row by row ------------------------------------------------------------------------------------------------------------
_SPMV = {}


def spmv_case(key, build, dtype, nsys=NSYS):
    """pattern, independent values and x per system, host results -- computed once per case"""
    if key not in _SPMV:
        rng = np.random.default_rng(sum(map(ord, repr(key))))
        ip, ix, _ = build(rng)
        n = len(ip) - 1
        vals = [rand_vec(rng, len(ix), dtype) for _ in range(nsys)]
        x = np.stack([rand_vec(rng, n, dtype) for _ in range(nsys)])
        _SPMV[key] = {"ip": ip, "ix": ix, "n": n, "vals": vals, "x": x,
                      "want": [R.spmv_in_type(ip, ix, vals[r], x[r], dtype)[0] for r in range(nsys)]}
    return _SPMV[key]


def check_spmv(pkg, gpu, c, dtype, bits=True, wide_form=0):
    ctx = gpu[0]
    nsys = len(c["vals"])
    s = batched(pkg, ctx, c["ip"], c["ix"], c["vals"], dtype)
    try:
        y, form = device_spmv(pkg, ctx, s, c["x"], c["n"], nsys, dtype)
    finally:
        s.close()
    assert form["family"] == "batched" and form["fused"] == 0 and form["partials"] == 0, form
    assert form["wide"] == wide_form, form
    for r in range(nsys):
        R.check_rows(y[r], c["ip"], c["ix"], c["vals"][r], c["x"][r], dtype, label=f"system {r}")
        if bits:
            assert R.bit_equal(y[r], c["want"][r]), f"system {r}: rows differ from the host restatement"
    return y


@pytest.mark.parametrize("dt", ALL)
def test_spmv_rows_bit_for_bit(pkg, gpu, dt):
    dtype = DT[dt]
    c = spmv_case(("base", dt), lambda rng: rand_csr(rng, 1000, 6, dtype, empty_rows=True), dtype)
    y = check_spmv(pkg, gpu, c, dtype)
    assert not R.bit_equal(y[0], y[1]) and not R.bit_equal(y[1], y[2])


@pytest.mark.parametrize("dt", ALL)
def test_spmv_long_row(pkg, gpu, dt):
    """a row of 700 entries in block 0: longer than any batch of the walk, a slice several times the others'"""
    dtype = DT[dt]
    c = spmv_case(("long", dt), lambda rng: rand_csr(rng, 1000, 6, dtype, empty_rows=True, long_row=(17, 700)), dtype)
    check_spmv(pkg, gpu, c, dtype, bits=False)


@pytest.mark.parametrize("dt", ["c64", "f64"])
def test_spmv_odd_size_through_the_callers_stride(pkg, gpu, dt):
    """n = 1521: the handle carries a padding row, x and y keep the caller's stride of 1521 values"""
    dtype = DT[dt]
    c = spmv_case(("odd", dt), lambda rng: rand_csr(rng, 1521, 6, dtype, empty_rows=True), dtype)
    ctx = gpu[0]
    s = batched(pkg, ctx, c["ip"], c["ix"], c["vals"], dtype)
    try:
        assert s.ld == 1522
    finally:
        s.close()
    check_spmv(pkg, gpu, c, dtype)


@pytest.mark.parametrize("dt", ALL)
def test_spmv_slices_beyond_the_lds_limit(pkg, gpu, dt):
    """40 entries per row on average: 256 rows of one system exceed the 64 KB slice limit in every type (about 10 000 entries x
    (sizeof(T) + 4) bytes), so the kernel that reads the matrix per row runs (form field `wide` = 1); same order, same bits"""
    dtype = DT[dt]
    c = spmv_case(("dense", dt), lambda rng: rand_csr(rng, 600, 40, dtype), dtype)
    spans, _ = R.plan_spans(c["ip"])
    assert spans[0] * (np.dtype(dtype).itemsize + 4) > 64 * 1024
    check_spmv(pkg, gpu, c, dtype, wide_form=1)


# ---- 2. fused d.q -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL)
def test_fused_dot_partials(pkg, gpu, dt):
    dtype = DT[dt]
    c = spmv_case(("base", dt), lambda rng: rand_csr(rng, 1000, 6, dtype, empty_rows=True), dtype)
    ctx = gpu[0]
    s = batched(pkg, ctx, c["ip"], c["ix"], c["vals"], dtype)
    try:
        y, form = device_spmv(pkg, ctx, s, c["x"], c["n"], NSYS, dtype, fused=True)
        part = s.dot_partials()
    finally:
        s.close()
    P = (c["n"] + 255) // 256
    assert form["family"] == "batched" and form["fused"] == 1 and form["partials"] == P, form
    assert part.shape == (NSYS, P)
    for r in range(NSYS):
        assert R.bit_equal(y[r], c["want"][r])
        re, im, _ = R.dot_ext(c["x"][r], y[r], dtype)
        got = part[r].sum()
        err = np.hypot(R.LD(got.real) - re, R.LD(got.imag) - im) if im is not None else abs(R.LD(got) - re)
        bound = R.stream_dot_bound(c["x"][r], y[r], dtype)
        print(f"system {r}: |sum of partials - d.y| = {float(err):.3g}, bound {float(bound):.3g}")
        assert err <= bound
        # the partial of a 256-row block is block_sum<256> of to_acc(vmul(d_i, y_i)), as every one-lane-per-row form writes it
        assert R.bit_equal(part[r], R.block_partials_in_type(c["x"][r], y[r], dtype))
    assert not np.array_equal(part[0], part[1]) and not np.array_equal(part[1], part[2]) and not np.array_equal(part[0], part[2])


# ---- 3. CG against the oracle, per system -------------------------------------------------------------------------------------------
_PATTERN = {}
_ORACLE = {}


def pattern(golden, cplx):
    """(ip, ix, a (wide), b (wide)): Helmholtz N = 32 for the complex types, Poisson 40 x 40 for the real ones"""
    if cplx not in _PATTERN:
        if cplx:
            g = golden["cg_iterates"]
            _PATTERN[cplx] = (g["helm32_indptr"], g["helm32_indices"], g["helm32_data"].astype(np.complex128),
                              g["helm32_b"].astype(np.complex128))
        else:
            ip, ix, a = cg_numpy.poisson2d(40)
            _PATTERN[cplx] = (ip, ix, a.astype(np.float64), np.linspace(1.0, 2.0, 1600))
    return _PATTERN[cplx]


def oracle(golden, cplx, r, iters=50):
    """the C oracle on system r alone (nrhs = 1), in the wide type; computed once"""
    if (cplx, r) not in _ORACLE:
        ip, ix, a, b = pattern(golden, cplx)
        _ORACLE[(cplx, r)] = cg_oracle.cg(ip, ix, scaled(ip, a, ix, 100 + r), b, n_iterations=iters, mode=cg_oracle.MODE_SEQUENTIAL)
    return _ORACLE[(cplx, r)]


def hold_to_oracle(h, x, ho, xo, dtype, r):
    narrow = np.dtype(dtype).itemsize // (2 if np.dtype(dtype).kind == "c" else 1) == 4
    rtol, kmax = (1e-4, 30) if narrow else (1e-10, 40)
    keep = np.abs(ho) / np.abs(ho[0]) > 1e-4
    keep[kmax + 1:] = False
    worst = np.max(np.abs(h[keep] - ho[keep]) / np.abs(ho[keep]))
    print(f"system {r}: largest relative delta_k difference {worst:.3g} over {int(keep.sum())} entries (rtol {rtol:g})")
    assert worst < rtol, (r, worst)
    if not narrow and x is not None:
        rel = np.linalg.norm(x - xo) / np.linalg.norm(xo)
        print(f"system {r}: ||x - x_o|| / ||x_o|| = {rel:.3g}")
        assert rel < 1e-8, (r, rel)


@pytest.mark.parametrize("flags", [0, 2, 4])      # graph replay, CGAMD_NO_GRAPH, CGAMD_UNFUSED
@pytest.mark.parametrize("nsys", [1, 3, 9])
@pytest.mark.parametrize("dt", ALL)
def test_cg_per_system_against_the_oracle(pkg, gpu, golden, dt, nsys, flags):
    dtype = DT[dt]
    cplx = np.dtype(dtype).kind == "c"
    ip, ix, a, b = pattern(golden, cplx)
    n = len(ip) - 1
    s = batched(pkg, gpu[0], ip, ix, [scaled(ip, a, ix, 100 + r) for r in range(nsys)], dtype, flags=flags)
    try:
        assert s.systems == nsys
        x, h = s.solve(np.tile(b, nsys).astype(dtype), None, 50)
    finally:
        s.close()
    assert h.shape == (51, nsys)
    for r in range(nsys):
        xo, ho = oracle(golden, cplx, r)
        hold_to_oracle(h[:, r], x[r * n:(r + 1) * n], ho[:, 0], xo, dtype, r)
    if nsys > 1:      # the systems really differ: 1-5 % in delta_k from k = 1 on
        assert abs(h[1, 0] - h[1, 1]) / abs(h[1, 0]) > 1e-3


def test_cg_more_than_256_row_blocks(pkg, gpu):
    """Poisson 300 x 300 (352 row blocks: every XCD's share of the schedule), float64, 3 systems, 30 iterations"""
    ip, ix, a = cg_numpy.poisson2d(300)
    a = a.astype(np.float64)
    n = len(ip) - 1
    b = np.linspace(1.0, 2.0, n)
    vals = [scaled(ip, a, ix, 100 + r) for r in range(NSYS)]
    s = batched(pkg, gpu[0], ip, ix, vals, np.float64)
    try:
        x, h = s.solve(np.tile(b, NSYS), None, 30)
    finally:
        s.close()
    for r in range(NSYS):
        _, ho = cg_oracle.cg(ip, ix, vals[r], b, n_iterations=30, mode=cg_oracle.MODE_SEQUENTIAL)
        hold_to_oracle(h[:, r], None, ho[:, 0], None, np.float64, r)


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------
def bits_case(golden, dt, seeds=(100, 101, 102)):
    """three scaled systems with a right-hand side of its own each"""
    dtype = DT[dt]
    ip, ix, a, b = pattern(golden, np.dtype(dtype).kind == "c")
    vals = [scaled(ip, a, ix, sd).astype(dtype) for sd in seeds]
    rhs = [(b * (1 + 0.25 * r)).astype(dtype) for r in range(len(seeds))]
    return dtype, ip, ix, vals, rhs


def run(pkg, ctx, ip, ix, vals, rhs, dtype, iters=(30,), flags=0):
    s = batched(pkg, ctx, ip, ix, vals, dtype, flags=flags)
    try:
        s.set_rhs(np.concatenate(rhs))
        for k in iters:
            s.iterate(k)
        return s.x(), s.history()
    finally:
        s.close()


@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_bits_are_stable(pkg, gpu, golden, dt):
    dtype, ip, ix, vals, rhs = bits_case(golden, dt)
    ctx = gpu[0]
    n = len(ip) - 1
    x30, h30 = run(pkg, ctx, ip, ix, vals, rhs, dtype)
    assert np.all(np.isfinite(h30.view(R.real_type(dtype))))
    x15, h15 = run(pkg, ctx, ip, ix, vals, rhs, dtype, iters=(15, 15))
    assert R.bit_equal(x15, x30) and R.bit_equal(h15, h30), "iterate(15) twice differs from iterate(30)"
    xn, hn = run(pkg, ctx, ip, ix, vals, rhs, dtype, flags=pkg._lib.NO_GRAPH)
    assert R.bit_equal(xn, x30) and R.bit_equal(hn, h30), "graph replay differs from plain launches"
    xa, ha = run(pkg, ctx, ip, ix, vals, rhs, dtype)
    assert R.bit_equal(xa, x30) and R.bit_equal(ha, h30), "results differ from run to run"
    perm = [2, 0, 1]
    xp, hp = run(pkg, ctx, ip, ix, [vals[p] for p in perm], [rhs[p] for p in perm], dtype)
    assert R.bit_equal(xp.reshape(3, n), x30.reshape(3, n)[perm]), "permuting the batch does not permute x"
    assert R.bit_equal(hp, np.ascontiguousarray(h30[:, perm])), "permuting the batch does not permute the history columns"
    assert not R.bit_equal(xp, x30)


# ---- 5. reload and borrowed values --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_reload_gives_the_bits_of_a_fresh_handle(pkg, gpu, golden, dt):
    dtype, ip, ix, vals, rhs = bits_case(golden, dt)
    _, _, _, vals2, _ = bits_case(golden, dt, seeds=(200, 201, 202))
    ctx = gpu[0]
    fresh = run(pkg, ctx, ip, ix, vals2, rhs, dtype)
    s = batched(pkg, ctx, ip, ix, vals, dtype)
    try:
        s.solve(np.concatenate(rhs), None, 30)
        with pytest.raises(ValueError):
            s.reload_matrix(vals2[0], ip, ix)               # one system's values: too few
        s.reload_matrix(np.concatenate(vals2), ip, ix)
        x, h = s.solve(np.concatenate(rhs), None, 30)
    finally:
        s.close()
    assert R.bit_equal(x, fresh[0]) and R.bit_equal(h, fresh[1])
    first = run(pkg, ctx, ip, ix, vals, rhs, dtype)
    assert not R.bit_equal(first[0], fresh[0])


@pytest.mark.parametrize("dt,shift", [("f64", 0), ("c64", 0), ("f32", 8), ("c128", 0)])
def test_borrowed_device_values(pkg, gpu, golden, dt, shift):
    """CGAMD_MATRIX_ON_DEVICE on a device array of nSystems * nnz values gives the bits of the owning handle; shift: the array starts
    that many bytes off a 16-byte boundary (the kernel realigns every slice)"""
    import torch
    dtype, ip, ix, vals, rhs = bits_case(golden, dt)
    ctx = gpu[0]
    dev = torch.device("cuda", 0)
    own = run(pkg, ctx, ip, ix, vals, rhs, dtype)
    raw = np.concatenate([np.zeros(shift, np.uint8), np.concatenate(vals).view(np.uint8), np.zeros(64, np.uint8)])
    tv = torch.from_numpy(raw).to(dev)
    tp = torch.from_numpy(np.asarray(ip, np.int32)).to(dev)
    tc = torch.from_numpy(np.asarray(ix, np.int32)).to(dev)
    assert tv.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    s = pkg.Solver(ctx, len(ip) - 1, len(ix), tv.data_ptr() + shift, tp, tc, 3, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype, batched=True)
    s._keep = (tv, tp, tc)
    try:
        x, h = s.solve(np.concatenate(rhs), None, 30)
    finally:
        s.close()
    assert R.bit_equal(x, own[0]) and R.bit_equal(h, own[1])


# ---- 6. contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("dt", ALL)
def test_contract_accessors_and_byte_models(pkg, gpu, golden, dt, flags):
    dtype, ip, ix, vals, rhs = bits_case(golden, dt)
    ctx = gpu[0]
    n, nnz, V, nsys = len(ip) - 1, len(ix), np.dtype(dtype).itemsize, 3
    s = batched(pkg, ctx, ip, ix, vals, dtype, flags=flags)
    plain = pkg.Solver(ctx, n, nnz, vals[0], ip, ix, 3)
    try:
        assert s.systems == nsys and plain.systems == 0
        lib = pkg._lib.load()
        assert lib.cgamd_solver_loop_launches(s.handle) >= 2
        assert lib.cgamd_solver_layout(s.handle) == 0
        assert (s.index_codes, s.value_codes, s.joint_codes) == (0, 0, 0)
        matrix = nnz * (nsys * V + 4) + 4 * (n + 1)
        assert s.spmv_bytes == matrix + 2 * n * V * nsys
        assert s.spmv_moved_bytes == matrix + 2 * n * V * nsys
        assert s.iter_bytes(True) == matrix + 11 * n * V * nsys
        assert s.iter_bytes(False) == matrix + 14 * n * V * nsys
        assert s.iter_moved_bytes == matrix + (14 if flags & 4 else 10) * n * V * nsys
        s.set_rhs(np.concatenate(rhs))
        s.iterate(5)
        assert lib.cgamd_solver_layout(s.handle) == 0 and lib.cgamd_solver_loop_launches(s.handle) >= 2
    finally:
        s.close()
        plain.close()


@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_refused_calls_leave_the_handle_as_it_was(pkg, gpu, golden, dt):
    dtype, ip, ix, vals, rhs = bits_case(golden, dt)
    ctx = gpu[0]
    n = len(ip) - 1
    lib, L = pkg._lib.load(), pkg._lib
    want = run(pkg, ctx, ip, ix, vals, rhs, dtype)
    m = np.ones(n, dtype=dtype)
    y = np.zeros(16 * n, dtype=dtype)
    s = batched(pkg, ctx, ip, ix, vals, dtype)
    try:
        x, h = s.solve(np.concatenate(rhs), None, 30)
        assert R.bit_equal(x, want[0]) and R.bit_equal(h, want[1])
        ran = ctypes.c_int(-1)
        refused = {
            "iterate_tol": lib.cgamd_solver_iterate_tol(s.handle, 10, 1e-6, ctypes.byref(ran)),
            "spmm_rowmajor": lib.cgamd_solver_spmm_rowmajor(s.handle, L.ptr(y), L.ptr(y), 16),
            "set_preconditioner": lib.cgamd_solver_set_preconditioner(s.handle, L.ptr(m), 0),
            "tridiag": lib.cgamd_solver_set_preconditioner_tridiag(s.handle, L.ptr(m), L.ptr(m), L.ptr(m), 0),
            "tridiag_strided": lib.cgamd_solver_set_preconditioner_tridiag_strided(s.handle, 2, L.ptr(m), L.ptr(m), L.ptr(m), 0),
            "line": lib.cgamd_solver_set_preconditioner_line(s.handle, 1),
            "jacobi": lib.cgamd_solver_set_preconditioner_jacobi(s.handle),
        }
        assert refused == {k: L.ERR_STATE for k in refused}, refused
        assert b"batched" in lib.cgamd_last_error()
        assert s.preconditioner_source == 0 and s.iterations_done() == 30
        # the state of the solve is untouched: the iterations go on where they were ...
        s.iterate(5)
        x35, h35 = s.x(), s.history()
        again = run(pkg, ctx, ip, ix, vals, rhs, dtype, iters=(30, 5))
        assert R.bit_equal(x35, again[0]) and R.bit_equal(h35, again[1])
        # ... removing a preconditioner that is not there is fine, and the next solve returns the same bits
        assert lib.cgamd_solver_set_preconditioner(s.handle, None, 0) == L.OK
        s.set_preconditioner(None)
        x, h = s.solve(np.concatenate(rhs), None, 30)
        assert R.bit_equal(x, want[0]) and R.bit_equal(h, want[1])
    finally:
        s.close()


def test_solve_subdomains_with_a_list_of_matrices(pkg, gpu, golden):
    """as_prec with VarCoeff: three sub-domain matrices on one pattern, complex64, against three batched-of-one solves"""
    import types
    ip, ix, a, b = pattern(golden, True)
    ctx = gpu[0]
    n = len(ip) - 1
    P = [types.SimpleNamespace(indptr=ip, indices=ix, data=scaled(ip, a, ix, 100 + r)) for r in range(3)]
    res = [(b * (1 + 0.25 * r)).reshape(32, 32) for r in range(3)]
    out = pkg.solve_subdomains(ctx, P, res, 20)
    assert len(out) == 3 and all(o.shape == (32, 32) and o.dtype == np.complex128 for o in out)
    keep = pkg.Solver(ctx, n, len(ix), np.zeros(3 * len(ix), np.complex64), ip, ix, 3, batched=True)
    try:
        out2 = pkg.solve_subdomains(ctx, tuple(P), res, 20, solver=keep)       # the caller's batched handle: values reloaded from P
    finally:
        keep.close()
    for r in range(3):
        x1, _ = run(pkg, ctx, ip, ix, [P[r].data], [res[r].ravel()], np.complex64, iters=(20,))
        rel = np.linalg.norm(out[r].ravel() - x1) / np.linalg.norm(x1)
        print(f"sub-domain {r}: relative difference to a batched-of-one solve {rel:.3g}")
        assert rel < 1e-5
        assert np.array_equal(out2[r], out[r])
    plain = pkg.Solver(ctx, n, len(ix), P[0].data.astype(np.complex64), ip, ix, 3)
    try:
        with pytest.raises(ValueError, match="batched"):
            pkg.solve_subdomains(ctx, P, res, 20, solver=plain)
    finally:
        plain.close()
    # the shared-matrix forms keep their meaning: one matrix for all residuals, as an object with .indptr or as a 3-tuple of arrays
    same = pkg.solve_subdomains(ctx, (ip, ix, P[0].data), res, 20)
    same2 = pkg.solve_subdomains(ctx, P[0], res, 20)
    x, _ = plain_solve(pkg, ctx, ip, ix, P[0].data, res)
    for r in range(3):
        assert np.array_equal(same[r], same2[r])
        assert np.array_equal(same[r].ravel(), x[r * n:(r + 1) * n].astype(complex))


def plain_solve(pkg, ctx, ip, ix, data, res, iters=20):
    """the shared-matrix handle on the residuals, as solve_subdomains has always run it"""
    s = pkg.Solver(ctx, len(ip) - 1, len(ix), np.asarray(data, np.complex64), ip, ix, len(res))
    try:
        return s.solve(np.concatenate([np.asarray(v).ravel() for v in res]).astype(np.complex64), None, iters)
    finally:
        s.close()
