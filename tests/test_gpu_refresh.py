"""cgamd_solver_refresh_values: new matrix VALUES on the same pattern, in place on the device (include/cgamd.h).  The yardstick is never
the refreshed handle on its own: it is a FRESH handle created from the new values under the same tuning keys and flags, compared bit for
bit -- the SpMV plain and with the fused d.q partials, and x plus history after set_rhs and 25 iterations.  That holds because every
coded form is a re-encoding with the same products in the same order.  The SpMV is compared with the host restatement of
tests/spmv_ref.py as well.  Every case asserts what the refresh says it did (last_refresh), the three code accessors and the SpMV form
that really ran (Solver.last_spmv_form)."""
import numpy as np
import pytest

import spmv_ref as R

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32, "c64": np.complex64}
GRID = (130, 5, 4)          # 2 600 rows, 27 row patterns, the non-zero count no multiple of 256
ITERS = 25

# struct Tuning's defaults (csrc/cgamd_internal.h) of every key this module sets
DEFAULTS = {"resident": 1, "index_codes_min_mb": 32, "dev.row_codes_min_mb": 32}
BASE = {"resident": 0, "index_codes_min_mb": 0, "dev.row_codes_min_mb": 0}      # such small systems then build every code


@pytest.fixture
def tuned(pkg):
    """the keys of BASE, set BEFORE a handle is created (a handle keeps the configuration it was created under); tuned(False) sets
    the defaults; the defaults are restored afterwards"""
    lib = pkg._lib.load()

    def put(kv):
        for k, v in kv.items():
            pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))

    def tune(base=True):
        put(BASE if base else DEFAULTS)
    tune()
    yield tune
    put(DEFAULTS)


# ---- matrices ------------------------------------------------------------------------------------------------------------------------
_MAT = {}


def pattern(grid=GRID):
    import cg_numpy
    if grid not in _MAT:
        ip, ix, da = cg_numpy.laplace3d(*grid) if len(grid) == 3 else cg_numpy.poisson2d(*grid)
        rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        _MAT[grid] = (np.asarray(ip, np.int32), np.asarray(ix, np.int32), np.asarray(da, np.float64), rows)
    return _MAT[grid]


def in_type(da, dtype):
    """complex symmetric, still few distinct entries (as the tests of the value codes make them)"""
    return (da * (1.0 + 0.25j)).astype(dtype) if np.dtype(dtype).kind == "c" else da.astype(dtype)


def stencil(grid=GRID, tau=None):
    """tau None: diag 6 (4 in 2-D) / off -1; else I + tau L: diag 1 + 6 tau, off -tau"""
    ip, ix, da, rows = pattern(grid)
    if tau is None:
        return da.copy()
    return np.where(ix == rows, 1.0 + da.max() * tau, -tau)


def aniso(grid=GRID):
    """the z couplings times 100"""
    ip, ix, da, rows = pattern(grid)
    out = stencil(grid, 0.375)
    out[np.abs(ix - rows) == grid[0] * grid[1]] *= 100.0
    return out


def variable(grid=GRID):
    da = stencil(grid)
    return da * (1.0 + np.arange(len(da)) / (4.0 * len(da)))


# ---- device side ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def put(t, a):
    """overwrite the device tensor in place, done when this returns"""
    import torch
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    torch.cuda.synchronize()


class Borrowed:
    """a handle on device arrays it borrows; `vals` is the tensor the handle reads"""

    def __init__(self, pkg, ctx, grid, da, dtype, flags=0, n_rhs=1, batched=False):
        ip, ix, _, _ = pattern(grid)
        self.ip, self.ix, self.vals = dev(ip), dev(ix), dev(da)
        self.s = pkg.Solver(ctx, len(ip) - 1, len(ix), self.vals, self.ip, self.ix, n_rhs, flags=flags | pkg._lib.MATRIX_ON_DEVICE, dtype=dtype,
                            batched=batched)

    def close(self):
        self.s.close()


def nan_vector(n, dtype):
    v = np.full(n, np.nan, dtype=dtype)
    if np.dtype(dtype).kind == "c":
        v = (v + 1j * v).astype(dtype)
    return dev(v)


_VEC = {}


def vectors(n, dtype, n_rhs):
    key = (n, np.dtype(dtype).name, n_rhs)
    if key not in _VEC:
        rng = np.random.default_rng(n * 8 + n_rhs)
        x = np.concatenate([R.adversarial_d(rng, n, dtype).reshape(-1) for _ in range(n_rhs)])
        b = np.concatenate([np.linspace(1.0, 2.0 + r, n) for r in range(n_rhs)]).astype(dtype)
        _VEC[key] = (x, b)
    return _VEC[key]


def results(pkg, ctx, s, dtype, iters=ITERS, spmv=True):
    """everything a case compares: the SpMV on an adversarial x (plain, fused, y prefilled with NaN), then set_rhs and `iters` iterations"""
    import torch
    n, k = s.size, s.n_rhs
    x, b = vectors(n, dtype, k)
    out = {"x_in": x}
    try:
        if spmv:
            xd = dev(x)
            for f in (False, True):
                yd = nan_vector(n * k, dtype)
                torch.cuda.synchronize()
                s.spmv(xd, yd, fused_dot=f)
                out[f"form{int(f)}"] = s.last_spmv_form()
                ctx.synchronize()
                out[f"y{int(f)}"] = yd.cpu().numpy()
            out["parts"] = s.dot_partials().copy()
        s.set_rhs(b)
        s.iterate(iters)
        ctx.synchronize()
    except pkg.CgAmdError as e:
        if e.status == pkg._lib.ERR_HIP:       # a kernel faulted: nothing more is started on that device in this session
            pytest.exit(f"HIP error, the session ends here: {e}", returncode=3)
        raise
    out["history"] = s.history().copy()
    out["x"] = s.x().copy()
    assert out["history"].shape == (iters + 1, k) and np.all(np.isfinite(out["history"]))
    return out


def same_bits(label, got, want):
    for key in ("y0", "y1", "parts", "history", "x"):
        if key in want or key in got:
            assert R.bit_equal(got[key], want[key]), f"{label}: {key} differs from the fresh handle"
    for key in ("form0", "form1"):
        if key in want:
            assert got[key] == want[key], f"{label}: launched {got[key]}, the fresh handle {want[key]}"


def host_bits(label, got, grid, da, dtype):
    """the SpMV against the host restatement (single right-hand side)"""
    ip, ix, _, _ = pattern(grid)
    n = len(ip) - 1
    x = got["x_in"].reshape(1, n)
    y = R.spmv_in_type(ip, ix, da, x, dtype)
    assert R.bit_equal(got["y0"].reshape(1, n), y) and R.bit_equal(got["y1"].reshape(1, n), y), f"{label}: y differs from the host restatement"
    assert R.bit_equal(got["parts"][0], R.block_partials_in_type(x[0], y[0], dtype)), f"{label}: d.q partials differ from the restated block sums"


def codes(s):
    return (s.index_codes, s.value_codes, s.joint_codes, s.row_codes)


_FRESH = {}


def fresh(pkg, ctx, grid, da, dtype, flags=0, pre=None, key=None, **kw):
    """the yardstick: a new borrowing handle on these values under the keys now in force; computed once per key and shared"""
    if key is not None and key in _FRESH:
        return _FRESH[key]
    h = Borrowed(pkg, ctx, grid, da, dtype, flags=flags, **kw)
    try:
        if pre is not None:
            h.s.set_preconditioner(pre)
        out = results(pkg, ctx, h.s, dtype)
        out["codes"] = codes(h.s)
    finally:
        h.close()
    if key is not None:
        _FRESH[key] = out
    return out


def refreshed(pkg, ctx, h, label, grid, da, dtype, outcome, flags=0, pre=None, key=None, accessors=True, host=True, **kw):
    """write da into the borrowed tensor, refresh, and hold the handle to the fresh one"""
    put(h.vals, da)
    h.s.refresh_values()
    assert h.s.last_refresh == outcome, f"{label}: last_refresh {h.s.last_refresh}, expected {outcome}"
    got = results(pkg, ctx, h.s, dtype)
    want = fresh(pkg, ctx, grid, da, dtype, flags=flags, pre=pre, key=key, **kw)
    print(f"{label}: outcome {h.s.last_refresh}, codes {codes(h.s)}, fresh {want['codes']}, form {got['form1']}")
    same_bits(label, got, want)
    if accessors:
        assert codes(h.s) == want["codes"], f"{label}: codes {codes(h.s)}, the fresh handle's {want['codes']}"
    if host and h.s.n_rhs == 1:
        host_bits(label, got, grid, da, dtype)
    return got


ROWCODE = {"family": "rowcode", "index_bits": 8, "value_codes": 3}


def ran(got, **want):
    for f in ("form0", "form1"):
        assert {k: got[f][k] for k in want} == want, (got[f], want)


# ---- 1. the fast path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,no_graph", [("f64", False), ("f64", True), ("f32", False), ("c64", False)], ids=["f64", "f64-no-graph", "f32", "c64"])
def test_fast_path(pkg, gpu, tuned, dt, no_graph):
    """diag 6 / off -1 (2 values, 7 pairs, 27 patterns) rescaled to I + 0.375 L after iterate(16) has captured the graphs of 8: the
    dictionaries are rewritten, nothing else moves, and the family-7 form returns the bits of a fresh handle"""
    dtype = DT[dt]
    ctx = gpu[0]
    flags = pkg._lib.NO_GRAPH if no_graph else 0
    h = Borrowed(pkg, ctx, GRID, in_type(stencil(), dtype), dtype, flags=flags)
    try:
        s = h.s
        assert codes(s) == (7, 2, 7, 27) and s.last_refresh == 0
        _, b = vectors(s.size, dtype, 1)
        s.set_rhs(b)
        s.iterate(16)
        ctx.synchronize()
        captured = s.graph_captures
        assert (captured == 0) == no_graph
        new = in_type(stencil(tau=0.375), dtype)
        got = refreshed(pkg, ctx, h, f"fast {dt}", GRID, new, dtype, 1, flags=flags, key=("rescaled", dt, no_graph))
        assert codes(s) == (7, 2, 7, 27)
        ran(got, **ROWCODE)
        # the 25 iterations after the refresh replayed the graph of 8 captured BEFORE it; only the graph of one iteration is new
        assert s.graph_captures == (0 if no_graph else captured + 1), (captured, s.graph_captures)
        captured = s.graph_captures
        # once more, back: the graphs captured above are replayed on the dictionaries as they are now
        refreshed(pkg, ctx, h, f"fast {dt} back", GRID, in_type(stencil(), dtype), dtype, 1, flags=flags, key=("plain", dt, no_graph))
        assert s.graph_captures == captured, "a refresh that rewrote the dictionaries only destroyed the graphs"
        # ... while a rebuild replaces the code arrays the graphs hold: both graphs are captured again
        refreshed(pkg, ctx, h, f"fast {dt} then rebuilt", GRID, in_type(aniso(), dtype), dtype, 2, flags=flags)
        assert s.graph_captures == (0 if no_graph else captured + 2), (captured, s.graph_captures)
    finally:
        h.close()


# ---- 2. one entry breaks a class -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [0, 255, 256, -1], ids=["first", "255", "256", "last"])
def test_one_entry_breaks_a_class(pkg, gpu, tuned, where):
    """from the rescaled state a single non-zero is perturbed -- the first, the two sides of a block edge, the last (the tail of the
    16-byte walk): the one-pass check sees it, the codes are rebuilt, the bits and the accessors are the fresh handle's"""
    dtype = np.float64
    ctx = gpu[0]
    h = Borrowed(pkg, ctx, GRID, stencil(), dtype)
    try:
        new = stencil(tau=0.375)
        refreshed(pkg, ctx, h, "rescaled", GRID, new, dtype, 1, key=("rescaled", "f64", False))
        j = where % len(new)
        new = new.copy()
        new[j] = new[j] * 1.5
        got = refreshed(pkg, ctx, h, f"perturbed {j}", GRID, new, dtype, 2)
        assert h.s.value_codes == 3 and h.s.row_codes >= 27       # (a corner row has a pattern of its own before and after)
        ran(got, **ROWCODE)
    finally:
        h.close()


# ---- 3. classes merge ----------------------------------------------------------------------------------------------------------------
def test_classes_merge(pkg, gpu, tuned):
    """all values 1.0: two codes now stand for equal values, the arrays are still right; the accessors keep the entries in use"""
    dtype = np.float64
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype)
    try:
        got = refreshed(pkg, gpu[0], h, "merged", GRID, np.ones_like(stencil()), dtype, 1, accessors=False)
        assert codes(h.s) == (7, 2, 7, 27)
        ran(got, **ROWCODE)
    finally:
        h.close()


# ---- 4. anisotropy appears -----------------------------------------------------------------------------------------------------------
def test_anisotropy_appears(pkg, gpu, tuned):
    """the z couplings times 100: the off-diagonal class splits; joint and row codes are present again after the rebuild"""
    dtype = np.float64
    h = Borrowed(pkg, gpu[0], GRID, stencil(tau=0.375), dtype)
    try:
        got = refreshed(pkg, gpu[0], h, "anisotropic", GRID, aniso(), dtype, 2)
        assert h.s.value_codes == 3 and h.s.joint_codes == 7 and h.s.row_codes == 27
        ran(got, **ROWCODE)
    finally:
        h.close()


# ---- 5. variable coefficients --------------------------------------------------------------------------------------------------------
def test_variable_coefficients_and_back(pkg, gpu, tuned):
    """more than 256 values: the codes of the values go, the row-block form reads aValues (and the column codes, which the refresh
    does not touch); back to the constant matrix the handle gains them again"""
    dtype = np.float64
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype)
    try:
        var = variable()
        assert R.distinct_values(var) > 256
        got = refreshed(pkg, gpu[0], h, "variable", GRID, var, dtype, 3)
        assert h.s.value_codes == 0 and h.s.row_codes == 0 and h.s.joint_codes == 0 and h.s.index_codes == 7
        ran(got, family="rowblock", index_bits=8, value_codes=0)
        got = refreshed(pkg, gpu[0], h, "constant again", GRID, stencil(), dtype, 2, key=("plain", "f64", False))
        assert codes(h.s) == (7, 2, 7, 27)
        ran(got, **ROWCODE)
    finally:
        h.close()


# ---- 6. a handle that owns its matrix; refused arguments -----------------------------------------------------------------------------
def test_owning_handle(pkg, gpu, tuned):
    """refresh_values from a numpy array and from a device tensor: the bits of reload_matrix with the same pattern"""
    dtype = np.float64
    ctx = gpu[0]
    ip, ix, _, _ = pattern()
    a, b = stencil(tau=0.375), aniso()
    s = pkg.Solver(ctx, len(ip) - 1, len(ix), stencil(), ip, ix, 1)
    t = pkg.Solver(ctx, len(ip) - 1, len(ix), stencil(), ip, ix, 1)
    try:
        for label, new, route, outcome in (("host", a, lambda v: v, 1), ("device", b, dev, 2)):
            s.refresh_values(route(new))
            assert s.last_refresh == outcome
            t.reload_matrix(new, ip, ix)
            got, want = results(pkg, ctx, s, dtype), results(pkg, ctx, t, dtype)
            same_bits(f"owning, {label} route", got, want)
            host_bits(f"owning, {label} route", got, GRID, new, dtype)
            assert codes(s) == codes(t)
        lib = pkg._lib.load()
        assert lib.cgamd_solver_refresh_values(s.handle, None, 0) == pkg._lib.ERR_INVALID
        assert lib.cgamd_solver_refresh_values(s.handle, None, 1) == pkg._lib.ERR_INVALID
        same_bits("owning, after the refused calls", results(pkg, ctx, s, dtype), want)
    finally:
        s.close()
        t.close()


def test_foreign_pointer_on_a_borrowing_handle(pkg, gpu, tuned):
    """another array than the borrowed one is ERR_INVALID and leaves the handle as it was: same bits, a solve in progress goes on"""
    dtype = np.float64
    ctx = gpu[0]
    lib, L = pkg._lib.load(), pkg._lib
    h = Borrowed(pkg, ctx, GRID, stencil(), dtype)
    try:
        before = results(pkg, ctx, h.s, dtype)
        other = dev(stencil(tau=0.375))
        for p, on_device in ((other, 1), (stencil(tau=0.375), 0), (h.vals, 0)):
            assert lib.cgamd_solver_refresh_values(h.s.handle, L.ptr(p), on_device) == L.ERR_INVALID
            assert b"borrow" in lib.cgamd_last_error()
        assert h.s.last_refresh == 0
        h.s.iterate(1)                  # rhs_set was not cleared
        same_bits("after the refused calls", results(pkg, ctx, h.s, dtype), before)
        # the borrowed pointer itself, on_device = 1, is the other spelling of NULL
        L.check(lib.cgamd_solver_refresh_values(h.s.handle, L.ptr(h.vals), 1))
        assert h.s.last_refresh == 1
        same_bits("after the refresh by pointer", results(pkg, ctx, h.s, dtype), before)
    finally:
        h.close()


# ---- 7. the next call must be set_rhs ------------------------------------------------------------------------------------------------
def test_iterate_needs_a_new_set_rhs(pkg, gpu, tuned):
    dtype = np.float64
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype)
    try:
        _, b = vectors(h.s.size, dtype, 1)
        h.s.set_rhs(b)
        h.s.iterate(3)
        h.s.refresh_values()
        with pytest.raises(pkg.CgAmdError) as e:
            h.s.iterate(1)
        assert e.value.status == pkg._lib.ERR_STATE
        h.s.set_rhs(b)
        h.s.iterate(1)
    finally:
        h.close()


# ---- 8. preconditioners --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["jacobi", ("line", 1), ("line", GRID[0] * GRID[1])], ids=["jacobi", "line-1", "line-nxny"])
def test_preconditioner_from_the_matrix_follows(pkg, gpu, tuned, pre):
    """built from the matrix: built again from the new values, same kind and stride -- the bits of a fresh handle with it"""
    dtype = np.float64
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype)
    try:
        h.s.set_preconditioner(pre)
        source = h.s.preconditioner_source
        assert source >= 2
        refreshed(pkg, gpu[0], h, f"{pre} rescaled", GRID, stencil(tau=0.375), dtype, 1, pre=pre)
        assert h.s.preconditioner_source == source
        refreshed(pkg, gpu[0], h, f"{pre} anisotropic", GRID, aniso(), dtype, 2, pre=pre)
        assert h.s.preconditioner_source == source
    finally:
        h.close()


def test_preconditioner_from_the_callers_array_is_kept(pkg, gpu, tuned):
    dtype = np.float64
    n = len(pattern()[0]) - 1
    m = 1.0 / (5.0 + np.arange(n) / n)
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype)
    try:
        h.s.set_preconditioner(m)
        refreshed(pkg, gpu[0], h, "caller's diagonal", GRID, stencil(tau=0.375), dtype, 1, pre=m)
        assert h.s.preconditioner_source == 1
    finally:
        h.close()


def test_failed_rebuild_removes_the_preconditioner(pkg, gpu, tuned):
    """new values with a zero diagonal in row 1234: the error names the row, the preconditioner is gone, the values are in force --
    the bits of a fresh unpreconditioned handle on them"""
    dtype = np.float64
    ip, ix, _, rows = pattern()
    new = stencil(tau=0.375)
    new[(rows == 1234) & (ix == 1234)] = 0.0
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype)
    try:
        h.s.set_preconditioner("jacobi")
        put(h.vals, new)
        with pytest.raises(pkg.CgAmdError) as e:
            h.s.refresh_values()
        assert e.value.status == pkg._lib.ERR_INVALID and "1234" in str(e.value)
        assert h.s.preconditioner_source == 0 and h.s.last_refresh == 2
        got = results(pkg, gpu[0], h.s, dtype)
        same_bits("after the failed rebuild", got, fresh(pkg, gpu[0], GRID, new, dtype))
    finally:
        h.close()


# ---- 9. handles that read the values live --------------------------------------------------------------------------------------------
def test_multi_rhs_handle(pkg, gpu, tuned):
    dtype = np.float64
    h = Borrowed(pkg, gpu[0], GRID, stencil(), dtype, n_rhs=3)
    try:
        assert codes(h.s)[1:] == (0, 0, 0)
        refreshed(pkg, gpu[0], h, "3 right-hand sides", GRID, aniso(), dtype, 0, n_rhs=3)
    finally:
        h.close()


def test_batched_handle_with_jacobi(pkg, gpu, tuned):
    dtype = np.float64
    three = lambda f: np.concatenate([f(), 1.25 * f(), 0.5 * f()])
    h = Borrowed(pkg, gpu[0], GRID, three(stencil), dtype, n_rhs=3, batched=True)
    try:
        h.s.set_preconditioner("jacobi")
        refreshed(pkg, gpu[0], h, "batched", GRID, three(aniso), dtype, 0, pre="jacobi", n_rhs=3, batched=True)
        assert h.s.preconditioner_source == 2
    finally:
        h.close()


def test_complex128_handle(pkg, gpu, tuned):
    dtype = np.complex128
    h = Borrowed(pkg, gpu[0], GRID, in_type(stencil(), dtype), dtype)
    try:
        assert codes(h.s)[1:] == (0, 0, 0)
        refreshed(pkg, gpu[0], h, "complex128", GRID, in_type(aniso(), dtype), dtype, 0)
    finally:
        h.close()


@pytest.mark.parametrize("side,launches", [(40, 0), (200, 1)], ids=["one-xcd", "chip-wide"])
def test_resident_handles(pkg, gpu, tuned, side, launches):
    """the default keys: 1 600 rows run the one-XCD resident loop, 40 000 the chip-wide one; both load the matrix at every launch"""
    dtype = np.float64
    tuned(False)
    grid = (side,)
    h = Borrowed(pkg, gpu[0], grid, stencil(grid), dtype)
    try:
        lib = pkg._lib.load()
        assert lib.cgamd_solver_loop_launches(h.s.handle) == launches
        _, b = vectors(h.s.size, dtype, 1)
        h.s.set_rhs(b)
        h.s.iterate(ITERS)
        got = refreshed(pkg, gpu[0], h, f"resident {side}", grid, stencil(grid, tau=0.375), dtype, 0)
        assert lib.cgamd_solver_loop_launches(h.s.handle) == launches
    finally:
        h.close()


# ---- 10. an odd size -----------------------------------------------------------------------------------------------------------------
def test_odd_size(pkg, gpu, tuned):
    """1 965 rows are carried with an empty row appended (ld > size), which has a pattern of its own: both paths, the fresh handle's bits"""
    dtype = np.float64
    grid = (131, 5, 3)
    h = Borrowed(pkg, gpu[0], grid, stencil(grid), dtype)
    try:
        assert h.s.ld > h.s.size and h.s.row_codes == 27
        got = refreshed(pkg, gpu[0], h, "odd, rescaled", grid, stencil(grid, tau=0.375), dtype, 1)
        ran(got, **ROWCODE)
        got = refreshed(pkg, gpu[0], h, "odd, anisotropic", grid, aniso(grid), dtype, 2)
        ran(got, **ROWCODE)
    finally:
        h.close()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_tail_of_the_check_decides(pkg, gpu, tuned, dt):
    """11 629 non-zeros: one beyond the last 16-byte pack of values in fp64 and in fp32.  Only that LAST non-zero is changed, so the
    one-by-one tail of the check is what sees the class split"""
    dtype = DT[dt]
    grid = (131, 5, 3)
    h = Borrowed(pkg, gpu[0], grid, in_type(stencil(grid), dtype), dtype)
    try:
        new = stencil(grid, tau=0.375)
        assert len(new) % (16 // np.dtype(dtype).itemsize) == 1
        refreshed(pkg, gpu[0], h, f"tail {dt}, rescaled", grid, in_type(new, dtype), dtype, 1)
        new[-1] *= 1.5
        got = refreshed(pkg, gpu[0], h, f"tail {dt}, last entry", grid, in_type(new, dtype), dtype, 2)
        assert h.s.value_codes == 3
        ran(got, **ROWCODE)
    finally:
        h.close()


# ---- 11. the borrowed tensor written on torch's stream, no synchronisation by the caller -------------------------------------------
def test_refresh_orders_torchs_stream(pkg, gpu, tuned):
    """the recipe of INTEGRATION.md: the tensor is rewritten by work still queued on torch's stream when refresh_values() is called.
    The handle's stream waits for no other, so the wrapper has to: a refresh that read the array too early would keep the old
    dictionaries (the old values pass the check) and return the OLD matrix's bits"""
    import torch
    dtype = np.float64
    ctx = gpu[0]
    h = Borrowed(pkg, ctx, GRID, stencil(), dtype)
    try:
        new = stencil(tau=0.375)
        want = fresh(pkg, ctx, GRID, new, dtype, key=("rescaled", "f64", False))
        old = results(pkg, ctx, h.s, dtype)
        assert not R.bit_equal(old["y0"], want["y0"])
        new_d = dev(new)
        a = torch.ones((4096, 4096), dtype=torch.float32, device=new_d.device)
        torch.cuda.synchronize()
        for _ in range(40):             # a few tens of milliseconds of work ahead of the write, on torch's stream
            a = (a @ a) * (1.0 / 4096)
        h.vals.copy_(new_d)             # queued behind it; NO synchronisation here
        h.s.refresh_values()
        assert h.s.last_refresh == 1
        got = results(pkg, ctx, h.s, dtype)
        same_bits("written on torch's stream", got, want)
        assert float(a[0, 0]) == 1.0
    finally:
        h.close()
