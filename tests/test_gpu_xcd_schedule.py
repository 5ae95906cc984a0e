"""The plane-matched XCD schedule of the row- and pair-coded SpMV (csrc/xcd_schedule.cpp, csrc/spmv.hip; include/cgamd.h
cgamd_solver_spmv_schedule): a table per handle names the super block (1024 rows) of every work-group, so that rows a largest stride
apart meet on one XCD.  Which work-group computes a row enters neither y nor the per-256-row d.q partials, so every case is compared
BIT FOR BIT with the host restatement of tests/spmv_ref.py (y prefilled with NaN, x of adversarial magnitudes) after asserting --
through Solver.spmv_schedule and the grid Solver.last_spmv_form() recorded at the launch site, restated here from the formula -- that
the table really ran; then again with the same matrix under dev.spmv_plane = 0 (the block-cyclic schedule).  Matrices, the host side
(computed once per case and shared) and the device side are the ones of test_gpu_row_codes.py / test_gpu_row_pairs.py."""
import ctypes

import numpy as np
import pytest

import spmv_ref as R
import test_gpu_row_codes as RC
import test_gpu_row_pairs as RP

pytestmark = pytest.mark.gpu

# struct Tuning's defaults (csrc/cgamd_internal.h) of every key this module sets
DEFAULTS = dict(RP.DEFAULTS, **{"dev.spmv_plane": -1})
# codes at any size; dev.row_pairs by the default rule: 8-byte values run the pair form, 4-byte values the row form
BASE = dict(RC.BASE, **{"dev.row_pairs_min_mb": 0, "dev.spmv_plane": 1})
DT = {"f64": (np.float64, "rowpair"), "f32": (np.float32, "rowcode")}
SUPER = 1024


@pytest.fixture
def tuned(pkg):
    """sets tuning keys BEFORE a handle is created; every call starts from the defaults plus BASE; the defaults are restored afterwards"""
    lib = pkg._lib.load()

    def put(kv):
        for k, v in kv.items():
            assert k in DEFAULTS, k
            pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))

    def tune(**kv):
        put(DEFAULTS)
        put(BASE)
        put({k.replace("dev_", "dev."): v for k, v in kv.items()})
    yield tune
    put(DEFAULTS)


def plane_grid(n, unit):
    """8 x the longest list of the table: super block s on XCD floor(8 frac(centre(s) / unit))"""
    supers = -(-(-(-n // 256)) // 4)
    count = [0] * 8
    for s in range(supers):
        count[8 * ((s * SUPER + SUPER // 2) % unit) // unit] += 1
    return 8 * max(count), count


def lap3d(grid):
    import cg_numpy
    return lambda: cg_numpy.laplace3d(*grid)


# (label, host key, matrix, rows, unit)
CASES = {
    "n3001": (("xcd-st7", 3001), lambda: RC.stencil_matrix(3001, *RP.STENCIL7, np.float64), 3001, 300),
    "n70001": (("xcd-st7", 70001), lambda: RC.stencil_matrix(70001, *RP.STENCIL7, np.float64), 70001, 300),
    "24x20x64": (("xcd-lap3d", (24, 20, 64)), lap3d((24, 20, 64)), 30720, 480),
    "250x200x3": (("xcd-lap3d", (250, 200, 3)), lap3d((250, 200, 3)), 150000, 50000),
}


def run_schedule(pkg, ctx, label, h, dtype, family, kind, unit):
    """one handle under the tuning in force: what it says about its schedule, the form with the schedule's grid, then the bits"""
    ip, ix, da = h["mat"]
    s = pkg.Solver(ctx, h["n"], len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        assert s.row_codes > 0 and (s.row_pairs > 0) == (family == "rowpair")
        sched = s.spmv_schedule
        want = RP.want_form(family, h)
        if kind == "plane":
            grid, count = plane_grid(h["n"], unit)
            print(f"{label}: super blocks per XCD {count}")
            want = dict(want, grid=grid)
        assert sched == {"kind": kind, "grid": want["grid"], "unit_rows": unit}, sched
        runs = RC.spmv_both(pkg, ctx, s, h, dtype)
        return RC.verify(label, h, dtype, runs, want)
    finally:
        s.close()


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("case", list(CASES))
def test_table_changes_no_bit(pkg, gpu, tuned, case, dt, depth):
    """n3001: odd, 3 super blocks, the stride below a super block -- the blocks are scattered over the XCDs and the grid is mostly
    padding; n70001: 69 super blocks at stride 300; 24x20x64: exactly 30 super blocks, unit 480; 250x200x3: the headline's plane of
    50 000 rows, 147 super blocks that straddle the planes and an incomplete last one (150 000 = 146 x 1024 + 496)"""
    key, build, n, unit = CASES[case]
    dtype, family = DT[dt]
    h = RC.host(key + (dt,), build, dtype)
    assert h["n"] == n and h["max_row"] == 7
    tuned(dev_row_pipe=depth)
    y1, p1 = run_schedule(pkg, gpu[0], f"{case} {dt} depth{depth} plane", h, dtype, family, "plane", unit)
    tuned(dev_row_pipe=depth, dev_spmv_plane=0)
    y0, p0 = run_schedule(pkg, gpu[0], f"{case} {dt} depth{depth} cycle", h, dtype, family, "cycle", unit)
    assert R.bit_equal(y1, y0) and R.bit_equal(p1, p0)


def test_default_rule_keeps_the_cycle_below_256_mb(pkg, gpu, tuned):
    """dev.spmv_plane = -1, a stride of 48 super blocks, a matrix of 12 MB: the rule as measured (profiles/xcd_plane/) starts at 256 MB"""
    key, build, n, unit = CASES["250x200x3"]
    h = RC.host(key + ("f64",), build, np.float64)
    tuned(dev_spmv_plane=-1)
    run_schedule(pkg, gpu[0], "default rule", h, np.float64, "rowpair", "cycle", unit)


def test_default_rule_declines_an_unbalanced_table(pkg, gpu):
    """96 x 96 x 1100 (10.1M rows, 850 MB in fp64): the plane is exactly 9 super blocks, the table would put two blocks of every plane
    on one XCD (lists of 1100 and 2200: tests/test_xcd_schedule.py) and the launch would last 1.78 times as long.  The default rule
    keeps the cycle; asked for by name the table is built"""
    ctx = gpu[0]
    lib = pkg._lib.load()
    n = 96 * 96 * 1100
    ip, ix, da = pkg.generators.laplace3d(ctx, 96, 96, 1100, dtype=np.float64)
    try:
        for plane, want in ((-1, {"kind": "cycle", "grid": RC.rowblock_grid(-(-n // SUPER), 16), "unit_rows": 9216}),
                            (1, {"kind": "plane", "grid": plane_grid(n, 9216)[0], "unit_rows": 9216})):
            pkg._lib.check(lib.cgamd_tune(b"dev.spmv_plane", plane))
            s = pkg.Solver(ctx, n, int(ix.numel()), da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=np.float64)
            try:
                assert s.row_pairs > 0 and s.spmv_schedule == want, s.spmv_schedule
            finally:
                s.close()
    finally:
        pkg._lib.check(lib.cgamd_tune(b"dev.spmv_plane", -1))
    assert plane_grid(n, 9216)[0] > 1.7 * n / SUPER


@pytest.mark.parametrize("dt", list(DT))
def test_default_rule_at_the_headline(pkg, gpu, dt):
    """the tuning defaults on the 250 x 200 x 200 system (837 / 558 MB, stride 48.8 super blocks), matrix generated on the device: the
    handle takes the table by itself, and 8 iterations give the history and x of a handle under dev.spmv_plane = 0"""
    import torch
    dtype, family = DT[dt]
    ctx = gpu[0]
    lib = pkg._lib.load()
    n = 250 * 200 * 200
    ip, ix, da = pkg.generators.laplace3d(ctx, 250, 200, 200, dtype=dtype)
    b = torch.full((n,), 5.0, dtype=pkg.generators.torch_dtype(dtype), device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    got = {}
    try:
        for plane in (-1, 0):
            pkg._lib.check(lib.cgamd_tune(b"dev.spmv_plane", plane))
            s = pkg.Solver(ctx, n, int(ix.numel()), da, ip, ix, 1, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
            try:
                want = {"kind": "plane", "grid": plane_grid(n, 50000)[0], "unit_rows": 50000} if plane else \
                       {"kind": "cycle", "grid": RC.rowblock_grid(-(-n // SUPER), 16), "unit_rows": 50000}
                assert s.spmv_schedule == want, s.spmv_schedule
                s.set_rhs(b, None, on_device=True)
                s.iterate(8)
                ctx.synchronize()
                form = s.last_spmv_form()
                assert form["family"] == family and form["grid"] == want["grid"], form
                got[plane] = (s.history().copy(), s.x().copy())
            finally:
                s.close()
    finally:
        pkg._lib.check(lib.cgamd_tune(b"dev.spmv_plane", -1))
    assert got[-1][0].shape == (9, 1) and np.all(np.isfinite(got[-1][0]))
    assert R.bit_equal(got[-1][0], got[0][0]) and R.bit_equal(got[-1][1], got[0][1])


def read_vector(pkg, ctx, s, which, n):
    out = np.empty(n, dtype=s.dtype)
    ctx.synchronize()
    pkg._lib.check(pkg._lib.load().cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), ctypes.c_void_p(s.vector(which)), out.nbytes))
    return out


def test_the_loop_is_bit_identical(pkg, gpu, tuned):
    """one iterate(8) of the four-launch loop on the 150 000-row system (captured: the graph holds the table's pointer): x, r, d and the
    history under the table equal those under the cycle"""
    import cg_numpy
    dtype = np.float64
    ctx = gpu[0]
    lib = pkg._lib.load()
    ip, ix, da = RC.in_type(cg_numpy.laplace3d(250, 200, 3), dtype)
    n = len(ip) - 1
    got = {}
    for plane in (1, 0):
        tuned(dev_spmv_plane=plane, **RP.FOUR_LAUNCH)
        s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype)
        try:
            assert s.row_pairs > 0 and lib.cgamd_solver_loop_launches(s.handle) == 4
            assert s.spmv_schedule["kind"] == ("plane" if plane else "cycle") and s.spmv_schedule["unit_rows"] == 50000
            s.set_rhs(np.linspace(1.0, 2.0, n).astype(dtype))
            s.iterate(8)
            ctx.synchronize()
            form = s.last_spmv_form()
            assert form["family"] == "rowpair" and form["grid"] == s.spmv_schedule["grid"], form
            got[plane] = (s.history().copy(), s.x().copy(), read_vector(pkg, ctx, s, "r", n), read_vector(pkg, ctx, s, "d", n))
        finally:
            s.close()
    assert got[1][0].shape == (9, 1) and np.all(np.isfinite(got[1][0]))
    for a, b, name in zip(got[1], got[0], ("history", "x", "r", "d")):
        assert R.bit_equal(a, b), f"{name} under the table differs from the cycle's"


def test_reload_with_another_stride_rebuilds_the_table(pkg, gpu, tuned):
    """reload_matrix with a pattern of another largest stride (the same size and non-zero count): spmv_schedule reports the new unit,
    the launch takes the new table's grid, and the bits are those of the host restatement and of the cycle"""
    dtype = np.float64
    ctx = gpu[0]
    n = 70001
    other = ((-310, -10, -1, 0, 1, 10, 310), RP.STENCIL7[1])
    h1 = RC.host(("xcd-st7", n, "f64"), lambda: RC.stencil_matrix(n, *RP.STENCIL7, np.float64), dtype)
    h2 = RC.host(("xcd-st7-310", n, "f64"), lambda: RC.stencil_matrix(n, *other, np.float64), dtype)
    assert len(h1["mat"][1]) == len(h2["mat"][1]) and not np.array_equal(h1["mat"][0], h2["mat"][0])
    assert plane_grid(n, 300)[1] != plane_grid(n, 310)[1]
    out = {}
    for plane in (1, 0):
        tuned(dev_spmv_plane=plane)
        ip, ix, da = h1["mat"]
        s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype)
        try:
            kind = "plane" if plane else "cycle"
            want = RP.want_form("rowpair", h1)
            if plane:
                want = dict(want, grid=plane_grid(n, 300)[0])
            assert s.spmv_schedule == {"kind": kind, "grid": want["grid"], "unit_rows": 300}, s.spmv_schedule
            RC.verify(f"before reload {kind}", h1, dtype, RC.spmv_both(pkg, ctx, s, h1, dtype), want)
            ip2, ix2, da2 = h2["mat"]
            s.reload_matrix(da2, ip2, ix2)
            want = RP.want_form("rowpair", h2)
            if plane:
                want = dict(want, grid=plane_grid(n, 310)[0])
            assert s.row_pairs > 0
            assert s.spmv_schedule == {"kind": kind, "grid": want["grid"], "unit_rows": 310}, s.spmv_schedule
            out[plane] = RC.verify(f"after reload {kind}", h2, dtype, RC.spmv_both(pkg, ctx, s, h2, dtype), want)
        finally:
            s.close()
    assert R.bit_equal(out[1][0], out[0][0]) and R.bit_equal(out[1][1], out[0][1])
