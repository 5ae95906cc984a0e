"""The row-pair form of the row-coded SpMV (csrc/spmv.hip spmv_rowpair_kernel; include/cgamd.h cgamd_solver_row_pairs): a lane owns rows
2t and 2t + 1, one byte per PAIR of rows names the union of the two rows' slots, and one 16-byte load per slot serves both rows.  Each
row's sum is still formed from zero in its stored order from the bits of the row dictionary, and the d.q partials follow the tree of
block_sum<256>, so every case is compared BIT FOR BIT with the host restatement of tests/spmv_ref.py (spmv_in_type for y,
block_partials_in_type for the fused partials) after asserting -- through Solver.last_spmv_form(), recorded at the launch site, and
Solver.row_pairs -- that the pair form ran.  y is prefilled with NaN, x carries adversarial magnitudes.  Every case also runs under
dev.row_pairs = 0 (the row form) and the two results are compared bit for bit.  Matrices, the host side (computed once per case and
shared) and the device side are the ones of test_gpu_row_codes.py."""
import numpy as np
import pytest

import spmv_ref as R
import test_gpu_row_codes as RC
import test_row_pairs_merge as M

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 4)          # dev.row_pipe; the pair form keeps min(depth, 2) passes in flight
FOUR_LAUNCH = {"two_launch": 0, "dev.no_fold_alpha": 1, "resident_wide": 0}
# struct Tuning's defaults (csrc/cgamd_internal.h) of every key this module sets
DEFAULTS = dict(RC.DEFAULTS, **{"dev.row_pipe": 0, "dev.no_fold_alpha": 0, "pad_rows": 1, "dev.row_pairs": -1, "dev.row_pairs_min_mb": 256})
BASE = dict(RC.BASE, **{"dev.row_pairs": 1, "dev.row_pairs_min_mb": 0})
STENCIL7 = ((-300, -20, -1, 0, 1, 20, 300), (-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0))


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


def want_form(family, h, nt=0):
    return dict(RC.expected_form("rowcode", h["n"], h["max_row"], nt), family=family)


def pair_patterns(ip, ix, da, n_rows=None):
    """the distinct (pattern of row 2p, pattern of row 2p + 1) of the n_rows rows the handle carries (rows past the matrix: empty), and
    the longest union of slots among them (None where one does not fit 8 slots)"""
    n = len(ip) - 1
    n_rows = n if n_rows is None else n_rows
    ids = RC.row_pattern_ids(ip, ix, da)[0].tolist() + [-1] * (n_rows - n + 1)
    offs = [tuple((ix[ip[i]:ip[i + 1]] - i).tolist()) for i in range(n)] + [()] * (n_rows - n + 1)
    empty = {i for i in range(n) if ip[i] == ip[i + 1]}
    key = lambda r: -1 if (r >= n or r in empty) else ids[r]
    seen = {}
    for r in range(0, n_rows, 2):
        seen.setdefault((key(r), key(r + 1)), (offs[r], offs[r + 1]))
    longest = 0
    for a, b in seen.values():
        m = M.merge(a, b)
        if m[0] == "long":
            return len(seen), None
        longest = max(longest, len(m[1]))
    return len(seen), longest


def run_form(pkg, ctx, label, h, dtype, family, nt=0, pairs=None):
    """one handle under the tuning in force: what it says about itself, the form, then the bits, plain and fused"""
    ip, ix, da = h["mat"]
    s = pkg.Solver(ctx, h["n"], len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        assert s.row_codes > 0
        if family == "rowpair":
            assert s.row_pairs > 0 and (pairs is None or s.row_pairs == pairs), (s.row_pairs, pairs)
        else:
            assert s.row_pairs == 0
        runs = RC.spmv_both(pkg, ctx, s, h, dtype)
        assert all(r[2]["family"] == family for r in runs), runs[0][2]
        return RC.verify(label, h, dtype, runs, want_form(family, h, nt))
    finally:
        s.close()


def pairs_and_rows(pkg, ctx, tuned, label, h, dtype, nts=(0,), pads=(1,), depths=DEPTHS, pairs=None):
    """the pair form at every setting asked for, then the row form: the same y and partials bit for bit"""
    out = []
    for pad in pads:
        for nt in nts:
            for depth in depths:
                tuned(dev_row_pipe=depth, spmv_nt=nt, pad_rows=pad)
                out.append(run_form(pkg, ctx, f"{label} pad{pad} nt{nt} depth{depth}", h, dtype, "rowpair", nt, pairs))
    tuned(dev_row_pairs=0)
    out.append(run_form(pkg, ctx, f"{label} row form", h, dtype, "rowcode"))
    assert all(R.bit_equal(y, out[0][0]) and R.bit_equal(p, out[0][1]) for y, p in out[1:])
    return out[0]


# ---- 1. ragged ends ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [5, 6, 7, 8])
@pytest.mark.parametrize("dt", list(RC.DT))
def test_ragged_ends(pkg, gpu, tuned, dt, blocks):
    """n = 256 b - 5 (odd): the second work-group holds 1 to 4 row blocks; rows 0 and n - 1 bring both address clamps (row 1's slot -1
    shares its load with nothing of row 0 at element -1; the last row's slot 0 would read x[n] in its upper half); pad_rows = 0 leaves
    the lone last row, which pairs with an empty partner and stores 8 bytes"""
    dtype = RC.DT[dt]
    n = 256 * blocks - 5
    h = RC.host(("pipe-ragged", dt, blocks), lambda: RC.stencil_matrix(n, *STENCIL7, np.float64), dtype)
    assert h["n"] % 2 == 1 and h["max_row"] == 7
    pairs_and_rows(pkg, gpu[0], tuned, f"ragged {dt} blocks{blocks}", h, dtype, nts=(0, 1), pads=(1, 0))


# ---- 2. patterns that differ inside a pair --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(23, 19, 31), (130, 5, 4)], ids=["23x19x31", "130x5x4"])
def test_patterns_differ_inside_a_pair(pkg, gpu, tuned, grid):
    """nx = 23 is odd: pairs straddle grid lines, so the two rows of a pair carry different patterns (the union still has 7 slots);
    130 x 5 x 4: pairs inside the lines, boundary rows beside interior ones"""
    import cg_numpy
    dtype = np.float64
    h = RC.host(("pipe-lap3d", grid), lambda: cg_numpy.laplace3d(*grid), dtype)
    ip, ix, da = h["mat"]
    ids = RC.row_pattern_ids(ip, ix, da)[0]
    assert (ids[0:h["n"] - 1:2] != ids[1:h["n"]:2]).any()
    count, longest = pair_patterns(ip, ix, da, h["n"] + h["n"] % 2)
    assert longest == 7 and 27 <= count <= 256
    pairs_and_rows(pkg, gpu[0], tuned, f"lap3d {grid}", h, dtype, pairs=count)


# ---- 3. values that differ inside a pair -------------------------------------------------------------------------------------------------
def _three_point_mod3(n, dtype):
    ip, ix, da = RC.stencil_matrix(n, (-1, 0, 1), (-1.25, 2.5, -1.125), dtype)
    rows = np.repeat(np.arange(n), np.diff(ip))
    return ip, ix, da * (1.0 + 0.25 * (rows % 3))


def test_values_differ_inside_a_pair(pkg, gpu, tuned):
    """the 3-point stencil with coefficients that depend on i % 3: the same offsets in both rows of a pair, other values (val0 != val1)"""
    dtype = np.float64
    h = RC.host(("pairs-mod3",), lambda: _three_point_mod3(1021, dtype), dtype)
    ip, ix, da = h["mat"]
    assert da[ip[2] + 1] != da[ip[3] + 1] and ix[ip[2] + 1] == 2 and ix[ip[3] + 1] == 3
    pairs_and_rows(pkg, gpu[0], tuned, "3-point mod 3", h, dtype)


# ---- 4. unused slots ---------------------------------------------------------------------------------------------------------------------
def test_unused_slots(pkg, gpu, tuned):
    """the plain 3-point stencil: unions of 3 slots, slots 3 to 6 load the pair's own entries and are dropped"""
    dtype = np.float64
    h = RC.host(("pipe-3pt",), lambda: RC.stencil_matrix(1021, (-1, 0, 1), (-1.25, 2.5, -1.125), dtype), dtype)
    assert h["max_row"] == 3 and pair_patterns(*h["mat"], 1022)[1] == 3
    pairs_and_rows(pkg, gpu[0], tuned, "3-point", h, dtype)


# ---- 5. empty rows ------------------------------------------------------------------------------------------------------------------------
def test_empty_rows(pkg, gpu, tuned):
    """rows 256 ... 319 emptied -- pairs of two empty rows -- and row 1001 alone -- a pair with one empty row: all of them exactly +0"""
    import cg_numpy
    dtype = np.float64
    gone = list(range(256, 320)) + [1001]
    h = RC.host(("pairs-empty",), lambda: RC.empty_rows(cg_numpy.laplace3d(130, 5, 4), gone), dtype)
    L = np.diff(h["mat"][0])
    assert (L[gone] == 0).all() and (L == 0).sum() == len(gone) and L[1000] > 0
    y, _ = pairs_and_rows(pkg, gpu[0], tuned, "empty rows", h, dtype)
    assert np.all(R.bits(y[0][gone]) == 0)


# ---- 6. stored order -----------------------------------------------------------------------------------------------------------------------
def test_stored_order_that_fits_8_slots(pkg, gpu, tuned):
    """odd rows store their last two entries the other way round: the union of a pair needs 8 slots (the 8-slot kernel), and each row
    is still summed in ITS stored order -- not the sorted one, which has other bits on this x"""
    dtype = np.float64
    offs, vals = (-64, -8, -1, 0, 1, 8, 64), (-1.25, -0.75, -1.5, 6.5, -1.125, -0.875, -1.375)
    n = 1021
    h = RC.host(("pairs-order8",), lambda: RC.stencil_matrix(n, offs, vals, dtype, order=lambda i: range(7) if i % 2 == 0 else (0, 1, 2, 3, 4, 6, 5)), dtype)
    ip, ix, da = h["mat"]
    assert pair_patterns(ip, ix, da, n + 1)[1] == 8
    rows = np.repeat(np.arange(n), np.diff(ip))
    perm = np.lexsort((ix, rows))
    y_sorted = R.spmv_in_type(ip, ix[perm], da[perm], h["x"], dtype)
    assert not R.bit_equal(y_sorted, h["y"]), "the two host walks agree: the case would pass vacuously"
    y, _ = pairs_and_rows(pkg, gpu[0], tuned, "stored order, 8 slots", h, dtype)
    assert not R.bit_equal(y, y_sorted)


def test_stored_order_that_does_not_fit(pkg, gpu, tuned):
    """even rows ascending, odd rows descending: the shortest common supersequence of a pair has 13 slots, the handle keeps the row form"""
    dtype = np.float64
    offs, vals = (-64, -8, -1, 0, 1, 8, 64), (-1.25, -0.75, -1.5, 6.5, -1.125, -0.875, -1.375)
    n = 1021
    h = RC.host(("order",), lambda: RC.stencil_matrix(n, offs, vals, dtype, order=lambda i: range(7) if i % 2 == 0 else range(6, -1, -1)), dtype)
    assert pair_patterns(*h["mat"], n + 1)[1] is None
    tuned()
    run_form(pkg, gpu[0], "stored order, too long", h, dtype, "rowcode")


# ---- 7. a caller's vector that is not 16-byte aligned ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["x", "y"])
def test_unaligned_caller_vector_runs_the_row_form(pkg, gpu, tuned, which):
    """x (or y) 8-byte but not 16-byte aligned: the launch takes the row form, and the result is the host's"""
    import torch
    dtype = np.float64
    ctx = gpu[0]
    h = RC.host(("pipe-ragged", "f64", 5), lambda: RC.stencil_matrix(256 * 5 - 5, *STENCIL7, np.float64), dtype)
    ip, ix, da = h["mat"]
    n = h["n"]
    tuned()
    s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        assert s.row_pairs > 0
        dev = torch.device("cuda", 0)
        xbuf = torch.zeros(n + 2, dtype=torch.float64, device=dev)
        ybuf = torch.from_numpy(np.full(n + 2, np.nan)).to(dev)
        ox, oy = (1, 0) if which == "x" else (0, 1)
        xd, yd = xbuf[ox:ox + n], ybuf[oy:oy + n]
        xd.copy_(torch.from_numpy(np.ascontiguousarray(h["x"].reshape(-1))))
        assert xbuf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0 and (xd.data_ptr() % 16, yd.data_ptr() % 16) == (8 * ox, 8 * oy)
        torch.cuda.synchronize()
        s.spmv(xd, yd, fused_dot=False)
        form = s.last_spmv_form()
        ctx.synchronize()
        assert form["family"] == "rowcode", form
        assert R.bit_equal(yd.cpu().numpy().reshape(1, n), h["y"])
    finally:
        s.close()


# ---- 8. the loop ----------------------------------------------------------------------------------------------------------------------------
def test_the_loop_is_bit_identical(pkg, gpu, tuned):
    """30 iterations of the four-launch loop on 24 000 rows, fp64, x lag by the default rule: history and x of the pair form at every
    depth equal those of the row form"""
    import cg_numpy
    dtype = np.float64
    ctx = gpu[0]
    lib = pkg._lib.load()
    ip, ix, da = RC.in_type(cg_numpy.laplace3d(40, 30, 20), dtype)
    n = len(ip) - 1
    got = {}
    for key, kv in [(("pairs", d), {"dev.row_pipe": d}) for d in DEPTHS] + [(("rows", 0), {"dev.row_pairs": 0})]:
        tuned(**kv, **FOUR_LAUNCH)
        s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype)
        try:
            assert s.row_codes == 27 and lib.cgamd_solver_loop_launches(s.handle) == 4
            assert (s.row_pairs == 27) == (key[0] == "pairs") and (s.row_pairs == 0) == (key[0] == "rows"), s.row_pairs
            s.set_rhs(np.linspace(1.0, 2.0, n).astype(dtype))
            s.iterate(30)
            ctx.synchronize()
            assert s.last_spmv_form()["family"] == ("rowpair" if key[0] == "pairs" else "rowcode"), s.last_spmv_form()
            got[key] = (s.history().copy(), s.x().copy(), lib.cgamd_solver_x_lag(s.handle))
        finally:
            s.close()
    ref = got[("rows", 0)]
    assert ref[0].shape == (31, 1) and np.all(np.isfinite(ref[0]))
    for d in DEPTHS:
        assert got[("pairs", d)][2] == ref[2]
        assert R.bit_equal(got[("pairs", d)][0], ref[0]), f"depth {d}: the history differs from the row form's"
        assert R.bit_equal(got[("pairs", d)][1], ref[1]), f"depth {d}: x differs from the row form's"


# ---- 9. refresh -------------------------------------------------------------------------------------------------------------------------------
def test_refresh_rewrites_the_pair_dictionary_in_place(pkg, gpu, tuned):
    """rescaled coefficients: refresh_values reports outcome 1 (dictionaries rewritten in place), and the handle then computes what a
    fresh handle on the new values computes, bit for bit"""
    import cg_numpy
    dtype = np.float64
    ctx = gpu[0]
    h = RC.host(("pipe-lap3d", (130, 5, 4)), lambda: cg_numpy.laplace3d(130, 5, 4), dtype)
    ip, ix, da = h["mat"]
    da2 = (da * 2.5 + np.where(da > 0, 0.125, 0.0)).astype(dtype)      # every class of equal values stays one; not a power-of-two scaling
    h2 = dict(h, mat=(ip, ix, da2), ext=R.spmv_ext(ip, ix, da2, h["x"], dtype), y=R.spmv_in_type(ip, ix, da2, h["x"], dtype))
    h2["parts"] = R.block_partials_in_type(h["x"][0], h2["y"][0], dtype)
    tuned()
    s = pkg.Solver(ctx, h["n"], len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        pairs = s.row_pairs
        assert pairs > 0
        RC.verify("before refresh", h, dtype, RC.spmv_both(pkg, ctx, s, h, dtype), want_form("rowpair", h))
        s.refresh_values(da2)
        assert s.last_refresh == 1 and s.row_pairs == pairs
        y1, p1 = RC.verify("after refresh", h2, dtype, RC.spmv_both(pkg, ctx, s, h2, dtype), want_form("rowpair", h2))
    finally:
        s.close()
    y2, p2 = run_form(pkg, ctx, "fresh handle", h2, dtype, "rowpair", pairs=pairs)
    assert R.bit_equal(y1, y2) and R.bit_equal(p1, p2)
