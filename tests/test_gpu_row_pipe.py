"""The gather pipeline of the row-coded SpMV (csrc/spmv.hip spmv_rowcode_kernel<..., DEPTH>; include/cgamd.h cgamd_solver_row_pipe):
dev.row_pipe = 1, 2 and 4 keep one, two and all four row blocks' gathers of a work-group in flight per wave.  Only the order of issue
changes: every depth forms the same products in the same order from the same bits, so every case is compared BIT FOR BIT with the host
restatement of tests/spmv_ref.py (spmv_in_type for y, block_partials_in_type for the fused d.q partials), after asserting -- through
Solver.last_spmv_form(), recorded at the launch site, and Solver.row_pipe -- that the row-coded form ran at the depth the case is
written for.  y is prefilled with NaN, x carries adversarial magnitudes (spmv_ref.adversarial_d).  Matrices, the host side (computed
once per case and shared) and the device side are the ones of test_gpu_row_codes.py."""
import numpy as np
import pytest

import spmv_ref as R
import test_gpu_row_codes as RC

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 4)
FOUR_LAUNCH = {"two_launch": 0, "dev.no_fold_alpha": 1, "resident_wide": 0}      # the four-launch loop at a small size (test_gpu_x_lag.py)
# struct Tuning's defaults (csrc/cgamd_internal.h) of every key this module sets
DEFAULTS = dict(RC.DEFAULTS, **{"dev.row_pipe": 0, "dev.no_fold_alpha": 0})
BASE = RC.BASE      # resident = 0, index_codes_min_mb = 0, dev.row_codes_min_mb = 0


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


def run_depth(pkg, ctx, label, h, dtype, depth, nt=0):
    """one handle created under dev.row_pipe = depth: the form and the depth first, then the bits, plain and fused"""
    ip, ix, da = h["mat"]
    s = pkg.Solver(ctx, h["n"], len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        assert s.row_codes > 0 and s.row_pipe == depth, (s.row_codes, s.row_pipe, depth)
        runs = RC.spmv_both(pkg, ctx, s, h, dtype)
        assert all(r[2]["family"] == "rowcode" for r in runs), runs[0][2]
        return RC.verify(f"{label} depth{depth}", h, dtype, runs, RC.expected_form("rowcode", h["n"], h["max_row"], nt))
    finally:
        s.close()


def every_depth(pkg, ctx, tuned, label, h, dtype, nts=(0,)):
    out = []
    for nt in nts:
        for depth in DEPTHS:
            tuned(dev_row_pipe=depth, spmv_nt=nt)
            out.append(run_depth(pkg, ctx, f"{label} nt{nt}", h, dtype, depth, nt))
    assert all(R.bit_equal(y, out[0][0]) and R.bit_equal(p, out[0][1]) for y, p in out[1:])
    return out[0]


# ---- 1. ragged last work-group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [5, 6, 7, 8])
@pytest.mark.parametrize("dt", list(RC.DT))
def test_ragged_last_work_group(pkg, gpu, tuned, dt, blocks):
    """5 to 8 row blocks, the last one 5 rows short: the second work-group of four holds 1, 2, 3 and 4 row blocks.  Blocks past the last
    one issue their gathers with length 0 on a clamped row and store nothing"""
    dtype = RC.DT[dt]
    n = 256 * blocks - 5
    assert (n + 255) // 256 == blocks and n % 256 != 0
    offs, vals = (-300, -20, -1, 0, 1, 20, 300), (-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0)
    h = RC.host(("pipe-ragged", dt, blocks), lambda: RC.stencil_matrix(n, offs, vals, np.float64), dtype)
    assert h["max_row"] == 7
    every_depth(pkg, gpu[0], tuned, f"ragged {dt} blocks{blocks}", h, dtype, nts=(0, 1))


# ---- 2. waves of one pattern and of several ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(23, 19, 31), (130, 5, 4)], ids=["23x19x31", "130x5x4"])
def test_mixed_uniform_and_non_uniform_waves(pkg, gpu, tuned, grid):
    """x-runs of 23 rows: no wave of one pattern; of 130 rows: waves of one pattern beside waves of 2 to 4"""
    import cg_numpy
    dtype = np.float64
    h = RC.host(("pipe-lap3d", grid), lambda: cg_numpy.laplace3d(*grid), dtype)
    key = RC.row_pattern_ids(*h["mat"])[0]
    per_wave = [len(set(key[w:w + 64].tolist())) for w in range(0, h["n"] - 63, 64)]
    assert max(per_wave) >= 2 and ((1 in per_wave) == (grid == (130, 5, 4)))
    every_depth(pkg, gpu[0], tuned, f"lap3d {grid}", h, dtype)


# ---- 3. uniform waves shorter than 7 -------------------------------------------------------------------------------------------------
def test_uniform_waves_shorter_than_7(pkg, gpu, tuned):
    """the 3-point stencil: every inner wave has one pattern of 3 entries, its slots 3 to 6 gather the row's own entry and are dropped"""
    dtype = np.float64
    h = RC.host(("pipe-3pt",), lambda: RC.stencil_matrix(1021, (-1, 0, 1), (-1.25, 2.5, -1.125), dtype), dtype)
    assert h["max_row"] == 3
    key = RC.row_pattern_ids(*h["mat"])[0]
    assert len(set(key[64:128].tolist())) == 1
    every_depth(pkg, gpu[0], tuned, "3-point", h, dtype)


# ---- 4. empty rows ---------------------------------------------------------------------------------------------------------------------
def test_a_whole_wave_of_empty_rows(pkg, gpu, tuned):
    """rows 256 ... 319 emptied: a uniform wave of length 0, every slot dropped; these rows come out exactly +0 in the NaN-prefilled y"""
    import cg_numpy
    dtype = np.float64
    gone = list(range(256, 320))
    h = RC.host(("pipe-empty",), lambda: RC.empty_rows(cg_numpy.laplace3d(130, 5, 4), gone), dtype)
    L = np.diff(h["mat"][0])
    assert (L[256:320] == 0).all() and (L == 0).sum() == 64
    for depth in DEPTHS:
        tuned(dev_row_pipe=depth)
        y, _ = run_depth(pkg, gpu[0], "empty wave", h, dtype, depth)
        assert np.all(R.bits(y[0][256:320]) == 0)


# ---- 5. the loop -----------------------------------------------------------------------------------------------------------------------
def test_the_loop_is_bit_identical_at_every_depth(pkg, gpu, tuned):
    """30 iterations of the four-launch loop on 24 000 rows, fp64: the history and x of depths 2 and 4 and of a handle created under the
    default equal those of depth 1"""
    import cg_numpy
    dtype = np.float64
    ctx = gpu[0]
    lib = pkg._lib.load()
    ip, ix, da = RC.in_type(cg_numpy.laplace3d(40, 30, 20), dtype)
    n = len(ip) - 1
    got = {}
    for depth in (1, 2, 4, 0):
        tuned(dev_row_pipe=depth, **FOUR_LAUNCH)
        s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype)
        try:
            assert s.row_codes == 27 and lib.cgamd_solver_loop_launches(s.handle) == 4
            assert s.row_pipe in DEPTHS and (depth == 0 or s.row_pipe == depth), (s.row_pipe, depth)
            s.set_rhs(np.linspace(1.0, 2.0, n).astype(dtype))
            s.iterate(30)
            ctx.synchronize()
            assert s.last_spmv_form()["family"] == "rowcode", s.last_spmv_form()
            got[depth] = (s.history().copy(), s.x().copy())
        finally:
            s.close()
    assert got[1][0].shape == (31, 1) and np.all(np.isfinite(got[1][0]))
    for depth in (2, 4, 0):
        assert np.array_equal(got[depth][0], got[1][0]), f"depth {depth}: the history differs from depth 1"
        assert np.array_equal(got[depth][1], got[1][1]), f"depth {depth}: x differs from depth 1"
