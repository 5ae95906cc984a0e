"""Row-pattern codes of the single-RHS SpMV (include/cgamd.h: cgamd_solver_row_codes; csrc/spmv.hip spmv_rowcode_kernel): one byte per
ROW names the row's sequence of (offset, value) pairs in stored order.  It is a re-encoding: the kernel forms the same products in
the same order from the same bits as every one-lane-per-row form, so every case is compared BIT FOR BIT with the host restatement of
tests/spmv_ref.py (spmv_in_type for y, block_partials_in_type for the fused d.q partials), after asserting -- through
Solver.last_spmv_form(), recorded at the launch site -- that the form the case is written for really ran.  y is prefilled with NaN;
rows without entries must come out exactly +0 (check_rows).  x carries adversarial magnitudes (spmv_ref.adversarial_d), so another
order of summation has other bits."""
import zlib

import numpy as np
import pytest

import spmv_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64}

# struct Tuning's defaults (csrc/cgamd_internal.h) of every key this module sets
DEFAULTS = {"index_codes": 1, "index_codes_min_mb": 32, "resident": 1, "resident_wide": 1, "two_launch": 1, "spmv_nt": -1, "spmv_cycle": 64,
            "dev.value_codes": 1, "dev.vc_pipe": 1, "dev.joint_codes": 1, "dev.row_codes": 1, "dev.row_codes_min_mb": 32}
BASE = {"resident": 0, "index_codes_min_mb": 0, "dev.row_codes_min_mb": 0}      # no resident loop (such handles build no codes); codes at any size


@pytest.fixture
def tuned(pkg):
    """sets tuning keys BEFORE a handle is created (a handle keeps the configuration it was created under); every call starts from
    the defaults plus BASE (base=False: from the defaults alone); the defaults are restored afterwards"""
    lib = pkg._lib.load()

    def put(kv):
        for k, v in kv.items():
            assert k in DEFAULTS, k
            pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))

    def tune(base=True, **kv):
        put(DEFAULTS)
        if base:
            put(BASE)
        put({k.replace("dev_", "dev."): v for k, v in kv.items()})
    yield tune
    put(DEFAULTS)


# ---- expected forms (the launcher's own arithmetic, restated) -------------------------------------------------------------------------
def rowblock_grid(row_blocks, cycle):
    if cycle > 1:
        return 8 * ((cycle + 7) // 8) * ((row_blocks + cycle - 1) // cycle)
    return 8 * max((x + 1) * row_blocks // 8 - x * row_blocks // 8 for x in range(8))


def fit_unroll(max_row):
    return 4 if max_row <= 4 else 5 if max_row == 5 else 7 if max_row <= 7 else 8


def expected_form(family, n, max_row, nt=0, cycle=64):
    """"rowcode": family 7, value_codes 3; "joint": the vcp kernel on joint codes.  Both walk four row blocks per work-group."""
    rb = (n + 255) // 256
    return {"family": "rowcode" if family == "rowcode" else "vcp", "vec": 1, "width": fit_unroll(max_row), "index_bits": 8,
            "value_codes": 3 if family == "rowcode" else 2, "nt": nt, "fused": 0, "wide": 0,
            "grid": rowblock_grid((rb + 3) // 4, max(1, cycle // 4)), "partials": rb}


# ---- matrices ------------------------------------------------------------------------------------------------------------------------
def stencil_matrix(n, offsets, values, dtype, order=None):
    """row i holds (i + off, value) for the offsets that stay inside the matrix, in the order given (`order(i)`: a permutation of the
    offsets for row i, or None)"""
    ip = np.zeros(n + 1, dtype=np.int32)
    ix, da = [], []
    for i in range(n):
        seq = range(len(offsets)) if order is None else order(i)
        for k in seq:
            c = i + offsets[k]
            if 0 <= c < n:
                ix.append(c)
                da.append(values[k])
        ip[i + 1] = len(ix)
    return ip, np.asarray(ix, dtype=np.int32), np.asarray(da, dtype=dtype)


def empty_rows(mat, rows):
    """the matrix with the entries of `rows` removed"""
    ip, ix, da = mat
    n = len(ip) - 1
    L = np.diff(ip).astype(np.int64)
    keep = np.ones(len(ix), dtype=bool)
    for r in rows:
        keep[ip[r]:ip[r + 1]] = False
        L[r] = 0
    ip2 = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(L, out=ip2[1:])
    return ip2, ix[keep], da[keep]


def row_pattern_ids(ip, ix, da):
    """per row: a number for its sequence of (offset, value bits) in stored order, and one for the SET of them"""
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    off = (np.asarray(ix, dtype=np.int64) - rows).tolist()
    vb = [tuple(b) for b in R.bits(np.asarray(da)).reshape(len(off), -1).tolist()]
    seqs, sets = {}, {}
    seq_id, set_id = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for i in range(n):
        seq = tuple(zip(off[ip[i]:ip[i + 1]], vb[ip[i]:ip[i + 1]]))
        seq_id[i] = seqs.setdefault(seq, len(seqs))
        set_id[i] = sets.setdefault(frozenset(seq), len(sets))
    return seq_id, set_id


def row_patterns(ip, ix, da):
    """(distinct rows as sequences in stored order, distinct rows as sets)"""
    seq_id, set_id = row_pattern_ids(ip, ix, da)
    return len(set(seq_id.tolist())), len(set(set_id.tolist()))


def in_type(mat, dtype):
    ip, ix, da = mat
    if np.dtype(dtype).kind == "c":
        da = da * (1.0 + 0.25j)          # complex symmetric, still few distinct entries (as test_value_codes_change_no_bit makes them)
    return np.asarray(ip, dtype=np.int32), np.asarray(ix, dtype=np.int32), np.asarray(da).astype(dtype)


# ---- host side of a case, computed once per (matrix, x) and shared -------------------------------------------------------------------
_HOST = {}


def host(key, build, dtype):
    if key not in _HOST:
        ip, ix, da = in_type(build(), dtype)
        n = len(ip) - 1
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        x = R.adversarial_d(rng, n, dtype).reshape(1, n)
        y = R.spmv_in_type(ip, ix, da, x, dtype)
        _HOST[key] = {"mat": (ip, ix, da), "x": x, "n": n, "max_row": int(np.diff(ip).max()), "ext": R.spmv_ext(ip, ix, da, x, dtype), "y": y,
                      "parts": R.block_partials_in_type(x[0], y[0], dtype)}
    return _HOST[key]


# ---- device side ---------------------------------------------------------------------------------------------------------------------
def nan_vector(n, dtype):
    import torch
    v = np.full(n, np.nan, dtype=dtype)
    if np.dtype(dtype).kind == "c":
        v = (v + 1j * v).astype(dtype)
    return torch.from_numpy(v).to(torch.device("cuda", 0))


def spmv_both(pkg, ctx, s, h, dtype):
    """the handle's SpMV on the case's x, plain and fused, y prefilled with NaN -> [(fused, y, form, partials)]"""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(h["x"].reshape(-1))).to(torch.device("cuda", 0))
    out = []
    try:
        for f in (False, True):
            yd = nan_vector(h["n"], dtype)
            torch.cuda.synchronize()
            s.spmv(xd, yd, fused_dot=f)
            form = s.last_spmv_form()
            ctx.synchronize()
            out.append((f, yd.cpu().numpy().reshape(1, h["n"]), form, s.dot_partials() if f else None))
    except pkg.CgAmdError as e:
        if e.status == pkg._lib.ERR_HIP:       # a kernel faulted: nothing more is started on that device in this session
            pytest.exit(f"HIP error in an SpMV launch, the session ends here: {e}", returncode=3)
        raise
    return out


def verify(label, h, dtype, runs, want_form):
    """the form first; then every row within the bound and empty rows +0, y and the partials bit-equal to the host restatement"""
    ip, ix, da = h["mat"]
    for f, y, form, parts in runs:
        want = dict(want_form, fused=int(f), partials=want_form["partials"] if f else 0)
        print(f"{label} fused={int(f)}: ran {form}")
        assert form == want, f"{label}: launched {form}, the case is written for {want}"
        R.check_rows(y, ip, ix, da, h["x"], dtype, ext=h["ext"], label=label)
        diff = np.argwhere(R.bits(y) != R.bits(h["y"]))
        assert diff.size == 0, f"{label}: {len(diff)} values differ from the host restatement, first at {diff[0].tolist()}"
        if f:
            assert parts.shape == (1, want["partials"])
            bad = np.nonzero(np.any((R.bits(parts[0]) != R.bits(h["parts"])).reshape(len(h["parts"]), -1), axis=1))[0]
            assert bad.size == 0, f"{label}: d.q partials of blocks {bad.tolist()[:8]} differ from the restated block sum"
    return runs[0][1], runs[1][3]


def run_case(pkg, ctx, label, h, dtype, family, nt=0, cycle=64, patterns=None):
    """one handle on the case's matrix: the form, the bits, and what the handle says about itself"""
    ip, ix, da = h["mat"]
    s = pkg.Solver(ctx, h["n"], len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        if patterns is not None:
            assert s.row_codes == patterns, (s.row_codes, patterns)
        V = np.dtype(dtype).itemsize
        if family == "rowcode":
            assert s.row_codes > 0 and s.joint_codes > 0
            assert s.spmv_moved_bytes == h["n"] * 1 + 2 * h["n"] * V          # one code byte per row, x, y: no per-non-zero bytes, no row pointers
        else:
            assert s.row_codes == 0
            assert s.spmv_moved_bytes == len(ix) * 1 + (h["n"] + 1) * 4 + 2 * h["n"] * V
        assert s.iter_moved_bytes - s.spmv_moved_bytes == 8 * h["n"] * V      # the vector passes do not change with the SpMV form
        y, parts = verify(label, h, dtype, spmv_both(pkg, ctx, s, h, dtype), expected_form(family, h["n"], h["max_row"], nt, cycle))
    finally:
        s.close()
    return y, parts


def both_forms(pkg, ctx, tuned, label, h, dtype, patterns):
    """row codes, then dev.row_codes = 0: the joint vcp form, the same y and partials bit for bit"""
    tuned()
    y1, p1 = run_case(pkg, ctx, label, h, dtype, "rowcode", patterns=patterns)
    tuned(dev_row_codes=0)
    y0, p0 = run_case(pkg, ctx, label + " joint", h, dtype, "joint")
    assert R.bit_equal(y1, y0) and R.bit_equal(p1, p0)


# ---- 1. uniform and mixed waves, ragged end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(130, 5, 4), (131, 5, 3)], ids=["130x5x4", "131x5x3"])
@pytest.mark.parametrize("dt", list(DT))
def test_uniform_and_mixed_waves(pkg, gpu, tuned, dt, grid):
    """x-runs of 130 / 131 rows: waves of one pattern, waves of 2 to 4 patterns, a last block and a last wave that are not full;
    1 965 rows is odd, so the handle appends empty rows (pad_rows): they take the length-0 pattern and nothing of them is seen"""
    import cg_numpy
    dtype = DT[dt]
    h = host(("lap3d", dt, grid), lambda: cg_numpy.laplace3d(*grid), dtype)
    ip, ix, da = h["mat"]
    n = h["n"]
    assert n == {(130, 5, 4): 2600, (131, 5, 3): 1965}[grid] and n % 256 != 0 and n % 64 != 0
    assert row_patterns(ip, ix, da)[0] == 27
    # waves (64 rows from a multiple of 64) of one pattern and of several exist
    key = row_pattern_ids(ip, ix, da)[0]
    per_wave = [len(set(key[w:w + 64].tolist())) for w in range(0, n - 63, 64)]
    assert 1 in per_wave and max(per_wave) >= 2
    both_forms(pkg, gpu[0], tuned, f"lap3d {dt} {grid}", h, dtype, 27)


# ---- 2. no uniform wave at all ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lap3d-23x19x31", "poisson2d-150"])
def test_no_uniform_wave(pkg, gpu, tuned, kind):
    """x-runs of 23 rows (shorter than a wave) / the 5-point grid of 150 x 150: 9 patterns, batch length 5"""
    import cg_numpy
    build = (lambda: cg_numpy.laplace3d(23, 19, 31)) if kind.startswith("lap3d") else (lambda: cg_numpy.poisson2d(150))
    h = host(("nouni", kind), build, np.float64)
    want = 27 if kind.startswith("lap3d") else 9
    assert row_patterns(*h["mat"])[0] == want and h["max_row"] == (7 if want == 27 else 5)
    both_forms(pkg, gpu[0], tuned, kind, h, np.float64, want)


# ---- 3. stored order is part of the pattern -----------------------------------------------------------------------------------------
def test_stored_order_is_part_of_the_pattern(pkg, gpu, tuned):
    """a 7-point pattern whose even rows are stored by ascending and whose odd rows by descending column: the same sets, other
    sequences.  The device walks the stored order -- not the sorted one, which has other bits on this x"""
    dtype = np.float64
    offs, vals = (-64, -8, -1, 0, 1, 8, 64), (-1.25, -0.75, -1.5, 6.5, -1.125, -0.875, -1.375)
    n = 1021
    h = host(("order",), lambda: stencil_matrix(n, offs, vals, dtype, order=lambda i: range(7) if i % 2 == 0 else range(6, -1, -1)), dtype)
    ip, ix, da = h["mat"]
    seqs, sets = row_patterns(ip, ix, da)
    assert seqs > sets and seqs <= 256
    # the same matrix with every row sorted by column: the other host walk
    rows = np.repeat(np.arange(n), np.diff(ip))
    perm = np.lexsort((ix, rows))
    y_sorted = R.spmv_in_type(ip, ix[perm], da[perm], h["x"], dtype)
    assert not R.bit_equal(y_sorted, h["y"]), "the two host walks agree: the case would pass vacuously"
    tuned()
    y, _ = run_case(pkg, gpu[0], "stored order", h, dtype, "rowcode", patterns=seqs)
    assert R.bit_equal(y, h["y"]) and not R.bit_equal(y, y_sorted)


# ---- 4. dictionary limits -----------------------------------------------------------------------------------------------------------
def _pattern_matrix(extra):
    """rows of two entries (+1, a), (+2, b), a and b out of 16 values: 255 of the 256 combinations, in turn, and the two last rows
    empty -- 256 patterns on 32 pairs.  extra: one row stores its two entries in the other order, a 257th pattern on the same pairs"""
    n = 1021
    pal = 1.0 + np.arange(16) / 16.0
    ip = np.zeros(n + 1, dtype=np.int32)
    ix, da = [], []
    for i in range(n - 2):
        p = i % 255
        ent = [(i + 1, pal[p // 16]), (i + 2, pal[p % 16])]
        if extra and i == 300 + 5:          # combination 5: a != b
            ent.reverse()
        ix += [e[0] for e in ent]
        da += [e[1] for e in ent]
        ip[i + 1] = len(ix)
    ip[n - 1:] = len(ix)
    return ip, np.asarray(ix, dtype=np.int32), np.asarray(da)


@pytest.mark.parametrize("count", [256, 257])
def test_dictionary_limits(pkg, gpu, tuned, count):
    """exactly 256 row patterns are coded; one more and the handle keeps the joint form"""
    dtype = np.float64
    h = host(("dict", count), lambda: _pattern_matrix(count == 257), dtype)
    ip, ix, da = h["mat"]
    assert row_patterns(ip, ix, da)[0] == count and R.distinct_pairs(ip, ix, da) == 32 <= 256
    tuned()
    if count == 256:
        run_case(pkg, gpu[0], "256 patterns", h, dtype, "rowcode", patterns=256)
    else:
        run_case(pkg, gpu[0], "257 patterns", h, dtype, "joint", patterns=0)


# ---- 5. row length limit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_row", [7, 8])
def test_row_length_limit(pkg, gpu, tuned, max_row):
    """a pattern key holds 7 joint codes: rows of 7 entries are coded, a matrix with a row of 8 keeps the joint form"""
    dtype = np.float64
    offs = sorted((-64, -8, -2, -1, 0, 1, 2, 8)[:max_row])
    vals = [-1.0 - 0.125 * k for k in range(max_row)]
    h = host(("rows", max_row), lambda: stencil_matrix(509, offs, vals, dtype), dtype)
    assert h["max_row"] == max_row and row_patterns(*h["mat"])[0] <= 256
    tuned()
    run_case(pkg, gpu[0], f"rows of {max_row}", h, dtype, "rowcode" if max_row == 7 else "joint", patterns=None if max_row == 7 else 0)


# ---- 6. empty rows inside the matrix --------------------------------------------------------------------------------------------------
def test_empty_rows_inside_the_matrix(pkg, gpu, tuned):
    """rows without entries -- the first, the last, a whole wave, single ones inside uniform and mixed waves -- share the length-0
    pattern and come out +0 in the NaN-prefilled y"""
    import cg_numpy
    dtype = np.float64
    gone = [0, 1, 70, 255, 256, 257, 1000] + list(range(1408, 1472)) + [2598, 2599]
    h = host(("empty",), lambda: empty_rows(cg_numpy.laplace3d(130, 5, 4), gone), dtype)
    L = np.diff(h["mat"][0])
    assert L[0] == 0 and L[-1] == 0 and (L[1408:1472] == 0).all() and (L == 0).sum() == len(gone)
    tuned()
    y, _ = run_case(pkg, gpu[0], "empty rows", h, dtype, "rowcode", patterns=row_patterns(*h["mat"])[0])
    assert np.all(R.bits(y[0][L == 0]) == 0)


# ---- 7. non-temporal code loads and the row-block schedule ----------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [3, 9, 65])
def test_nt_and_schedule(pkg, gpu, tuned, blocks):
    """spmv_nt 0 / 1 and spmv_cycle 1 (contiguous eighths), 8 and 64 at 3, 9 and 65 row blocks (1, 3 and 17 work-groups of four row
    blocks, the last one not full): every row block exactly once, the same bits"""
    dtype = np.float64
    n = 256 * blocks - 5
    offs, vals = (-300, -20, -1, 0, 1, 20, 300), (-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0)
    h = host(("sched", blocks), lambda: stencil_matrix(n, offs, vals, dtype), dtype)
    ys = []
    for nt, cycle in [(0, 64), (1, 64), (0, 1), (1, 8)]:
        tuned(spmv_nt=nt, spmv_cycle=cycle)
        ys.append(run_case(pkg, gpu[0], f"blocks{blocks} nt{nt} cycle{cycle}", h, dtype, "rowcode", nt=nt, cycle=cycle)[0])
    assert all(R.bit_equal(y, ys[0]) for y in ys[1:])


# ---- 8. the loop ----------------------------------------------------------------------------------------------------------------------
def _iterate(pkg, ctx, mat, dtype, iters):
    ip, ix, da = mat
    n = len(ip) - 1
    s = pkg.Solver(ctx, n, len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        lib = pkg._lib.load()
        s.set_rhs(np.linspace(1.0, 2.0, n).astype(dtype))
        s.iterate(iters)
        ctx.synchronize()
        return {"row_codes": s.row_codes, "launches": lib.cgamd_solver_loop_launches(s.handle), "x_lag": lib.cgamd_solver_x_lag(s.handle),
                "history": s.history().copy(), "x": s.x().copy()}
    finally:
        s.close()


@pytest.mark.parametrize("grid,launches,lag,keys", [((100, 80, 70), 4, 4, {}), ((130, 5, 4), 3, 1, {"two_launch": 0})], ids=["560000-rows", "2600-rows"])
def test_the_loop_is_bit_identical(pkg, gpu, tuned, grid, launches, lag, keys):
    """25 iterations with row codes and with dev.row_codes = 0: the same history and x, bit for bit, in the same loop.  560 000 rows
    (more than 2 048 d.q partials): the four-launch loop with the default x lag; 2 600 rows with two_launch = 0: the three-launch
    loop of small systems, which launches the same SpMV"""
    import cg_numpy
    dtype = np.float64
    mat = in_type(cg_numpy.laplace3d(*grid), dtype)
    tuned(**keys)
    a = _iterate(pkg, gpu[0], mat, dtype, 25)
    tuned(dev_row_codes=0, **keys)
    b = _iterate(pkg, gpu[0], mat, dtype, 25)
    assert a["row_codes"] == 27 and b["row_codes"] == 0
    assert (a["launches"], a["x_lag"]) == (launches, lag) == (b["launches"], b["x_lag"])
    assert a["history"].shape == (26, 1) and np.all(np.isfinite(a["history"]))
    assert R.bit_equal(a["history"], b["history"]) and R.bit_equal(a["x"], b["x"])


# ---- 9. reload ------------------------------------------------------------------------------------------------------------------------
def test_reload_rebuilds_the_codes(pkg, gpu, tuned):
    """cgamd_solver_reload_matrix with a variable-coefficient matrix of the same pattern (more than 256 values): no value codes, so no
    row codes, and the SpMV is the host's bit for bit; the 7-point matrix again: 27 patterns again"""
    import cg_numpy
    dtype = np.float64
    ctx = gpu[0]
    lib = pkg._lib.load()
    h = host(("lap3d", "f64", (130, 5, 4)), lambda: cg_numpy.laplace3d(130, 5, 4), dtype)
    ip, ix, da = h["mat"]
    da_var = da * (1.0 + np.arange(len(da)) / (4.0 * len(da)))
    assert R.distinct_values(da_var) > 256
    hv = dict(h, mat=(ip, ix, da_var), ext=R.spmv_ext(ip, ix, da_var, h["x"], dtype), y=R.spmv_in_type(ip, ix, da_var, h["x"], dtype))
    hv["parts"] = R.block_partials_in_type(h["x"][0], hv["y"][0], dtype)
    tuned()
    s = pkg.Solver(ctx, h["n"], len(ix), da, ip, ix, 1, dtype=dtype)
    try:
        assert s.row_codes == 27
        verify("before reload", h, dtype, spmv_both(pkg, ctx, s, h, dtype), expected_form("rowcode", h["n"], 7))
        pkg._lib.check(lib.cgamd_solver_reload_matrix(s.handle, pkg._lib.ptr(da_var), pkg._lib.ptr(ip), pkg._lib.ptr(ix)))
        assert s.row_codes == 0 and s.value_codes == 0 and s.index_codes == 7
        runs = spmv_both(pkg, ctx, s, hv, dtype)
        assert all(r[2]["family"] == "rowblock" and r[2]["index_bits"] == 8 and r[2]["value_codes"] == 0 for r in runs), runs[0][2]
        for f, y, form, parts in runs:
            R.check_rows(y, ip, ix, da_var, h["x"], dtype, ext=hv["ext"], label="reloaded")
            assert R.bit_equal(y, hv["y"])
            if f:
                assert R.bit_equal(parts[0], hv["parts"])
        pkg._lib.check(lib.cgamd_solver_reload_matrix(s.handle, pkg._lib.ptr(da), pkg._lib.ptr(ip), pkg._lib.ptr(ix)))
        assert s.row_codes == 27
        verify("after the second reload", h, dtype, spmv_both(pkg, ctx, s, h, dtype), expected_form("rowcode", h["n"], 7))
    finally:
        s.close()


# ---- 10. thresholds -------------------------------------------------------------------------------------------------------------------
def test_small_matrices_keep_the_joint_form_by_default(pkg, gpu, tuned):
    """the tuning defaults with index_codes_min_mb = 0 alone (what the tests of the joint form set): a matrix below 32 MB builds no row
    codes and runs the joint vcp form"""
    import cg_numpy
    dtype = np.float64
    h = host(("lap3d", "f64", (130, 5, 4)), lambda: cg_numpy.laplace3d(130, 5, 4), dtype)
    assert len(h["mat"][1]) * 12 < 32 << 20
    tuned(base=False, resident=0, index_codes_min_mb=0)
    run_case(pkg, gpu[0], "default thresholds", h, dtype, "joint", patterns=0)
