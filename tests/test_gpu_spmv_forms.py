"""Every kernel form the launcher of csrc/spmv.hip (spmv_impl) can choose, row by row against the host (tests/spmv_ref.py).

Each case first asserts Solver.last_spmv_form() -- recorded at the launch site -- equals the form it was written for, so a plan
threshold that moves cannot turn it into a test of another kernel: a case that does not reach its form fails.  Then
  * check_rows: every row of every right-hand side within the textbook bound of the extended-precision product, rows without
    entries exactly +0 (y is prefilled with NaN);
  * bit equality with the host restatement for every form but the generic stream kernel (one lane per row: spmv_in_type; chunked:
    spmv_chunked_in_type), hence also of all forms of one matrix with each other;
  * with fused_dot: the d.q partials bit-equal to the restated block sum per 256-row block (stream kernel: the derived bound of
    spmv_ref.stream_dot_bound), on x whose magnitudes spread over 2^30 (2^48 for the 32-bit types) within every wave.
The bounds are derived in spmv_ref's docstring; nothing here is tuned to a device result."""
import ctypes
import zlib

import numpy as np
import pytest

import spmv_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
ALL = list(DT)
CODABLE = ["f32", "f64", "c64"]          # value codes: types of at most 8 bytes

# struct Tuning's defaults (csrc/cgamd_internal.h) of every key this module sets
DEFAULTS = {"index_codes": 1, "index_codes16": 1, "index_codes_min_mb": 32, "resident": 1, "spmv_nt": -1, "spmv_cycle": 64,
            "dev.generic_spmv": 0, "dev.value_codes": 1, "dev.vc_pipe": 1, "dev.joint_codes": 1, "dev.spmv_unroll": 0,
            "dev.spmv_slice_kb": 0, "dev.spmv_chunk_kb": 0, "dev.spmv_chunked": 1, "dev.spmm_wide_max": -1, "dev.spmm_group": 0}
BASE = {"resident": 0, "index_codes_min_mb": 0}      # no resident loop (such handles build no codes); codes at any size


@pytest.fixture
def tuned(pkg):
    """sets tuning keys BEFORE a handle is created (a handle keeps the configuration it was created under); every call starts from
    the defaults plus BASE; the defaults are restored afterwards"""
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


# ---- expected forms -----------------------------------------------------------------------------------------------------------------
def rowblock_grid(row_blocks, cycle):
    if cycle > 1:
        return 8 * ((cycle + 7) // 8) * ((row_blocks + cycle - 1) // cycle)
    return 8 * max((x + 1) * row_blocks // 8 - x * row_blocks // 8 for x in range(8))


def fit_unroll(max_row, dtype):
    if np.dtype(dtype).itemsize > 8:
        return 4
    return 8 if max_row <= 0 else 4 if max_row <= 4 else 5 if max_row == 5 else 7 if max_row <= 7 else 8


def expected_form(family, n, width, index_bits=0, value_codes=0, nt=0, wide=0, vec=1, cycle=64):
    rb = (n + 255) // 256
    if family == "stream":
        grid = min(rb, 2048)
        grid = grid & ~7 if grid >= 8 else max(grid, 1)
        parts = grid
    elif family in ("vc", "vcp"):
        grid, parts = rowblock_grid((rb + 3) // 4, max(1, cycle // 4)), rb
    else:
        grid, parts = rowblock_grid(rb, cycle), rb
    return {"family": family, "vec": vec, "width": width, "index_bits": index_bits, "value_codes": value_codes, "nt": nt,
            "fused": 0, "wide": wide, "grid": grid, "partials": parts}      # (verify() sets fused, and partials 0 when not)


def spmm_width(nrhs, dtype):
    rbmax = 8 if np.dtype(dtype).itemsize <= 8 else 4
    groups = (nrhs + rbmax - 1) // rbmax
    w = min((nrhs + groups - 1) // groups, rbmax)
    if rbmax == 8:
        return 8 if w > 6 else w if w >= 2 else 2
    return 4 if w > 3 else 3 if w == 3 else 2


# ---- host side of a case, computed once per (matrix, x) and shared -------------------------------------------------------------------
_HOST = {}


def host(key, build, dtype, nrhs=1):
    """build() -> (ip, ix, da); adds x (adversarial magnitudes), the extended product and the restatements"""
    if key not in _HOST:
        ip, ix, da = build()
        n = len(ip) - 1
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        x = np.stack([R.adversarial_d(rng, n, dtype) for _ in range(nrhs)])
        _HOST[key] = {"mat": (ip, ix, da), "x": x, "n": n, "ext": R.spmv_ext(ip, ix, da, x, dtype, nrhs), "lane": None, "chunked": {}}
    h = _HOST[key]
    return h


def host_lane(h, dtype, nrhs):
    if h["lane"] is None:
        h["lane"] = R.spmv_in_type(*h["mat"], h["x"], dtype, nrhs)
    return h["lane"]


def host_chunked(h, dtype, lpr):
    if lpr not in h["chunked"]:
        h["chunked"][lpr] = R.spmv_chunked_in_type(*h["mat"], h["x"][0], dtype, lpr)
    return h["chunked"][lpr]


# ---- device side ---------------------------------------------------------------------------------------------------------------------
def launch(pkg, ctx, h, dtype, nrhs=1, fused=(False, True), misalign=False):
    """one handle on the case's matrix; SpMV on caller arrays, y prefilled with NaN -> [(fused, y, form, partials)]"""
    import torch
    dev = torch.device("cuda", 0)
    ip, ix, da = h["mat"]
    n = h["n"]
    keep = None
    if misalign:      # a borrowed matrix whose values and columns start 8 bytes off a 16-byte boundary: no 16-byte loads (VEC = false)
        def off8(a):
            raw = np.concatenate([np.zeros(8, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])
            t = torch.from_numpy(raw).to(dev)
            assert t.data_ptr() % 16 == 0
            return t, t.data_ptr() + 8
        tv, pv = off8(da.astype(dtype))
        tc, pc = off8(ix.astype(np.int32))
        tp = torch.from_numpy(ip.astype(np.int32)).to(dev)
        keep = (tv, tc, tp)
        torch.cuda.synchronize()
        s = pkg.Solver(ctx, n, len(ix), pv, tp, pc, nrhs, flags=pkg._lib.MATRIX_ON_DEVICE, dtype=dtype)
        s._keep = keep
    else:
        s = pkg.Solver(ctx, n, len(ix), da.astype(dtype), ip, ix, nrhs, dtype=dtype)
    xd = torch.from_numpy(np.ascontiguousarray(h["x"].reshape(-1))).to(dev)
    out = []
    try:
        for f in fused:
            nan = np.full(nrhs * n, np.nan, dtype=dtype)
            if np.dtype(dtype).kind == "c":
                nan = nan + 1j * nan
            yd = torch.from_numpy(nan.astype(dtype)).to(dev)
            torch.cuda.synchronize()
            s.spmv(xd, yd, fused_dot=f)
            form = s.last_spmv_form()
            ctx.synchronize()
            parts = s.dot_partials() if f else None
            out.append((f, yd.cpu().numpy().reshape(nrhs, n), form, parts))
    except pkg.CgAmdError as e:
        if e.status == pkg._lib.ERR_HIP:       # a kernel faulted: nothing more is started on that device in this session
            pytest.exit(f"HIP error in an SpMV launch, the session ends here: {e}", returncode=3)
        raise
    s.close()
    return out


RATIOS = {}      # label -> largest error / bound seen (printed per case; DESIGN.md section 2 quotes them)


def verify(label, h, dtype, nrhs, run, want_form, mode):
    """mode "lane": bit-equal to spmv_in_type; "chunked": to spmv_chunked_in_type; "stream": the bound only"""
    f, y, form, parts = run
    want = dict(want_form, fused=int(f), partials=want_form["partials"] if f else 0)
    print(f"{label} fused={int(f)}: ran {form}")
    assert form == want, f"{label}: launched {form}, the case is written for {want}"
    ip, ix, da = h["mat"]
    worst = R.check_rows(y, ip, ix, da, h["x"], dtype, nrhs, ext=h["ext"], label=label)
    RATIOS[label] = max(RATIOS.get(label, 0.0), worst)
    if mode == "lane":
        ref = host_lane(h, dtype, nrhs)
        diff = np.argwhere(R.bits(y) != R.bits(ref))
        assert diff.size == 0, f"{label}: {len(diff)} values differ from the host restatement, first at {diff[0].tolist()}"
    elif mode == "chunked":
        ref = host_chunked(h, dtype, form["width"])
        diff = np.argwhere(R.bits(y) != R.bits(ref))
        assert diff.size == 0, f"{label}: {len(diff)} values differ from the chunked restatement, first at {diff[0].tolist()}"
    if not f:
        return y
    assert parts.shape == (nrhs, want["partials"])
    if mode == "stream":
        for r in range(nrhs):
            re, im, _ = R.dot_ext(h["x"][r], y[r], dtype)
            got = parts[r].astype(np.clongdouble if im is not None else R.LD).sum()
            err = abs(got - (re + 1j * im if im is not None else re))
            bound = R.stream_dot_bound(h["x"][r], y[r], dtype, ip=ip, s_rows=h["ext"][2][r], chunk=2048)
            print(f"{label} rhs {r}: |sum of partials - x.y| / bound = {float(err / bound):.3g}")
            assert err <= bound
        return y
    for r in range(nrhs):
        if mode == "chunked":
            ref = R.block_partials_chunked_in_type(h["x"][r], y[r], dtype, form["width"])
        else:
            ref = R.block_partials_in_type(h["x"][r], y[r], dtype)
        bad = np.nonzero(np.any((R.bits(parts[r]) != R.bits(ref)).reshape(len(ref), -1), axis=1))[0]
        assert bad.size == 0, f"{label}: d.q partials of blocks {bad.tolist()[:8]} of right-hand side {r} differ from the restated block sum"
    return y


def run_case(pkg, ctx, label, h, dtype, want_form, mode, nrhs=1, fused=(False, True), misalign=False):
    ys = [verify(label, h, dtype, nrhs, run, want_form, mode) for run in launch(pkg, ctx, h, dtype, nrhs, fused, misalign)]
    for y in ys[1:]:
        assert R.bit_equal(y, ys[0]), f"{label}: the fused and the plain instance differ"
    return ys[0]


# ---- matrices ------------------------------------------------------------------------------------------------------------------------
def ragged(seed, n, U, dtype, enc, nnz_mod=None):
    def build():
        rng = np.random.default_rng(seed)
        L = R.ragged_lengths(rng, n, R.length_set(U), nnz_mod)
        offs = R.offsets16(rng) if enc == 16 else R.offsets8(rng)
        return R.banded_matrix(rng, L, offs, dtype)
    return build


STENCILS = {4: (-1, 0, 1), 5: (-37, -1, 0, 1, 37), 7: (-300, -20, -1, 0, 1, 20, 300)}


def enc_tune(enc):
    return {"index_codes": 0} if enc == 0 else {}


# ---- the row-block kernel, three encodings -------------------------------------------------------------------------------------------
SIZES = [(1, None), (255, None), (256, None), (257, None), (1287, 1), (1287, 2), (1287, 3)]


RAGGED_CASES = [(dt, enc, n, m) for dt in ALL for enc in (0, 8, 16) for n, m in SIZES if not (enc == 16 and n == 1)]      # (1 x 1: one offset only)


@pytest.mark.parametrize("dt,enc,n,nnz_mod", RAGGED_CASES, ids=[f"{dt}-enc{e}-n{n}" + (f"-tail{m}" if m else "") for dt, e, n, m in RAGGED_CASES])
def test_rowblock_ragged(pkg, gpu, tuned, dt, enc, n, nnz_mod):
    """ragged banded matrix (row lengths 0, 1, U-1, U, U+1, 2U, 2U+1; empty first / last row of a block, an empty block, empty
    final rows), slice starts p0 % 4 = 0..3, nnz % 4 = 1, 2, 3 (the FULL = false tail of stage_slice), on aCols, 8-bit and 16-bit codes"""
    dtype = DT[dt]
    U = fit_unroll(99, dtype)
    h = host(("ragged", dt, enc, n, nnz_mod), ragged(100 + n + (nnz_mod or 0), n, U, dtype, enc, nnz_mod), dtype)
    ip, ix, _ = h["mat"]
    if n == 1287:
        assert R.slice_starts_mod4(ip) == [0, 1, 2, 3] and ip[-1] % 4 == nnz_mod
    k = R.distinct_offsets(ip, ix)
    assert (k > 256) if enc == 16 else (k <= 256)
    tuned(dev_value_codes=0, **enc_tune(enc))
    run_case(pkg, gpu[0], f"rowblock {dt} enc{enc} n{n}", h, dtype, expected_form("rowblock", n, U, index_bits=enc), "lane")


@pytest.mark.parametrize("U", [4, 5, 7, 8])
@pytest.mark.parametrize("dt", ALL)
def test_rowblock_batch_length_from_the_matrix(pkg, gpu, tuned, dt, U):
    """tridiagonal chain (longest row 3: batch 4), 5-point and 7-point grids, ragged (8); complex128 always walks in batches of 4"""
    dtype = DT[dt]
    n = 1287
    if U == 8:
        h = host(("ragged", dt, 8, n, 1), ragged(100 + n + 1, n, fit_unroll(99, dtype), dtype, 8, 1), dtype)
    else:
        h = host(("stencil", dt, U), lambda: R.toeplitz_matrix(np.random.default_rng(U), n, STENCILS[U], dtype), dtype)
    assert R.plan_spans(h["mat"][0])[1] == {4: 3, 5: 5, 7: 7, 8: 2 * fit_unroll(99, dtype) + 1}[U]
    tuned(dev_value_codes=0)
    run_case(pkg, gpu[0], f"rowblock {dt} batch{U}", h, dtype, expected_form("rowblock", n, fit_unroll(U if U < 8 else 99, dtype), index_bits=8), "lane")


@pytest.mark.parametrize("U", [4, 5, 7, 8])
@pytest.mark.parametrize("dt", ALL)
def test_rowblock_batch_length_forced(pkg, gpu, tuned, dt, U):
    """dev.spmv_unroll on the ragged matrix built around that batch length"""
    dtype = DT[dt]
    n = 1287
    h = host(("ragged-U", dt, U), ragged(200 + U, n, U, dtype, 8, 2), dtype)
    spans, _ = R.plan_spans(h["mat"][0])
    slice_kb = 64 if spans[0] * (np.dtype(dtype).itemsize + 4) + 64 > 40 * 1024 else 0      # complex128, batches of 8: past the default slice limit
    tuned(dev_value_codes=0, index_codes=0, dev_spmv_unroll=U, dev_spmv_slice_kb=slice_kb)
    run_case(pkg, gpu[0], f"rowblock {dt} unroll{U}", h, dtype, expected_form("rowblock", n, U), "lane")


def _span_matrix(dtype, span):
    """more than 256 offsets, every block inside 65 536 columns; the columns of block 1 span exactly `span`"""
    def build():
        rng = np.random.default_rng(9)
        n = 65536 + 512 + 7
        L = R.ragged_lengths(rng, n, R.length_set(4), 3)
        L[300], L[301] = 1, 1
        pos = R.offsets16(rng, 300, 2000)
        ip, ix, da = R.banded_matrix(rng, L, np.concatenate([pos, -pos]), dtype, wrap=False)
        blk = slice(ip[256], ip[512])
        lo = int(ix[blk].min())
        ix[ip[300]] = lo
        ix[ip[301]] = lo + span
        assert int(ix[blk].max()) - int(ix[blk].min()) == span
        return ip, ix, da
    return build


@pytest.mark.parametrize("span,enc", [(65535, 16), (65536, 0)])
@pytest.mark.parametrize("dt", ALL)
def test_rowblock_16bit_span_limit(pkg, gpu, tuned, dt, span, enc):
    """one block's columns span exactly 65 535: the largest 16-bit code; one more and the handle keeps aCols"""
    dtype = DT[dt]
    h = host(("span", dt, span), _span_matrix(dtype, span), dtype)
    assert R.distinct_offsets(*h["mat"][:2]) > 256
    tuned(dev_value_codes=0)
    run_case(pkg, gpu[0], f"rowblock {dt} span{span}", h, dtype, expected_form("rowblock", h["n"], fit_unroll(9, dtype), index_bits=enc), "lane",
             fused=(True,))


@pytest.mark.parametrize("dt", ["f64", "c128"])
def test_rowblock_scattered_columns(pkg, gpu, tuned, dt):
    """about 70 000 rows with columns anywhere: no code form applies although codes are on"""
    dtype = DT[dt]

    def build():
        rng = np.random.default_rng(70)
        n = 70_001
        L = R.ragged_lengths(rng, n, R.length_set(4), 1)
        ip = np.zeros(n + 1, np.int32)
        np.cumsum(L, out=ip[1:])
        return ip, rng.integers(0, n, int(ip[-1])).astype(np.int32), R.rand_values(rng, int(ip[-1]), dtype)
    h = host(("scattered", dt), build, dtype)
    tuned(dev_value_codes=0)
    run_case(pkg, gpu[0], f"rowblock {dt} scattered", h, dtype, expected_form("rowblock", h["n"], fit_unroll(9, dtype)), "lane", fused=(True,))


@pytest.mark.parametrize("enc", [0, 8])
@pytest.mark.parametrize("dt", ALL)
def test_rowblock_long_slices(pkg, gpu, tuned, dt, enc):
    """256-row slices of more than 2048 entries -- a second staging round -- that still fit the one-lane kernel: rows of 9-13 (f64,
    c64), 9-20 (f32).  complex128: such a slice is past the 40 KB limit (2048 x 20 bytes + the partials' 64 bytes), the plan gives
    the chunked kernel with 2 lanes per row -- complex128 never stages a second round in the one-lane kernel."""
    dtype = DT[dt]
    n = 2 * 256 + 3
    hi = 20 if dt == "f32" else 13

    def build():
        rng = np.random.default_rng(13)
        return R.banded_matrix(rng, rng.integers(9, hi + 1, n), R.offsets8(rng), dtype)
    h = host(("long", dt), build, dtype)
    spans, max_row = R.plan_spans(h["mat"][0])
    assert spans[0] > 2048 and max_row == hi
    tuned(dev_value_codes=0, **enc_tune(enc))
    if dt == "c128":
        assert spans[0] * 20 + 64 > 40 * 1024 and spans[1] * 20 <= 32 * 1024
        run_case(pkg, gpu[0], f"long slice {dt} enc{enc}", h, dtype, expected_form("chunked", n, 2, index_bits=enc), "chunked")
    else:
        assert spans[0] * (np.dtype(dtype).itemsize + 4) + 64 <= 40 * 1024
        run_case(pkg, gpu[0], f"long slice {dt} enc{enc}", h, dtype, expected_form("rowblock", n, 8, index_bits=enc), "lane")


# ---- value-coded forms ---------------------------------------------------------------------------------------------------------------
VC_FORMS = {"cols": ({"index_codes": 0}, ("rowblock", 0, 0)), "codes8": ({"dev_value_codes": 0}, ("rowblock", 8, 0)),
            "vc": ({"dev_vc_pipe": 0}, ("vc", 8, 1)), "vcp": ({"dev_joint_codes": 0}, ("vcp", 8, 1)), "joint": ({}, ("vcp", 8, 2))}


@pytest.mark.parametrize("n", [253, 509, 765, 1021, 2301])
@pytest.mark.parametrize("dt", CODABLE)
def test_value_coded_forms_and_pipeline_tails(pkg, gpu, tuned, dt, n):
    """a 7-point pattern with values from a palette of 5 on aCols, 8-bit codes, vc, vcp and joint codes: ceil(n / 256) % 4 = 1, 2,
    3, 0, 1 row blocks in the last four-block group of the vc / vcp pipelines; all five forms return the same bits"""
    dtype = DT[dt]
    h = host(("palette7", dt, n), lambda: R.toeplitz_matrix(np.random.default_rng(n), n, (-64, -8, -1, 0, 1, 8, 64), dtype,
                                                           R.palette_values(np.random.default_rng(5), 5, dtype)), dtype)
    ys = {}
    for name, (keys, (family, bits, vcodes)) in VC_FORMS.items():
        tuned(**keys)
        ys[name] = run_case(pkg, gpu[0], f"{name} {dt} n{n}", h, dtype, expected_form(family, n, 7, index_bits=bits, value_codes=vcodes), "lane")
    assert all(R.bit_equal(y, ys["cols"]) for y in ys.values())


@pytest.mark.parametrize("U", [4, 5])
@pytest.mark.parametrize("dt", CODABLE)
def test_value_coded_short_batches(pkg, gpu, tuned, dt, U):
    """the batch lengths 4 and 5 of the value-coded kernels: a tridiagonal chain and a 5-point grid with palette values"""
    dtype = DT[dt]
    n = 765
    h = host(("palette-stencil", dt, U), lambda: R.toeplitz_matrix(np.random.default_rng(U), n, STENCILS[U], dtype,
                                                                   R.palette_values(np.random.default_rng(5), 5, dtype)), dtype)
    ys = []
    for name in ("vc", "vcp", "joint"):
        keys, (family, bits, vcodes) = VC_FORMS[name]
        tuned(**keys)
        ys.append(run_case(pkg, gpu[0], f"{name} {dt} batch{U}", h, dtype, expected_form(family, n, U, index_bits=bits, value_codes=vcodes), "lane"))
    assert R.bit_equal(ys[0], ys[1]) and R.bit_equal(ys[0], ys[2])


def _rows_up_to(max_row, n, dtype):
    """a stencil pattern whose longest row has max_row entries; for 9 only every 50th row is that long (the +-2 entries are dropped
    elsewhere), so that the 256-row slice stays inside the 8 x 256 entries the code staging holds"""
    offs = sorted((-64, -8, -2, -1, 0, 1, 2, 8, 64)[:max_row])
    ip, ix, da = R.toeplitz_matrix(np.random.default_rng(max_row), n, offs, dtype, R.palette_values(np.random.default_rng(6), 5, dtype))
    if max_row < 9:
        return ip, ix, da
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    keep = (np.abs(ix - rows) != 2) | (rows % 50 == 25)
    ip2 = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=ip2[1:])
    return ip2, ix[keep], da[keep]


@pytest.mark.parametrize("max_row,family,width", [(6, "vcp", 7), (7, "vcp", 7), (8, "vcp", 8), (9, "vc", 8)])
@pytest.mark.parametrize("dt", CODABLE)
def test_value_coded_pipeline_needs_rows_inside_one_batch(pkg, gpu, tuned, dt, max_row, family, width):
    """longest row shorter than, equal to (7 and 8) and one longer than the batch: the last leaves vcp for vc"""
    dtype = DT[dt]
    n = 509
    h = host(("palette-rows", dt, max_row), lambda: _rows_up_to(max_row, n, dtype), dtype)
    spans, longest = R.plan_spans(h["mat"][0])
    assert longest == max_row and spans[0] <= 2048
    tuned()
    run_case(pkg, gpu[0], f"{family} {dt} rows{max_row}", h, dtype,
             expected_form(family, n, width, index_bits=8, value_codes=2 if family == "vcp" else 1), "lane")


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("dt", CODABLE)
def test_value_coded_slice_limit(pkg, gpu, tuned, dt, extra):
    """all rows of 8 entries: the slice is exactly 8 x 256, the most the code staging holds; one row of 9 and the handle must fall
    back to the row-block kernel on 8-bit codes"""
    dtype = DT[dt]
    n = 509

    def build():
        rng = np.random.default_rng(8)
        L = np.full(n, 8)
        L[100] += extra
        offs = np.array([-9, -5, -2, -1, 1, 2, 5, 9])
        return R.banded_matrix(rng, L, offs, dtype, palette=R.palette_values(rng, 5, dtype), wrap=False)
    h = host(("slice8", dt, extra), build, dtype)
    assert R.plan_spans(h["mat"][0])[0][0] == 2048 + extra
    tuned()
    want = expected_form("rowblock", n, 8, index_bits=8) if extra else expected_form("vcp", n, 8, index_bits=8, value_codes=2)
    run_case(pkg, gpu[0], f"slice limit {dt} +{extra}", h, dtype, want, "lane")


@pytest.mark.parametrize("what,count,landing", [("values", 256, ("vcp", 1)), ("values", 257, ("rowblock", 0)),
                                                ("pairs", 256, ("vcp", 2)), ("pairs", 257, ("vcp", 1))])
@pytest.mark.parametrize("dt", CODABLE)
def test_value_coded_dictionary_limits(pkg, gpu, tuned, dt, what, count, landing):
    """256 distinct values: value codes (more than 256 pairs: two code streams); 257: none.  256 distinct (offset, value) pairs:
    joint codes; 257: two code streams"""
    dtype = DT[dt]
    n = 1021
    if what == "values":
        build = lambda: R.toeplitz_matrix(np.random.default_rng(count), n, (-64, -8, -1, 0, 1, 8, 64), dtype,
                                          R.palette_values(np.random.default_rng(7), count, dtype))
        width = 7
    else:
        offs = np.array([o for o in range(-8, 9) if o])
        build = lambda: R.pair_matrix(np.random.default_rng(count), n, 8, offs, R.palette_values(np.random.default_rng(7), 16, dtype), dtype,
                                      extra_pair=count == 257)
        width = 8
    h = host(("dict", dt, what, count), build, dtype)
    ip, ix, da = h["mat"]
    assert (R.distinct_values(da) if what == "values" else R.distinct_pairs(ip, ix, da)) == count
    if what == "values":
        assert R.distinct_pairs(ip, ix, da) > 256
    tuned()
    family, vcodes = landing
    run_case(pkg, gpu[0], f"{count} {what} {dt}", h, dtype, expected_form(family, n, width, index_bits=8, value_codes=vcodes), "lane")


# ---- the chunked kernel --------------------------------------------------------------------------------------------------------------
def chunked_case(dtype, lpr, enc, blocks=1):
    """n one more than a whole number of chunks (a block ends in a one-row chunk, then breaks); row lengths 0, 1, LPR-1, LPR,
    LPR+1, U LPR, U LPR+1.  Returns (build, n)"""
    U = 4 if np.dtype(dtype).itemsize > 8 else 8
    n = 256 * blocks + 256 // lpr + 1

    def build():
        rng = np.random.default_rng(1000 + lpr)
        L = R.ragged_lengths(rng, n, R.length_set(U, lpr), steer=False)
        return R.banded_matrix(rng, L, R.offsets16(rng) if enc == 16 else R.offsets8(rng), dtype)
    return build, n


def chunked_tune(ip, dtype, lpr):
    """the keys that make the plan take `lpr` lanes per row: no one-lane slice, and a preferred chunk size between the span of
    256 / lpr rows and that of twice as many (finalize_spmv_plan takes the smallest lpr that fits)"""
    spans, _ = R.plan_spans(ip)
    eb = np.dtype(dtype).itemsize + 4
    lv = {2: 1, 4: 2, 8: 3, 16: 4, 32: 5}[lpr]
    kb = -(-spans[lv] * eb // 1024)
    assert spans[0] * eb > 1024
    assert lv == 1 or spans[lv - 1] * eb > kb * 1024, (spans, kb)
    return {"dev_spmv_slice_kb": 1, "dev_spmv_chunk_kb": int(kb)}


@pytest.mark.parametrize("enc", [0, 8, 16])
@pytest.mark.parametrize("lpr", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("dt", ALL)
def test_chunked(pkg, gpu, tuned, dt, lpr, enc):
    dtype = DT[dt]
    build, n = chunked_case(dtype, lpr, enc)
    h = host(("chunked", dt, lpr, enc), build, dtype)
    ip, ix, _ = h["mat"]
    k = R.distinct_offsets(ip, ix)
    assert (k > 256) if enc == 16 else (k <= 256)
    L = np.diff(ip)
    assert L.max() == (4 if dt == "c128" else 8) * lpr + 1 and (L[L > 0] < lpr).any()       # rows shorter than the lanes of a row
    tuned(**chunked_tune(ip, dtype, lpr), **enc_tune(enc))
    run_case(pkg, gpu[0], f"chunked {dt} lpr{lpr} enc{enc}", h, dtype, expected_form("chunked", n, lpr, index_bits=enc), "chunked")


@pytest.mark.parametrize("dt", ALL)
def test_chunked_by_row_density(pkg, gpu, tuned, dt):
    """default thresholds: rows of 40-60 entries no longer fit a 256-row slice; the plan's own choice of lanes per row"""
    dtype = DT[dt]
    n = 256 + 7

    def build():
        rng = np.random.default_rng(44)
        return R.banded_matrix(rng, rng.integers(40, 61, n), R.offsets8(rng), dtype)
    h = host(("dense", dt), build, dtype)
    spans, _ = R.plan_spans(h["mat"][0])
    eb = np.dtype(dtype).itemsize + 4
    assert spans[0] * eb > 40 * 1024
    lpr = next(2 << lv for lv in range(5) if spans[lv + 1] * eb <= 32 * 1024)
    tuned()
    run_case(pkg, gpu[0], f"chunked {dt} by density", h, dtype, expected_form("chunked", n, lpr, index_bits=8), "chunked")


# ---- multi-RHS -----------------------------------------------------------------------------------------------------------------------
def _mrhs(dt, nrhs):
    dtype = DT[dt]
    n = 1287                # odd: every right-hand side after the first starts off a 16-byte boundary
    return host(("mrhs", dt, nrhs), ragged(300, n, fit_unroll(99, dtype), dtype, 8, 3), dtype, nrhs), n


@pytest.mark.parametrize("dt,nrhs", [(dt, k) for dt in ALL for k in ((2, 3, 4, 5, 9) if dt == "c128" else (2, 3, 4, 5, 6, 7, 8, 9, 12, 17))])
def test_spmm_grouped(pkg, gpu, tuned, dt, nrhs):
    """register groups of 2, 3, 4, 5, 6 and 8 right-hand sides; 7, 9 and 17 (complex128: 3, 5, 9) end in a group whose spare slots
    alias its first right-hand side; fused partials for every right-hand side"""
    h, n = _mrhs(dt, nrhs)
    want = {2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 8, 8: 8, 9: 5, 12: 6, 17: 6}[nrhs] if dt != "c128" else {2: 2, 3: 3, 4: 4, 5: 3, 9: 3}[nrhs]
    assert spmm_width(nrhs, DT[dt]) == want
    tuned(dev_spmm_wide_max=0)
    run_case(pkg, gpu[0], f"spmm {dt} x{nrhs}", h, DT[dt], expected_form("spmm", n, want), "lane", nrhs=nrhs)


@pytest.mark.parametrize("nrhs", [2, 9])
@pytest.mark.parametrize("dt", ALL)
def test_spmm_wide(pkg, gpu, tuned, dt, nrhs):
    """one work-group per (row block, right-hand side) runs the single-RHS row-block kernel"""
    h, n = _mrhs(dt, nrhs)
    tuned()
    run_case(pkg, gpu[0], f"wide {dt} x{nrhs}", h, DT[dt], expected_form("rowblock", n, fit_unroll(99, DT[dt]), wide=1), "lane", nrhs=nrhs)


# ---- the generic stream kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True], ids=["vec", "novec"])
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("dt", ALL)
def test_stream(pkg, gpu, tuned, dt, nrhs, misalign):
    """dev.generic_spmv = 1 (16-byte loads) and a borrowed matrix at 8-byte-aligned pointers (VEC = false); one row of 2500 entries
    -- more than one chunk of 2048 -- between empty rows.  Per-chunk sums: the bound, no bit identity."""
    dtype = DT[dt]
    n = 700

    def build():
        rng = np.random.default_rng(17)
        L = R.ragged_lengths(rng, n, R.length_set(8), 2)
        L[299:302] = (0, 2500, 0)
        return R.banded_matrix(rng, L, R.offsets16(rng, 600, 340), dtype)
    h = host(("stream", dt, nrhs), build, dtype, nrhs)
    tuned(dev_generic_spmv=0 if misalign else 1)
    run_case(pkg, gpu[0], f"stream {dt} x{nrhs} {'novec' if misalign else 'vec'}", h, dtype,
             expected_form("stream", n, 0, vec=0 if misalign else 1), "stream", nrhs=nrhs, misalign=misalign)


def test_stateless_spmv_records_its_form(pkg, gpu):
    """cgamd_spmv (no handle, no plan): the generic kernel, not fused"""
    import torch
    ctx = gpu[0]
    h = host(("ragged", "f64", 0, 257, None), ragged(100 + 257, 257, 8, np.float64, 0), np.float64)
    ip, ix, da = h["mat"]
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (da, ip, ix, h["x"][0], np.full(257, np.nan))]
    torch.cuda.synchronize()
    lib = pkg._lib.load()
    pkg._lib.check(lib.cgamd_spmv(ctx.handle, pkg._lib.F64, 257, len(ix), *[pkg._lib.ptr(a) for a in t], 1))
    form = (ctypes.c_int * 10)()
    assert lib.cgamd_last_spmv_form(form, 10) == 10
    ctx.synchronize()
    assert list(form) == [0, 1, 0, 0, 0, 0, 0, 0, 2, 0]
    R.check_rows(t[4].cpu().numpy(), ip, ix, da, h["x"], np.float64, ext=h["ext"], label="cgamd_spmv")


# ---- across the families: non-temporal loads and the row-block schedule -------------------------------------------------------------
def _family_case(family, dt, blocks):
    """(host case, tuning keys, expected form without nt / cycle, mode) of one representative per family at `blocks` row blocks"""
    dtype = DT[dt]
    n = 256 * blocks - 5
    if family in ("cols", "codes8", "codes16"):
        enc = {"cols": 0, "codes8": 8, "codes16": 16}[family]
        h = host(("fam-ragged", dt, enc, blocks), ragged(500 + blocks, n, 8, dtype, enc, 1), dtype)
        return h, dict(dev_value_codes=0, **enc_tune(enc)), dict(family="rowblock", n=n, width=8, index_bits=enc), "lane", 1
    if family in ("vc", "vcp", "joint"):
        h = host(("fam-palette", dt, blocks), lambda: R.toeplitz_matrix(np.random.default_rng(blocks), n, (-64, -8, -1, 0, 1, 8, 64), dtype,
                                                                        R.palette_values(np.random.default_rng(5), 5, dtype)), dtype)
        keys, (fam, bits, vcodes) = VC_FORMS[family]
        return h, dict(keys), dict(family=fam, n=n, width=7, index_bits=bits, value_codes=vcodes), "lane", 1
    if family == "chunked":
        build, n = chunked_case(dtype, 4, 8, blocks - 1)
        h = host(("fam-chunked", dt, blocks), build, dtype)
        return h, chunked_tune(h["mat"][0], dtype, 4), dict(family="chunked", n=n, width=4, index_bits=8), "chunked", 1
    h = host(("fam-mrhs", dt, blocks), ragged(600 + blocks, n, 8, dtype, 8, 3), dtype, 3)
    if family == "spmm":
        return h, dict(dev_spmm_wide_max=0), dict(family="spmm", n=n, width=3), "lane", 3
    return h, {}, dict(family="rowblock", n=n, width=8, wide=1), "lane", 3


FAMILIES = ["cols", "codes8", "codes16", "vc", "vcp", "joint", "chunked", "spmm", "wide"]


@pytest.mark.parametrize("family", FAMILIES)
def test_non_temporal_loads_on_and_off(pkg, gpu, tuned, family):
    """NT = true otherwise runs only for matrices above 256 MB: spmv_nt 0 and 1 in every family, same bits"""
    h, keys, want, mode, nrhs = _family_case(family, "f64", 3)
    ys = []
    for nt in (0, 1):
        tuned(spmv_nt=nt, **keys)
        ys.append(run_case(pkg, gpu[0], f"{family} nt{nt}", h, np.float64, expected_form(nt=nt, **want), mode, nrhs=nrhs, fused=(True,)))
    assert R.bit_equal(ys[0], ys[1])


@pytest.mark.parametrize("blocks", [3, 9, 65])
@pytest.mark.parametrize("cycle", [1, 8, 12, 64])
@pytest.mark.parametrize("family", ["codes8", "joint", "chunked", "spmm"])
def test_row_block_schedule(pkg, gpu, tuned, family, cycle, blocks):
    """spmv_cycle 1 (contiguous eighths: XCDs without a block at 3 blocks), 8, 12 (not a multiple of 8: padding work-groups inside
    every cycle) and 64, at 3, 9 and 65 row blocks: every row block exactly once, whatever the grid"""
    h, keys, want, mode, nrhs = _family_case(family, "f64", blocks)
    tuned(spmv_cycle=cycle, **keys)
    run_case(pkg, gpu[0], f"{family} cycle{cycle} blocks{blocks}", h, np.float64, expected_form(cycle=cycle, **want), mode, nrhs=nrhs, fused=(True,))


def test_zz_report_ratios():
    """the largest error / bound ratio of every case that ran in this session (the table of DESIGN.md section 2)"""
    groups = {}
    for label, r in RATIOS.items():
        key = label.split()[0]
        groups[key] = max(groups.get(key, 0.0), r)
    for key, r in sorted(groups.items()):
        print(f"largest error/bound, {key}: {r:.3g}")
    assert all(r <= 1 for r in RATIOS.values())
