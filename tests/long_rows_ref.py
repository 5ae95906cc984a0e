"""Host restatement of the CGAMD_SPLIT_LONG_ROWS form (csrc/long_rows.hip, setup_long_rows in csrc/solver.cpp) -- pure numpy, no GPU.

The plan, from the row pointers alone
-------------------------------------
* HEAVY: a 256-row block is heavy when any of its 8-row slices spans more than heavy_bytes / (sizeof(T) + 4) entries, the span
  measured from ip[first row] rounded down to a multiple of 4 (spmv_span_kernel's measure); heavy_bytes = 48 KB unless
  dev.long_row_bytes lowers it.
* REGULAR blocks, in the order the block-cyclic schedule deals them (rowblock_of over the work-groups of a full launch), and their
  spans, from which the body's kernel is chosen by the launcher's rules (`choose_kind`).
* SEGMENTS: every heavy block's span [ip[r0] & ~3, ip[r1]) cut into pieces of `segment` entries.

The arithmetic of a heavy block, in the value type T (helpers of spmv_ref)
--------------------------------------------------------------------------
products T(a x) as vmul forms them; a row's PIECE inside a segment: up to PIECE = 64 entries by one lane in stored order from +0,
longer by 64 lanes (lane l adds entries l, l + 64, ... from +0, then v[l] += v[l + off], off = 32 ... 1, lane 0); a row inside one
segment is its piece, a row that crosses segment edges the sum of its pieces in ascending segment order from +0; a row without
entries is +0."""
import numpy as np

import spmv_ref as R

PIECE = 64                  # kLongRowPiece
SEGMENT = 2048              # kLongRowSegment
MAX_CHUNK_BYTES = 48 * 1024  # kMaxChunkBytes
CHUNK_BYTES = 32 * 1024     # kChunkBytes
MAX_SLICE_BYTES = 40 * 1024  # kMaxSliceBytes
MAX_LDS = 128 * 1024        # kLongRowMaxLds


def rowblock_of(b, row_blocks, cycle):
    xcd, i = b & 7, b >> 3
    if cycle > 1:
        chunk = (cycle + 7) >> 3
        k = i // chunk
        lo = xcd * chunk + (i - k * chunk)
        rb = k * cycle + lo
        return rb if lo < cycle and rb < row_blocks else -1
    xb, xe = xcd * row_blocks // 8, (xcd + 1) * row_blocks // 8
    return xb + i if i < xe - xb else -1


def rowblock_grid(row_blocks, cycle):
    if cycle > 1:
        return 8 * ((cycle + 7) // 8) * ((row_blocks + cycle - 1) // cycle)
    return 8 * max((x + 1) * row_blocks // 8 - x * row_blocks // 8 for x in range(8))


def block_spans(ip, blocks):
    """spmv_span_kernel over the row blocks `blocks`: ([span of the 256 >> lv - row slices, lv = 0..5], longest row)"""
    ip = np.asarray(ip, dtype=np.int64)
    n = len(ip) - 1
    spans, max_row = [0] * 6, 0
    for rb in blocks:
        r0, r1 = rb * 256, min(rb * 256 + 256, n)
        for lv in range(6):
            rows = 256 >> lv
            for ra in range(r0, r1, rows):
                spans[lv] = max(spans[lv], int(ip[min(ra + rows, n)] - ip[ra] // 4 * 4))
        max_row = max(max_row, int(np.diff(ip[r0:r1 + 1]).max()))
    return spans, max_row


def choose_kind(spans, dtype, slice_kb=0, chunk_kb=0):
    """finalize_spmv_plan for one right-hand side (dev.spmv_slice_kb / dev.spmv_chunk_kb: 0 = the defaults): (kind, lanes per row)"""
    V = np.dtype(dtype).itemsize
    acc = 16 if R.is_complex(dtype) else 8
    if spans[0] <= 0:
        return 0, 1
    if spans[0] * (V + 4) + acc * 4 <= (slice_kb * 1024 if slice_kb > 0 else MAX_SLICE_BYTES):
        return 5, 1
    for lv in range(5):
        if spans[lv + 1] > 0 and spans[lv + 1] * (V + 4) <= (chunk_kb * 1024 if chunk_kb > 0 else CHUNK_BYTES):
            return 7, 2 << lv
    if spans[5] > 0 and spans[5] * (V + 4) <= MAX_CHUNK_BYTES:
        return 7, 32
    return 0, 1


def plan(ip, dtype, heavy_bytes=0, segment=0, cycle=64, slice_kb=0, chunk_kb=0):
    """the handle's lists; an empty plan (no heavy block) has heavy == [] and everything else empty / zero"""
    ip = np.asarray(ip, dtype=np.int64)
    n = len(ip) - 1
    V = np.dtype(dtype).itemsize
    hb = heavy_bytes if 0 < heavy_bytes < MAX_CHUNK_BYTES else MAX_CHUNK_BYTES
    thr = hb // (V + 4)
    seg = segment if segment > 0 else SEGMENT
    seg = max(min(seg, MAX_LDS // (V + 4)) & ~3, 4)
    row_blocks = (n + 255) // 256
    heavy = []
    for rb in range(row_blocks):
        r0, r1 = rb * 256, min(rb * 256 + 256, n)
        if any(ip[min(ra + 8, n)] - ip[ra] // 4 * 4 > thr for ra in range(r0, r1, 8)):
            heavy.append(rb)
    if not heavy:
        return {"heavy": [], "regular": [], "segments": [], "seg0": [0], "segment": 0, "body_kind": 0, "body_lanes": 0, "scratch_bytes": 0}
    hs = set(heavy)
    regular = [rb for rb in (rowblock_of(b, row_blocks, cycle) for b in range(rowblock_grid(row_blocks, cycle))) if rb >= 0 and rb not in hs]
    segments, seg0 = [], [0]
    for h, rb in enumerate(heavy):
        cfirst, p1 = int(ip[rb * 256]) // 4 * 4, int(ip[min(rb * 256 + 256, n)])
        segments += [(h, e0) for e0 in range(cfirst, p1, seg)]
        seg0.append(len(segments))
    spans, max_row = block_spans(ip, regular)
    kind, lanes = choose_kind(spans, dtype, slice_kb, chunk_kb) if regular else (0, 0)
    return {"heavy": heavy, "regular": regular, "segments": segments, "seg0": seg0, "segment": seg, "body_kind": kind,
            "body_lanes": lanes if kind == 7 else 1 if kind == 5 else 0, "body_spans": spans, "body_max_row": max_row,
            "scratch_bytes": len(segments) * 2 * V}


def _seq(v, R_):
    """sum from +0 in order, every addition rounded in the real type R_"""
    return np.add.accumulate(np.concatenate([np.zeros(1, R_), v]))[-1]


def _piece(v, R_):
    """one component of a piece's products -> its sum as the segment kernel forms it"""
    L = len(v)
    if L <= PIECE:
        return _seq(v, R_)
    rounds = (L + 63) // 64
    pad = np.zeros(rounds * 64, R_)
    pad[:L] = v
    pad = pad.reshape(rounds, 64)
    lanes = np.zeros(64, R_)
    for r in range(rounds):
        m = min(64, L - r * 64)
        lanes[:m] = lanes[:m] + pad[r, :m]
    off = 32
    while off > 0:
        lanes[:off] = lanes[:off] + lanes[off:2 * off]
        off //= 2
    return lanes[0]


def heavy_rows(ip, ix, da, x, dtype, pl):
    """{row: value} for every row of the heavy blocks, and {row: True} for the rows that lie in one segment and are at most PIECE long
    (those must have the bits of spmv_in_type)"""
    ip = np.asarray(ip, dtype=np.int64)
    n = len(ip) - 1
    R_ = R.real_type(dtype)
    cplx = R.is_complex(dtype)
    seg = pl["segment"]
    out, plain = {}, {}
    with np.errstate(all="ignore"):
        for rb in pl["heavy"]:
            r0, r1 = rb * 256, min(rb * 256 + 256, n)
            cfirst = int(ip[r0]) // 4 * 4
            for row in range(r0, r1):
                s, e = int(ip[row]), int(ip[row + 1])
                if e == s:
                    out[row] = np.dtype(dtype).type(0)
                    plain[row] = True
                    continue
                cols = np.asarray(ix)[s:e]
                xs = np.asarray(x, dtype=dtype)[cols]
                pr, pi = R.vmul_t(R._parts(np.asarray(da, dtype=dtype)[s:e], dtype), R._parts(xs, dtype), dtype)
                ks, ke = (s - cfirst) // seg, (e - 1 - cfirst) // seg
                pieces = []
                for k in range(ks, ke + 1):
                    lo, hi = max(s, cfirst + k * seg) - s, min(e, cfirst + (k + 1) * seg) - s
                    pieces.append((_piece(pr[lo:hi], R_), _piece(pi[lo:hi], R_) if cplx else None))
                if len(pieces) == 1:
                    re, im = pieces[0]
                    plain[row] = e - s <= PIECE
                else:
                    re = _seq(np.array([p[0] for p in pieces], R_), R_)
                    im = _seq(np.array([p[1] for p in pieces], R_), R_) if cplx else None
                    plain[row] = False
                out[row] = R._join(np.array([re], R_), np.array([im], R_) if cplx else None, dtype)[0]
    return out, plain


def spmv_split(ip, ix, da, x, dtype, pl, body=None):
    """y (n,) of the split form: the body's restatement (spmv_in_type for kind 5, spmv_chunked_in_type for kind 7; `body` when the
    caller has it already) with the rows of the heavy blocks replaced"""
    n = len(ip) - 1
    if body is None:
        if pl["body_kind"] == 7:
            body = R.spmv_chunked_in_type(ip, ix, da, x, dtype, pl["body_lanes"])[0]
        else:
            body = R.spmv_in_type(ip, ix, da, x, dtype)[0]
    y = np.array(body, dtype=dtype).reshape(n).copy()
    rows, _ = heavy_rows(ip, ix, da, x, dtype, pl)
    for row, v in rows.items():
        y[row] = v
    return y


def block_partials(d, y, dtype, pl):
    """the d.q partial of every 256-row block: the body's tree for the regular blocks, block_sum<256> for the heavy ones"""
    lane = R.block_partials_in_type(d, y, dtype)
    if pl["body_kind"] != 7:
        return lane
    out = R.block_partials_chunked_in_type(d, y, dtype, pl["body_lanes"])
    out[pl["heavy"]] = lane[pl["heavy"]]
    return out


# ---- fixtures shared by the host test and the device test -----------------------------------------------------------------------------
def hub_matrix(rng, n, hubs, dtype, short=None, steer=True):
    """ragged banded matrix (spmv_ref.ragged_lengths over `short`) whose rows `hubs` = {row: length} are hubs with distinct random
    columns; hubs override the forced empty rows"""
    short = short if short is not None else R.length_set(8)
    L = R.ragged_lengths(rng, n, short, steer=steer)
    for row, length in hubs.items():
        L[row] = length
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(L, out=ip[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), L)
    offs = rng.choice(R.offsets8(rng), size=rows.size)
    ix = ((rows + offs) % n).astype(np.int32)
    for row, length in hubs.items():
        if length <= n:
            ix[ip[row]:ip[row + 1]] = rng.permutation(n)[:length]
        else:
            ix[ip[row]:ip[row + 1]] = rng.integers(0, n, length)
    da = R.rand_values(rng, rows.size, dtype)
    return ip, ix, da


def loop_system(dtype):
    """the coupled grid system of the loop tests: 2-D 5-point Laplacian 75 x 80 plus 0.1 I, hubs 3000, 3001 and 5999 coupled to every
    other non-hub row with weight -1/64 (+1/64 on the coupled row's diagonal, the sum on the hub's); complex: times (1 + 0.05i).
    Symmetric positive definite; the longest row has 5999 entries.  -> (ip, ix, da) with sorted columns"""
    nx, ny = 75, 80
    n = nx * ny
    hubs = [3000, 3001, 5999]
    w = 1.0 / 64
    A = {}

    def add(i, j, v):
        A[(i, j)] = A.get((i, j), 0.0) + v
    for j in range(ny):
        for i in range(nx):
            r = j * nx + i
            add(r, r, 4.1)
            if i > 0:
                add(r, r - 1, -1.0)
            if i < nx - 1:
                add(r, r + 1, -1.0)
            if j > 0:
                add(r, r - nx, -1.0)
            if j < ny - 1:
                add(r, r + nx, -1.0)
    hs = set(hubs)
    for h in hubs:
        for r in range(n):
            if r in hs:
                continue
            add(h, r, -w)
            add(r, h, -w)
            add(r, r, w)
            add(h, h, w)
    keys = sorted(A)
    rows = np.array([k[0] for k in keys], dtype=np.int64)
    ix = np.array([k[1] for k in keys], dtype=np.int32)
    vals = np.array([A[k] for k in keys], dtype=np.float64)
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=ip[1:])
    if R.is_complex(dtype):
        vals = vals * (1 + 0.05j)
    return ip, ix, vals.astype(dtype)


# ---- the cases of tests/test_long_rows_ref.py and tests/test_gpu_long_rows.py ----------------------------------------------------------
HEAVY_ENTRIES = 200         # the lowered threshold of the small cases: dev.long_row_bytes = HEAVY_ENTRIES * (sizeof(T) + 4)
SMALL_SEGMENT = 256


def small_case(variant, dtype):
    """n = 700 + 37 (three row blocks, the last one partial), ragged short rows, block 0 regular, blocks 1 and 2 heavy.  Hubs: 257 at
    the first row of block 1, 256 at its last row, 512 and 513 adjacent (rows 300, 301), 512 at row 400 whose first entry falls on
    a segment start, 255 between empty rows (row 600), 2500 at the last row of the matrix -- hubs in two adjacent blocks.  The
    starts of the heavy blocks' slices are steered to ip[256] % 4, ip[512] % 4 = (1, 2) (variant 0) and (3, 0) (variant 1)."""
    n = 737
    rng = np.random.default_rng(900 + variant)
    hubs = {256: 257, 511: 256, 300: 512, 301: 513, 400: 512, 600: 255, 736: 2500}
    short = R.length_set(8)
    L = R.ragged_lengths(rng, n, short, steer=False)
    L[599], L[601] = 0, 0
    for row, length in hubs.items():
        L[row] = length
    t1, t2 = ((1, 2), (3, 0))[variant]
    L[1] += (t1 - int(L[:256].sum())) % 4
    cfirst = int(L[:256].sum()) // 4 * 4
    L[399] += (-(int(L[:400].sum()) - cfirst)) % SMALL_SEGMENT
    L[402] += (t2 - int(L[:512].sum())) % 4
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(L, out=ip[1:])
    assert ip[256] % 4 == t1 and ip[512] % 4 == t2 and (ip[400] - cfirst) % SMALL_SEGMENT == 0
    rows = np.repeat(np.arange(n, dtype=np.int64), L)
    ix = ((rows + rng.choice(R.offsets8(rng), size=rows.size)) % n).astype(np.int32)
    for row, length in hubs.items():
        ix[ip[row]:ip[row + 1]] = rng.permutation(n)[:length] if length <= n else rng.integers(0, n, length)
    return ip, ix, R.rand_values(rng, rows.size, dtype)


def small_tune(dtype):
    return {"dev.long_row_bytes": HEAVY_ENTRIES * (np.dtype(dtype).itemsize + 4), "dev.long_row_segment": SMALL_SEGMENT}


def default_case(dtype):
    """n = 10 000 with one hub of 9000 entries, default threshold and segment length"""
    rng = np.random.default_rng(77)
    return hub_matrix(rng, 10000, {5000: 9000}, dtype)


def dense_body_case(dtype):
    """rows of about 40 entries (the body lands in the chunked kernel) and one hub of 1500 entries in block 1 of three"""
    n = 700
    rng = np.random.default_rng(78)
    L = rng.integers(36, 45, n)
    L[300] = 1500
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(L, out=ip[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), L)
    ix = ((rows + rng.choice(R.offsets8(rng), size=rows.size)) % n).astype(np.int32)
    ix[ip[300]:ip[301]] = rng.integers(0, n, 1500)
    return ip, ix, R.rand_values(rng, rows.size, dtype)


def dense_body_tune(ip, dtype, lanes=4):
    """chunked_tune of test_gpu_spmv_forms.py on the spans of the REGULAR blocks, plus the heavy threshold of 1000 entries"""
    eb = np.dtype(dtype).itemsize + 4
    pl = plan(ip, dtype, heavy_bytes=1000 * eb, segment=SMALL_SEGMENT)
    lv = {2: 1, 4: 2, 8: 3, 16: 4, 32: 5}[lanes]
    kb = -(-pl["body_spans"][lv] * eb // 1024)
    assert pl["body_spans"][lv - 1] * eb > kb * 1024
    return {"dev.long_row_bytes": 1000 * eb, "dev.long_row_segment": SMALL_SEGMENT, "dev.spmv_slice_kb": 1, "dev.spmv_chunk_kb": int(kb)}
