"""Host restatement of the SpMV kernels of csrc/spmv.hip and of their fused d.q partials -- pure numpy, no GPU.

What is restated, and why it can be exact
-----------------------------------------
The library is compiled with -ffp-contract=off and `vfma(a, b, c)` is `vadd(c, vmul(a, b))` (csrc/device_types.h): one rounding
per multiply and one per add, in the value type T.  Complex products are formed by components,

    vmul(a, x).re = T(T(ar * xr) - T(ai * xi))        vmul(a, x).im = T(T(ar * xi) + T(ai * xr))

and vadd adds the components.  Every one-lane-per-row form (row-block kernel on aCols / 8-bit / 16-bit codes, vc, vcp, joint,
wide, grouped SpMM) walks a row in STORED order starting from +0:  sum = T(sum + T(a * x)).  `spmv_in_type` does exactly that,
`spmv_chunked_in_type` does it for the chunked kernel (lane l of a row takes entries s+l, s+l+LPR, ...; the LPR lane sums meet
in the xor butterfly v += v[lane ^ off], off = LPR/2 ... 1, of which lane 0's value is stored).  numpy's float32 / float64 scalar
operations are IEEE operations with one rounding, so the results can be compared with the device's BIT FOR BIT.

The d.q partial of a 256-row block (block_sum<256> of to_acc(vmul(d_i, y_i)), product rounded in T, then widened to double) is
the documented tree of wave_sum -- v[l] += v[l + off], off = 32, 16, 8, 4, 2, 1, lane 0 -- per wave of 64 rows, then
((w0 + w1) + w2) + w3: `block_partials_in_type`.  d.y is unconjugated.  The chunked kernel parks the products elsewhere in the
block before the same tree (thread j * LPR holds the rows c * 256/LPR + j, c = 0 .. LPR-1, added in that order):
`block_partials_chunked_in_type`.

The bound (`row_bound`), for ANY order of summation
---------------------------------------------------
u = 2^-24 (float32, complex64) or 2^-53 (float64, complex128), gamma_k = k u / (1 - k u), s_i = sum_j |a_ij| |x_j|.
* Real row of L entries: each product is rounded once and then passes through at most L - 1 additions whatever the order
  (a binary tree with L leaves has depth <= L - 1; the addition to the initial +0 is exact), so every term carries at most L
  factors (1 + delta), |delta| <= u, and   |y_i - yhat_i| <= gamma_L * s_i          (Higham, Accuracy and Stability, section 3.1).
* Complex row: the real part is sum_j (ar xr - ai xi), a real inner product of 2 L terms.  As the helpers are written, each of
  its 2 L products is rounded once (vmul's multiply), once more by vmul's subtraction, and then passes through at most L - 1
  component additions: L + 1 roundings, not 2 L.  So |Re err| <= gamma_{L+1} * sum_j (|ar||xr| + |ai||xi|) <= gamma_{L+1} * s_i
  (Cauchy-Schwarz per term: |ar||xr| + |ai||xi| <= |a||x|), the same for the imaginary part, and
        |y_i - yhat_i| <= sqrt(2) * gamma_{L+1} * s_i.
  This is the code's constant; it is never larger than the sqrt(2) * gamma_{2 L} of the generic 2 L-term argument (L >= 1).
* The reference itself (`spmv_ext`, np.longdouble, u_ext = eps/2) is not exact: its own error, the same expressions with u_ext,
  is added to the bound (about 2^-11 of the float64 bound on x87 extended precision, nothing where longdouble is wider).
* L = 0: the row is exactly +0 (both zeros with the sign bit clear).

The fused dot of the stream kernel (bound only, `stream_dot_bound`)
-------------------------------------------------------------------
The stream kernel adds, per thread, to_acc(vmul(d_i, sum)) in double in an order that depends on the grid.  For a row that lies
in one chunk `sum` is y_i as stored, so each term is fl_T(d_i y_i): relative error u_T (real) or, by components as above,
sqrt(2) * gamma_2 < 4 u_T (complex); 4 u_T covers both.  The <= n terms are then added in double in some order: gamma^double_n
relative to the sum of their moduli, which is at most (1 + 4 u_T) times sum |d_i||y_i|:
        |sum of partials - d.y_got| <= (4 u_T + gamma^double_n (1 + 4 u_T)) * sum_i |d_i| |y_i|     (+ the reference's own error).
A row that spans C > 1 chunks contributes d_i times each chunk's sum instead of d_i y_i; y_i = fl(sum of the chunk sums) differs
from their exact sum by at most gamma^T_{C-1} * sum_c |sum_c| and sum_c |sum_c| <= (1 + gamma^T_L) s_i, so such a row adds
(4 u_T + gamma^T_C)(1 + gamma^T_L) |d_i| s_i with s_i in place of |y_i|.
"""
import numpy as np

LD = np.longdouble
U_EXT = LD(np.finfo(LD).eps) / 2


def real_type(dtype):
    return np.dtype(dtype).type(0).real.dtype.type


def unit_roundoff(dtype):
    return LD(2) ** (-24 if real_type(dtype) is np.float32 else -53)


def gamma(k, u):
    k = np.asarray(k, dtype=LD)
    return k * u / (1 - k * u)


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def _parts(v, dtype):
    """(re, im) arrays in the real type of `dtype` (im is None for real types)"""
    R = real_type(dtype)
    v = np.asarray(v, dtype=dtype)
    if is_complex(dtype):
        return np.ascontiguousarray(v.real, dtype=R), np.ascontiguousarray(v.imag, dtype=R)
    return np.ascontiguousarray(v, dtype=R), None


def vmul_t(a, x, dtype):
    """device_types.h vmul on (re, im) pairs in T: every operation below is one IEEE operation in T"""
    ar, ai = a
    xr, xi = x
    if ai is None:
        return ar * xr, None
    return (ar * xr) - (ai * xi), (ar * xi) + (ai * xr)


def _join(re, im, dtype):
    if im is None:
        return re.astype(dtype)
    out = np.empty(re.shape, dtype=dtype)
    out.real, out.imag = re, im
    return out


def _walk(ip, ix, da, xk, dtype, start, stride):
    """per row: sum = T(sum + T(a * x)) over the entries start_i, start_i + stride, ... < ip[i + 1], from +0; vectorised over the
    rows by stepping the entry index under a mask"""
    R = real_type(dtype)
    n = len(ip) - 1
    ip = np.asarray(ip, dtype=np.int64)
    ar, ai = _parts(da, dtype)
    xr, xi = _parts(xk, dtype)
    cplx = ai is not None
    sr = np.zeros(n, dtype=R)
    si = np.zeros(n, dtype=R) if cplx else None
    k = start.astype(np.int64).copy()
    end = ip[1:]
    while True:
        m = np.nonzero(k < end)[0]
        if m.size == 0:
            break
        e = k[m]
        c = np.asarray(ix)[e]
        pr, pi = vmul_t((ar[e], ai[e] if cplx else None), (xr[c], xi[c] if cplx else None), dtype)
        sr[m] = sr[m] + pr
        if cplx:
            si[m] = si[m] + pi
        k[m] += stride
    return sr, si


def spmv_in_type(ip, ix, da, x, dtype, nrhs=1):
    """y[r] = A x[r] exactly as every one-lane-per-row kernel forms it; x and the result are (nrhs, n)"""
    n = len(ip) - 1
    x = np.asarray(x, dtype=dtype).reshape(nrhs, n)
    start = np.asarray(ip[:-1], dtype=np.int64)
    out = np.empty((nrhs, n), dtype=dtype)
    with np.errstate(all="ignore"):
        for r in range(nrhs):
            out[r] = _join(*_walk(ip, ix, da, x[r], dtype, start, 1), dtype)
    return out


def spmv_chunked_in_type(ip, ix, da, x, dtype, lpr):
    """the chunked kernel, lpr lanes per row (single right-hand side): (1, n)"""
    n = len(ip) - 1
    x = np.asarray(x, dtype=dtype).reshape(n)
    start = np.asarray(ip[:-1], dtype=np.int64)
    with np.errstate(all="ignore"):
        lanes = [_walk(ip, ix, da, x, dtype, start + l, lpr) for l in range(lpr)]
        re = np.stack([v[0] for v in lanes])                      # [lane][row]
        im = np.stack([v[1] for v in lanes]) if lanes[0][1] is not None else None
        off = lpr // 2
        idx = np.arange(lpr)
        while off > 0:                                            # v += v[lane ^ off] in every lane at once
            re = re + re[idx ^ off]
            if im is not None:
                im = im + im[idx ^ off]
            off //= 2
    return _join(re[0], im[0] if im is not None else None, dtype).reshape(1, n)


def spmv_ext(ip, ix, da, x, dtype, nrhs=1):
    """the same product in np.longdouble (complex as two of them): (re, im or None, s) with s_i = sum_j |a_ij| |x_j|, each (nrhs, n)"""
    n = len(ip) - 1
    ip = np.asarray(ip, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(ip))
    x = np.asarray(x, dtype=dtype).reshape(nrhs, n)
    da = np.asarray(da, dtype=dtype)
    cplx = is_complex(dtype)
    ar, ai = da.real.astype(LD), (da.imag.astype(LD) if cplx else None)
    absa = np.hypot(ar, ai) if cplx else np.abs(ar)
    re = np.zeros((nrhs, n), LD)
    im = np.zeros((nrhs, n), LD) if cplx else None
    s = np.zeros((nrhs, n), LD)
    for r in range(nrhs):
        xr = x[r].real.astype(LD)[ix]
        if cplx:
            xi = x[r].imag.astype(LD)[ix]
            np.add.at(re[r], rows, ar * xr - ai * xi)
            np.add.at(im[r], rows, ar * xi + ai * xr)
            np.add.at(s[r], rows, absa * np.hypot(xr, xi))
        else:
            np.add.at(re[r], rows, ar * xr)
            np.add.at(s[r], rows, absa * np.abs(xr))
    return re, im, s


def row_bound(L, dtype):
    """bound / s_i for a row of L entries, any summation order (module docstring); includes the longdouble reference's own error"""
    L = np.asarray(L, dtype=LD)
    u = unit_roundoff(dtype)
    if is_complex(dtype):
        b = np.sqrt(LD(2)) * (gamma(L + 1, u) + gamma(L + 1, U_EXT))
    else:
        b = gamma(L, u) + gamma(L, U_EXT)
    return np.where(L > 0, b, LD(0))


def bits(a):
    """the bit patterns of a real or complex array (so that -0 != +0 and NaNs compare)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[real_type(a.dtype)(0).itemsize])


def bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_rows(got, ip, ix, da, x, dtype, nrhs=1, ext=None, label=""):
    """every row of every right-hand side within row_bound of spmv_ext; rows without entries exactly +0.  No mask, no filter.
    Prints the largest error / bound ratio before it asserts and returns it."""
    n = len(ip) - 1
    got = np.asarray(got)
    assert got.dtype == np.dtype(dtype) and got.size == nrhs * n, (got.dtype, got.shape)
    got = got.reshape(nrhs, n)
    re, im, s = ext if ext is not None else spmv_ext(ip, ix, da, x, dtype, nrhs)
    L = np.diff(np.asarray(ip, dtype=np.int64))
    bound = row_bound(L, dtype)[None, :] * s
    if im is not None:
        err = np.hypot(got.real.astype(LD) - re, got.imag.astype(LD) - im)
    else:
        err = np.abs(got.astype(LD) - re)
    finite = np.isfinite(err)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
    ratio = np.where(finite, ratio, np.inf)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"check_rows {label}: largest error/bound = {worst:.3g} over {nrhs} x {n} rows")
    bad = np.argwhere(~(ratio <= 1))
    assert bad.size == 0, f"{label}: {len(bad)} rows outside the bound, first (rhs, row) = {bad[0].tolist()}, got {got[tuple(bad[0])]!r}"
    empty = L == 0
    zero_bits = bits(np.zeros(1, dtype=dtype))[0]
    eb = bits(got)[:, np.repeat(empty, 2) if im is not None else empty]
    assert np.all(eb == zero_bits), f"{label}: a row without entries is not exactly +0"
    return worst


def _tree256(v):
    """block_sum<256> on (nb, 256) doubles (or complex128, by components): wave tree, then the four wave sums in order"""
    w = v.reshape(v.shape[0], 4, 64)
    off = 32
    while off > 0:
        w = w[..., :off] + w[..., off:2 * off]
        off //= 2
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _dq_terms(d, y, dtype):
    """to_acc(vmul(d_i, y_i)): product in T, widened to double, padded with zeros to whole 256-row blocks -> (nb, 256)"""
    n = len(y)
    with np.errstate(all="ignore"):
        pr, pi = vmul_t(_parts(d, dtype), _parts(y, dtype), dtype)
    nb = (n + 255) // 256
    t = np.zeros(nb * 256, dtype=np.complex128 if pi is not None else np.float64)
    if pi is not None:
        t.real[:n], t.imag[:n] = pr.astype(np.float64), pi.astype(np.float64)
    else:
        t[:n] = pr.astype(np.float64)
    return t.reshape(nb, 256)


def block_partials_in_type(d, y, dtype):
    """one d.y partial per 256-row block, as the one-lane-per-row kernels form it (d, y: one right-hand side)"""
    with np.errstate(all="ignore"):
        return _tree256(_dq_terms(d, y, dtype))


def block_partials_chunked_in_type(d, y, dtype, lpr):
    """... as the chunked kernel forms it: thread j * lpr adds the rows c * (256 / lpr) + j, c = 0 .. lpr - 1, in that order from
    +0, every other thread holds 0; then the same tree"""
    t = _dq_terms(d, y, dtype)
    rc = 256 // lpr
    v = np.zeros_like(t)
    with np.errstate(all="ignore"):
        acc = np.zeros((t.shape[0], rc), dtype=t.dtype)
        for c in range(lpr):
            acc = acc + t[:, c * rc:(c + 1) * rc]
        v[:, ::lpr] = acc
        return _tree256(v)


def dot_ext(d, y, dtype):
    """(re, im or None, sum |d_i||y_i|) of the unconjugated d.y in longdouble"""
    d, y = np.asarray(d, dtype=dtype), np.asarray(y, dtype=dtype)
    if is_complex(dtype):
        dr, di, yr, yi = (v.astype(LD) for v in (d.real, d.imag, y.real, y.imag))
        return (dr * yr - di * yi).sum(), (dr * yi + di * yr).sum(), (np.hypot(dr, di) * np.hypot(yr, yi)).sum()
    return (d.astype(LD) * y.astype(LD)).sum(), None, (np.abs(d.astype(LD)) * np.abs(y.astype(LD))).sum()


def stream_dot_bound(d, y_got, dtype, ip=None, s_rows=None, chunk=None):
    """bound of |sum of the stream kernel's partials - d.y_got| (module docstring).  With `chunk` (entries per chunk of the
    kernel) rows that span several chunks are priced on s_i = sum_j |a_ij||x_j| instead of |y_i|."""
    n = len(y_got)
    uT, uD = unit_roundoff(dtype), LD(2) ** -53
    d, y = np.asarray(d, dtype=dtype), np.asarray(y_got, dtype=dtype)
    t = np.abs(d).astype(LD) * np.abs(y).astype(LD)
    base = 4 * uT + gamma(n, uD) * (1 + 4 * uT) + gamma(n, U_EXT)
    total = base * t.sum()
    if chunk is not None:
        ip = np.asarray(ip, dtype=np.int64)
        L = np.diff(ip)
        rows = np.arange(n)
        cfirst = ip[rows // 256 * 256] // 4 * 4                  # the chunks of a 256-row block start at its slice start & ~3
        C = np.where(L > 0, (ip[1:] - 1 - cfirst) // chunk - (ip[:-1] - cfirst) // chunk + 1, 1)
        extra = (4 * uT + gamma(C, uT)) * (1 + gamma(L, uT)) * np.abs(d).astype(LD) * s_rows
        total = total + (np.where(C > 1, extra, 0)).sum() * (1 + gamma(n, uD))
    return total


def adversarial_d(rng, n, dtype):
    """magnitudes spread over about 2^30 inside every wave of 64 rows (random exponents, random mantissas), so that the sum of
    d_i y_i depends on the pairing: a tree with two waves exchanged, or a left-to-right sum, has other bits.  The 32-bit types take
    2^48: their products reach the double accumulator with 24-bit significands, and a double sum of such terms is EXACT -- the same
    bits in any order -- unless they spread over more than 2^29."""
    R = real_type(dtype)
    half = 24 if R is np.float32 else 15

    def one():
        return (rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-half, half + 1, n)) * rng.choice([-1.0, 1.0], n)).astype(R)
    if is_complex(dtype):
        return _join(one(), one(), dtype)
    return one().astype(dtype)


# ---- fixtures shared by the host tests (test_spmv_ref.py) and the device tests (test_gpu_spmv_forms.py): pure numpy -----------------
def rand_values(rng, n, dtype):
    """conftest.rand_vec (standard normal components), restated here so that this module imports nothing from the suite"""
    v = rng.standard_normal(n)
    if is_complex(dtype):
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dtype)


def length_set(U, lpr=1):
    """row lengths around the batch length U of the row walk (lpr lanes per row): 0, 1, lpr-1, lpr, lpr+1, U lpr, U lpr + 1 for the
    chunked kernel, 0, 1, U-1, U, U+1, 2U, 2U+1 for the one-lane-per-row kernels"""
    if lpr > 1:
        return [0, 1, lpr - 1, lpr, lpr + 1, U * lpr, U * lpr + 1]
    return [0, 1, U - 1, U, U + 1, 2 * U, 2 * U + 1]


def ragged_lengths(rng, n, lengths, nnz_mod=None, steer=True):
    """row lengths drawn from `lengths` with, where n allows: an empty last row of block 0 (row 255), an empty first row of block 1
    (row 256), a wholly empty row block (rows 512..767), three empty final rows; then, by choosing two rows in front of every block
    boundary from the same set, slice starts ip[256 b] % 4 == b % 4 (so that p0 % 4 takes 0, 1, 2, 3 over five blocks), and
    nnz % 4 == nnz_mod."""
    lengths = list(lengths)
    L = rng.choice(lengths, size=n).astype(np.int64)
    fixed = np.zeros(n, dtype=bool)
    if n == 1:
        L[0] = lengths[4]
        return L

    def force(sl):
        L[sl] = 0
        fixed[sl] = True
    if n >= 256:
        force(slice(255, 256))
    if n > 256:
        force(slice(256, 257))
    if n >= 768:
        force(slice(512, 768))
    force(slice(n - min(3, n - 1), n))

    def steer_rows(r1, r2, upto, target):
        if r1 < 0 or fixed[r1] or fixed[r2]:
            return
        base = int(L[:upto].sum() - L[r1] - L[r2])
        for l1 in lengths:
            for l2 in lengths:
                if (base + l1 + l2) % 4 == target:
                    L[r1], L[r2] = l1, l2
                    fixed[r1] = fixed[r2] = True
                    return
    if steer:
        for b in range(1, (n + 255) // 256):
            steer_rows(256 * b - 3, 256 * b - 2, 256 * b, b % 4 if b < 3 else (b - 1) % 4)
    if nnz_mod is not None:
        steer_rows(n - 6, n - 5, n, nnz_mod)
        assert int(L.sum()) % 4 == nnz_mod
    return L


def banded_matrix(rng, L, offsets, dtype, palette=None, wrap=True):
    """CSR with row lengths L, entry columns row + one of `offsets`, drawn with replacement (duplicates inside a row are legal CSR
    and the kernels must not care), unsorted.  wrap: columns are taken mod n, so rows near either end carry offsets +- n as well
    (large positive ones at row 0, large negative ones at the last rows); else an offset that leaves the matrix is mirrored
    (`offsets` symmetric, reach < n / 2: the set of column - row stays `offsets`).  Values: standard normal, or drawn from
    `palette`, every palette entry used at least once where there are that many entries."""
    n = len(L)
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(L, out=ip[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), L)
    offs = rng.choice(np.asarray(offsets, dtype=np.int64), size=rows.size)
    if wrap:
        ix = ((rows + offs) % n).astype(np.int32)
    else:
        out = (rows + offs < 0) | (rows + offs >= n)
        offs = np.where(out, -offs, offs)
        ix = (rows + offs).astype(np.int32)
        assert ix.size == 0 or (ix.min() >= 0 and ix.max() < n)
    if palette is None:
        da = rand_values(rng, rows.size, dtype)
    else:
        idx = rng.integers(0, len(palette), rows.size)
        k = min(len(palette), rows.size)
        idx[rng.permutation(rows.size)[:k]] = np.arange(k)
        da = np.asarray(palette, dtype=dtype)[idx]
    return ip, ix, da


def toeplitz_matrix(rng, n, offsets, dtype, palette=None):
    """row i holds the entries i + off, off in `offsets` in the order given, that lie inside the matrix: the pattern of a stencil
    ((-1, 0, 1): a tridiagonal chain; (-nx, -1, 0, 1, nx): a 5-point grid; (-nx ny, -nx, -1, 0, 1, nx, nx ny): a 7-point grid)"""
    rows = np.repeat(np.arange(n, dtype=np.int64), len(offsets))
    cols = rows + np.tile(np.asarray(offsets, dtype=np.int64), n)
    keep = (cols >= 0) & (cols < n)
    rows, cols = rows[keep], cols[keep]
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=ip[1:])
    if palette is None:
        da = rand_values(rng, cols.size, dtype)
    else:
        idx = rng.integers(0, len(palette), cols.size)
        k = min(len(palette), cols.size)
        idx[rng.permutation(cols.size)[:k]] = np.arange(k)
        da = np.asarray(palette, dtype=dtype)[idx]
    return ip, cols.astype(np.int32), da


def pair_matrix(rng, n, row_len, offsets, palette, dtype, extra_pair=False):
    """every (offset, value) pair of `offsets` x `palette` occurs (offsets symmetric, no wrap): len(offsets) * len(palette) distinct
    pairs exactly; extra_pair: one entry more carries a value of its own (one pair and one value more)"""
    L = np.full(n, row_len, dtype=np.int64)
    ip, ix, da = banded_matrix(rng, L, offsets, dtype, wrap=False)
    reach = int(np.max(np.abs(offsets)))
    rows = np.repeat(np.arange(n, dtype=np.int64), L)
    inner = np.nonzero((rows >= reach) & (rows < n - reach))[0]
    k = len(offsets) * len(palette)
    assert inner.size > k
    da = np.asarray(palette, dtype=dtype)[rng.integers(0, len(palette), rows.size)]
    pick = inner[:k]
    ix[pick] = (rows[pick] + np.repeat(np.asarray(offsets, dtype=np.int64), len(palette))).astype(np.int32)
    da[pick] = np.tile(np.asarray(palette, dtype=dtype), len(offsets))
    if extra_pair:
        da[inner[k]] = np.asarray(palette, dtype=dtype).sum() + 3      # a value the palette does not hold
    return ip, ix, da


def distinct_pairs(ip, ix, da):
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    off = (np.asarray(ix, dtype=np.int64) - rows).tolist()
    vb = [tuple(b) for b in bits(np.asarray(da)).reshape(len(off), -1).tolist()]
    return len(set(zip(off, vb)))


def distinct_values(da):
    return len(set(tuple(b) for b in bits(np.asarray(da)).reshape(len(da), -1).tolist()))


def palette_values(rng, k, dtype):
    """k distinct values (distinct bit patterns)"""
    while True:
        p = rand_values(rng, k, dtype)
        if distinct_values(p) == k:
            return p


def offsets8(rng, count=40, reach=60):
    """`count` distinct offsets in [-reach, reach]: with the wrapped copies at most 3 * count <= 256 distinct column - row"""
    return rng.choice(np.arange(-reach, reach + 1), size=count, replace=False)


def offsets16(rng, count=600, reach=2000):
    """more than 256 distinct offsets: no one-byte dictionary; blocks span fewer than 65 536 columns at n < 65 536"""
    return rng.choice(np.arange(-reach, reach + 1), size=count, replace=False)


def distinct_offsets(ip, ix):
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    return np.unique(np.asarray(ix, dtype=np.int64) - rows).size


def plan_spans(ip):
    """host copy of spmv_span_kernel: [largest p1 - (p0 & ~3) over the 256 >> lv - row slices, lv = 0..5], longest row"""
    ip = np.asarray(ip, dtype=np.int64)
    n = len(ip) - 1
    spans = []
    for lv in range(6):
        rows = 256 >> lv
        starts = np.arange(0, n, rows)
        ends = np.minimum(starts + rows, (starts // 256 + 1) * 256)
        ends = np.minimum(ends, n)
        spans.append(int((ip[ends] - (ip[starts] // 4 * 4)).max()) if n else 0)
    return spans, int(np.diff(ip).max()) if n else 0


def slice_starts_mod4(ip):
    n = len(ip) - 1
    return sorted(set(int(ip[r]) % 4 for r in range(0, n, 256)))
