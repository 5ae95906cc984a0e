"""Host tests of tests/spmv_ref.py, the reference the device tests of the SpMV forms (test_gpu_spmv_forms.py) are held to: the
restatements stay inside the textbook bound of the extended-precision product, the extended product agrees with scipy, the
block-sum tree agrees with math.fsum, the restatement is sensitive to the order it claims, and the checks reject the mistakes a
kernel could make (each applied to a correct host result)."""
import math

import numpy as np
import pytest

import spmv_ref as R
from conftest import ALL_DTYPES, rand_vec

IDS = {np.float32: "f32", np.float64: "f64", np.complex64: "c64", np.complex128: "c128"}


def _ragged(dtype, n=1287, U=8, nnz_mod=1, seed=11):
    rng = np.random.default_rng(seed)
    L = R.ragged_lengths(rng, n, R.length_set(U), nnz_mod)
    ip, ix, da = R.banded_matrix(rng, L, R.offsets8(rng), dtype)
    return ip, ix, da, rand_vec(rng, n, dtype)


def _dense(dtype, lpr, seed=12):
    rng = np.random.default_rng(seed)
    n = 256 + 256 // lpr + 1
    L = R.ragged_lengths(rng, n, R.length_set(4, lpr), steer=False)
    ip, ix, da = R.banded_matrix(rng, L, R.offsets16(rng, 200, 120), dtype)
    return ip, ix, da, rand_vec(rng, n, dtype)


def test_fixture_has_the_edges_it_promises():
    ip, ix, da, _ = _ragged(np.float64)
    L = np.diff(ip)
    assert R.slice_starts_mod4(ip) == [0, 1, 2, 3] and ip[-1] % 4 == 1
    assert L[255] == 0 and L[256] == 0 and np.all(L[512:768] == 0) and np.all(L[-3:] == 0)
    assert set(L.tolist()) == set(R.length_set(8))
    assert R.distinct_offsets(ip, ix) <= 256
    rows = np.repeat(np.arange(len(L)), L)
    off = ix.astype(np.int64) - rows
    assert off[rows < 60].max() > 1000 and off[rows > len(L) - 70].min() < -1000      # the wrapped offsets at either end


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS.get)
def test_restatements_stay_inside_the_bound(dtype):
    ip, ix, da, x = _ragged(dtype)
    ext = R.spmv_ext(ip, ix, da, x, dtype)
    y = R.spmv_in_type(ip, ix, da, x, dtype)
    worst = R.check_rows(y, ip, ix, da, x, dtype, ext=ext, label="in type")
    assert 0 < worst <= 1
    for lpr in (2, 8, 32):
        ipd, ixd, dad, xd = _dense(dtype, lpr)
        yc = R.spmv_chunked_in_type(ipd, ixd, dad, xd, dtype, lpr)
        R.check_rows(yc, ipd, ixd, dad, xd, dtype, label=f"chunked {lpr}")
        y1 = R.spmv_in_type(ipd, ixd, dad, xd, dtype)
        assert not R.bit_equal(yc, y1)              # another order: other bits (or the chunked restatement restates nothing)
        short = np.diff(ipd) <= 1                   # ... but a row of at most one entry has one order only
        assert R.bit_equal(yc[:, short], y1[:, short])


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS.get)
def test_extended_product_agrees_with_scipy(dtype):
    import scipy.sparse as sp
    ip, ix, da, x = _ragged(dtype)
    n = len(ip) - 1
    wide = np.complex128 if R.is_complex(dtype) else np.float64
    A = sp.csr_matrix((da.astype(wide), ix, ip), shape=(n, n))
    want = A @ x.astype(wide)
    re, im, s = R.spmv_ext(ip, ix, da, x, dtype)
    got = re[0].astype(np.float64) + (1j * im[0].astype(np.float64) if im is not None else 0)
    L = np.diff(ip)
    tol = (np.sqrt(2) * (L + 1) if im is not None else L) * 2.0 ** -53 * 1.01 * s[0].astype(np.float64) + 2.0 ** -52 * np.abs(want)
    assert np.all(np.abs(got - want) <= tol)
    # multi-RHS: right-hand side r is the product with x[r]
    X = np.stack([x, x[::-1]])
    re2, _, _ = R.spmv_ext(ip, ix, da, X, dtype, nrhs=2)
    assert np.array_equal(re2[0], re[0]) and not np.array_equal(re2[1], re[0])


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS.get)
def test_block_tree_agrees_with_fsum_and_depends_on_the_order(dtype):
    rng = np.random.default_rng(3)
    n = 1287
    d = R.adversarial_d(rng, n, dtype)
    y = rand_vec(rng, n, dtype)
    part = R.block_partials_in_type(d, y, dtype)
    assert part.shape == (6,) and part.dtype == (np.complex128 if R.is_complex(dtype) else np.float64)
    terms = R._dq_terms(d, y, dtype)
    g = float(R.gamma(255, R.LD(2) ** -53))
    ltr = np.zeros_like(part)
    for b in range(6):
        for comp in ("real", "imag") if R.is_complex(dtype) else ("real",):
            t = getattr(terms[b], comp)
            exact = math.fsum(t.tolist())
            assert abs(getattr(part[b], comp) - exact) <= g * math.fsum(np.abs(t).tolist())
        acc = terms[b][0] * 0
        for v in terms[b]:
            acc = acc + v
        ltr[b] = acc
    # the adversarial d makes the pairing visible: left to right has other bits (two orders may still round alike in a block)
    assert sum(not R.bit_equal(part[b:b + 1], ltr[b:b + 1]) for b in range(5)) >= 3
    # rows past n contribute nothing: the last block is the tree over 7 rows
    assert R.bit_equal(part[5:6], R.block_partials_in_type(d[1280:], y[1280:], dtype))
    # the chunked kernel's arrangement is another order again
    for lpr in (2, 32):
        pc = R.block_partials_chunked_in_type(d, y, dtype, lpr)
        assert not R.bit_equal(pc[:5], part[:5])
        assert np.allclose(pc, part, rtol=1e-9, atol=0)


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS.get)
def test_mutations_are_rejected(dtype):
    ip, ix, da, x = _ragged(dtype)
    n = len(ip) - 1
    L = np.diff(ip)
    X = np.stack([x, np.roll(x, 5)])
    ext = R.spmv_ext(ip, ix, da, X, dtype, nrhs=2)
    good = R.spmv_in_type(ip, ix, da, X, dtype, nrhs=2)
    R.check_rows(good, ip, ix, da, X, dtype, nrhs=2, ext=ext, label="correct")

    def check(y):
        R.check_rows(y, ip, ix, da, X, dtype, nrhs=2, ext=ext, label="mutant")

    def with_matrix(ip2, ix2, da2):
        return R.spmv_in_type(ip2, ix2, da2, X, dtype, nrhs=2)

    # one row's last entry dropped
    row = int(np.nonzero(L == 17)[0][3])
    da2 = da.copy()
    da2[ip[row + 1] - 1] = 0
    m = with_matrix(ip, ix, da2)
    assert not R.bit_equal(m, good)
    _rejected(lambda: check(m))
    # one entry's column off by one
    ix2 = ix.copy()
    e = int(ip[row] + 2)
    ix2[e] = (ix2[e] + 1) % n
    m = with_matrix(ip, ix2, da)
    _rejected(lambda: check(m))
    # a row that starts its block takes the previous block's last entry as well (block 4 starts at row 1024)
    first = 1024 + int(np.nonzero(L[1024:] > 0)[0][0])
    assert np.all(L[1024:first] == 0)
    ip2 = ip.copy()
    ip2[1024:first + 1] -= 1
    m = with_matrix(ip2, ix, da)
    _rejected(lambda: check(m))
    # an empty row left at the prefill value
    m = good.copy()
    m[1, 600] = np.nan
    _rejected(lambda: check(m))
    m = good.copy()
    m[0, 255] = -0.0                                  # ... or at a zero of the wrong sign
    _rejected(lambda: check(m))
    # two right-hand sides swapped
    _rejected(lambda: check(good[::-1].copy()))
    # a few ulps off in one row, still inside the bound: only the bit comparison sees it
    m = good.copy()
    r8 = int(np.nonzero(L == 16)[0][0])
    v = m[0, r8:r8 + 1].view(R.real_type(dtype))
    for _ in range(3):
        v[0] = np.nextafter(v[0], R.real_type(dtype)(np.inf))
    check(m)
    assert not R.bit_equal(m, good)

    # the partials
    d = R.adversarial_d(np.random.default_rng(4), n, dtype)
    y = good[0]
    part = R.block_partials_in_type(d, y, dtype)
    # one block partial missing its last row
    y2 = y.copy()
    y2[1023] = 0
    assert L[1023] > 0 and y[1023] != 0
    p2 = R.block_partials_in_type(d, y2, dtype)
    assert not R.bit_equal(p2[3:4], part[3:4]) and R.bit_equal(np.delete(p2, 3), np.delete(part, 3))
    # waves 1 and 2 exchanged before the final adds: ((w0 + w1) + w2) + w3 with w = (1, 2^53, -2^53, 0) is 0, exchanged it is 1
    dc, yc = np.zeros(256, dtype=dtype), np.ones(256, dtype=dtype)
    dc[0], dc[64], dc[128] = 1, 2.0 ** 53, -2.0 ** 53
    terms = R._dq_terms(dc, yc, dtype)
    assert R.block_partials_in_type(dc, yc, dtype)[0] == 0
    assert R._tree256(terms.reshape(-1, 4, 64)[:, [0, 2, 1, 3], :].reshape(-1, 256))[0] == 1


def test_row_bound_constants():
    u32, u64 = 2.0 ** -24, 2.0 ** -53
    assert float(R.row_bound(0, np.float32)) == 0 and float(R.row_bound(0, np.complex128)) == 0
    assert math.isclose(float(R.row_bound(7, np.float32)), 7 * u32 / (1 - 7 * u32), rel_tol=1e-6)
    assert math.isclose(float(R.row_bound(7, np.complex64)), math.sqrt(2) * 8 * u32 / (1 - 8 * u32), rel_tol=1e-6)
    assert math.isclose(float(R.row_bound(7, np.float64)), 7 * u64 / (1 - 7 * u64), rel_tol=2e-3)       # + the reference's own error
    # the complex constant, gamma_{L+1}, is the helpers' own count of roundings: attained to within a factor by a row of one entry
    a, x = np.complex64(1 + 2 ** -12 + 1j), np.complex64(1 + 2 ** -12 + 1j * (1 - 2 ** -12))
    ip, ix = np.array([0, 1], np.int32), np.array([0], np.int32)
    got = R.spmv_in_type(ip, ix, np.array([a]), np.array([x]), np.complex64)
    assert R.check_rows(got, ip, ix, np.array([a]), np.array([x]), np.complex64, label="one entry") <= 1
