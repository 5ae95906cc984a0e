"""The reference and the checker of the tridiagonal sweep tests (tridiag_pcg.thomas_ext / sweep_in_type / segments /
check_sweep) on the host: the extended-precision solve against scipy, and proof that the checker can fail -- it accepts the
sequential sweep and rejects five mutations of it, each the signature of a kernel fault that whole-PCG norms would absorb."""
import numpy as np
import pytest
import scipy.linalg as sla

import tridiag_pcg as tp

CHUNK = {np.dtype(np.float32): 2048, np.dtype(np.float64): 1024}      # rows per chunk of the scan sweep (256 threads x 32 bytes)


def chain(rng, n, stride=1, shift=0.1, cplx=False):
    """couplings -U(0.2, 1) (symmetric), diagonal (1 + shift)(|lower| + |upper|); complex: every entry with a phase in +-0.3"""
    off = -rng.uniform(0.2, 1.0, n - stride)
    if cplx:
        off = off * np.exp(1j * rng.uniform(-0.3, 0.3, n - stride))
    lower, upper = np.zeros(n, off.dtype), np.zeros(n, off.dtype)
    lower[stride:], upper[:n - stride] = off, off
    diag = (1.0 + shift) * (np.abs(lower) + np.abs(upper))
    if cplx:
        diag = diag * np.exp(1j * rng.uniform(-0.3, 0.3, n))
    return lower, diag, upper


def cut(lower, upper, rows, stride=1):
    for i in rows:
        lower[i] = 0
        upper[i - stride] = 0


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18          # the fp64 kernels are judged against it


@pytest.mark.parametrize("stride", [1, 3, 7])
def test_thomas_ext_against_solve_banded(stride):
    """complex128 systems of 50 rows (chains of unequal length at stride 3 and 7), two right-hand sides, with cuts"""
    rng = np.random.default_rng(3)
    n = 50
    lower, diag, upper = chain(rng, n, stride, shift=0.3, cplx=True)
    cut(lower, upper, [20, 33], stride)
    r = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    ab = np.zeros((2 * stride + 1, n), complex)
    ab[0, stride:], ab[stride], ab[-1, :n - stride] = upper[:n - stride], diag, lower[stride:]
    want = sla.solve_banded((stride, stride), ab, r.T).T
    got = tp.thomas_ext(lower, diag, upper, r, stride)
    assert got.dtype == np.clongdouble
    assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-14
    z = tp.sweep_in_type(lower, diag, upper, r, np.complex128, stride)
    assert z.dtype == np.complex128 and np.max(np.abs(z - want)) / np.max(np.abs(want)) < 1e-14
    # the residual of the extended solve, taken in extended precision, is far below double
    zz = np.zeros((2, n + 2 * stride), np.clongdouble)
    zz[:, stride:n + stride] = got
    res = lower * zz[:, :n] + diag * got + upper * zz[:, 2 * stride:] - r
    assert np.max(np.abs(res)) < 1e-17


def test_segments_rule():
    """a cut needs both couplings zero; stride 3 with chains of 4, 3, 3 rows"""
    rng = np.random.default_rng(4)
    lower, diag, upper = chain(rng, 12)
    cut(lower, upper, [5])
    lower[8] = 0                      # one-sided: no cut
    upper[2] = 0                      # one-sided: no cut
    assert tp.segments(lower, diag, upper, np.float64).tolist() == [[0, 5, 1], [5, 7, 1]]
    lo2, up2 = lower.copy(), upper.copy()
    lo2[9] = up2[8] = -1e-50          # both stored couplings round to zero in fp32 only
    assert tp.segments(lo2, diag, up2, np.float64).tolist() == [[0, 5, 1], [5, 7, 1]]
    assert tp.segments(lo2, diag, up2, np.float32).tolist() == [[0, 5, 1], [5, 4, 1], [9, 3, 1]]
    lower, diag, upper = chain(rng, 10, stride=3)
    cut(lower, upper, [7], stride=3)
    assert tp.segments(lower, diag, upper, np.float64, 3).tolist() == [[0, 4, 3], [1, 2, 3], [2, 3, 3], [7, 1, 3]]


def system(dtype):
    """2 C + 301 rows: a low-magnitude segment [40, 70), cuts at 40, 70, 700 and C + 300, so the segment [700, C + 300) crosses
    the chunk boundary at C; two right-hand sides"""
    dtype = np.dtype(dtype)
    C = CHUNK[dtype]
    rng = np.random.default_rng(17)
    n = 2 * C + 301
    lower, diag, upper = (v.astype(dtype) for v in chain(rng, n, shift=0.5))
    cuts = [40, 70, 700, C + 300]
    cut(lower, upper, cuts)
    r = rng.standard_normal((2, n))
    r[:, 40:70] *= 1e-6
    r = r.astype(dtype)
    segs = tp.segments(lower, diag, upper, dtype)
    assert segs[:, 0].tolist() == [0] + cuts
    return lower, diag, upper, r, segs, C


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_check_sweep_accepts_the_sequential_sweep_and_rejects_faults(dtype, capsys):
    lower, diag, upper, r, segs, C = system(dtype)
    eps = np.finfo(dtype).eps
    z_ref = tp.thomas_ext(lower, diag, upper, r)
    z_seq = tp.sweep_in_type(lower, diag, upper, r, dtype)
    assert z_seq.dtype == np.dtype(dtype)
    figures = tp.check_sweep(z_seq, z_ref, z_seq, segs, dtype, "sequential")
    assert "e(z_seq)" in capsys.readouterr().out                      # the figures are printed
    assert all(0 < e_seq < 8 * eps and e_dev == e_seq for e_dev, e_seq in figures)

    def rejected(z, what):
        with pytest.raises(AssertionError):
            tp.check_sweep(z, z_ref, z_seq, segs, dtype, what)

    # a segment cut ignored: the sweeps run through row 700 with the couplings the matrix had before the cut
    nl, ne, w = (f.astype(dtype) for f in tp._factors(lower, diag, upper, 1, np.float64))
    nl2, ne2 = nl.copy(), ne.copy()
    nl2[700], ne2[699] = nl[701], ne[698]
    y = tp._recurrence(nl2, r, 1)
    rejected(tp._recurrence(ne2, w * y, 1, reverse=True), "cut ignored")
    # the carry-in of the second chunk zeroed: the forward sweep restarts at row C
    nl2 = nl.copy()
    nl2[C] = 0
    y = tp._recurrence(nl2, r, 1)
    rejected(tp._recurrence(ne, w * y, 1, reverse=True), "carry-in zeroed")
    # one row left stale (it keeps r, what the storage held before)
    z = z_seq.copy()
    z[0, C + 7] = r[0, C + 7]
    rejected(z, "stale row")
    # right-hand side 1 holds right-hand side 0's answer
    z = z_seq.copy()
    z[1] = z_seq[0]
    rejected(z, "rhs 1 = rhs 0")
    # one element of the low-magnitude segment off by 64 eps of that segment's scale: 1e-6 of it on the scale of the whole vector
    z = z_seq.copy()
    z[0, 55] += dtype(64 * eps * np.max(np.abs(z_seq[0, 40:70])))
    assert np.max(np.abs(z - z_seq)) / np.max(np.abs(z_seq)) < 1e-3 * eps
    rejected(z, "64 eps in a small segment")
    # ... and a NaN is no pass
    z = z_seq.copy()
    z[1, 3] = np.nan
    rejected(z, "NaN")
