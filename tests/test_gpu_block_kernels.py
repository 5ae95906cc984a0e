"""The kernels of block CG (csrc/block_cg.hip) one by one, BIT FOR BIT against the type-true restatement tests/block_ref.py.

The three vector kernels run alone through cgamd_block_gram, cgamd_block_update_xw and cgamd_block_update_qp on random data: float32
and float64, s in {2, 9, 16}, size in {957 (four work-groups, the last one ragged), 4096 + 3, 512 * 256 + 256 + 5 (beyond the cap of
the Gram grid: a thread owns rows of two passes, the second pass ragged)}.  Every block lies in a canary buffer
(tests/canary_buffers.py), once with its columns on 16-byte boundaries (ld whole packs) and once not (ld = size + 1 behind a pointer
one value off a boundary): one thread owns a row, so both take the same path and must give the same bits, and the whole buffer is
compared -- the rows between size and ld and the bytes around keep theirs, what is only read stays.  Q and P are updated in place.
The entries below the diagonal of tau^-1 and tau are NaN: the kernel must not read them.

The small steps run on a handle (33 x 29 Laplacian): after set_rhs and after each of three iterations the matrices they leave
(cgamd_solver_block_state) are compared bit for bit with the float64 restatement of the same elimination order, fed with the device's
own summed Gram matrices; after set_rhs (x0 = 0, so R0 = b exactly) the summed R0^T R0 itself is compared with the restated partials
and their restated sum."""
import numpy as np
import pytest

import block_ref as B
import shift_ref as R
from canary_buffers import Embedded

pytestmark = pytest.mark.gpu

SIZES = (957, 4096 + 3, 512 * 256 + 256 + 5)
BLOCKS = (2, 9, 16)
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def env(pkg, gpu):
    return pkg, gpu[0], pkg._lib.load()


def _layouts(dtype, size):
    E = 16 // np.dtype(dtype).itemsize
    return (((size + E - 1) // E * E + E, 0, "packs"), (size + 1, np.dtype(dtype).itemsize, "off a boundary"))


def _block(rng, s, size, dtype):
    return rng.standard_normal((s, size)).astype(dtype)


def _upper(rng, s, dtype):
    m = rng.standard_normal((s, s)).astype(dtype)
    m[np.tril_indices(s, -1)] = np.nan
    return m


def _partials(pkg, ctx, s, size):
    return pkg.DeviceBuffer(ctx, hostbuf=np.full(s * (s + 1) // 2 * B.gram_grid(size), np.nan))


def _same(got, want, what):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what}: {int(np.count_nonzero(got != want))} values differ"


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("s", BLOCKS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_vector_kernels_bit_for_bit(env, dtype, s, size):
    pkg, ctx, lib = env
    dtype = np.dtype(dtype)
    code = pkg._lib.DTYPE_CODE[dtype]
    rng = np.random.default_rng(1000 * s + size % 997)
    grid = lib.cgamd_block_gram_grid(size)
    assert grid == B.gram_grid(size)
    P, AP, X, Q = (_block(rng, s, size, dtype) for _ in range(4))
    M, al = (rng.standard_normal((s, s)).astype(dtype) for _ in range(2))
    ti, tau = _upper(rng, s, dtype), _upper(rng, s, dtype)
    want_g = B.gram_partials(P, AP)
    want_x, want_w = B.update_xw(P, AP, X, Q, M, al)
    want_ww = B.gram_partials(want_w, want_w)
    tz, tauz = np.nan_to_num(ti), np.nan_to_num(tau)          # (the restatement reads the upper triangle only, as stored)
    want_q, want_p = B.update_qp(Q, P, np.triu(tz), np.triu(tauz))
    want_q0, _ = B.update_qp(Q, P, np.triu(tz), np.triu(tauz), init=True)
    coef = {k: pkg.DeviceBuffer(ctx, hostbuf=np.ascontiguousarray(v)) for k, v in (("M", M), ("al", al), ("ti", ti), ("tau", tau))}
    for ld, off, name in _layouts(dtype, size):
        what = f"{dtype.name} s {s} size {size} {name}"
        # Gram: both blocks only read
        ea, eb = Embedded(pkg, ctx, P, ld, off), Embedded(pkg, ctx, AP, ld, off)
        part = _partials(pkg, ctx, s, size)
        pkg._lib.check(lib.cgamd_block_gram(ctx.handle, code, size, ld, s, ea.ptr, eb.ptr, part.ptr))
        ctx.synchronize()
        _same(part.get().reshape(-1, grid), want_g, "Gram partials " + what)
        ea.check("a " + what)
        eb.check("b " + what)
        # X += P M, W = Q - AP alpha over Q, partials of W^T W
        ex, eq = Embedded(pkg, ctx, X, ld, off), Embedded(pkg, ctx, Q, ld, off)
        part2 = _partials(pkg, ctx, s, size)
        pkg._lib.check(lib.cgamd_block_update_xw(ctx.handle, code, size, ld, s, ea.ptr, eb.ptr, ex.ptr, eq.ptr, coef["M"].ptr, coef["al"].ptr,
                                                 part2.ptr))
        ctx.synchronize()
        ex.check("x " + what, want_x)
        eq.check("w " + what, want_w)
        ea.check("p behind the update " + what)
        eb.check("ap behind the update " + what)
        _same(part2.get().reshape(-1, grid), want_ww, "W^T W partials " + what)
        # Q <- W tau^-1, P <- Q + P tau^T, in place
        e1, e2 = Embedded(pkg, ctx, Q, ld, off), Embedded(pkg, ctx, P, ld, off)
        pkg._lib.check(lib.cgamd_block_update_qp(ctx.handle, code, size, ld, s, e1.ptr, e2.ptr, coef["ti"].ptr, coef["tau"].ptr, 0))
        ctx.synchronize()
        e1.check("q " + what, want_q)
        e2.check("p " + what, want_p)
        # set_rhs: P <- Q whatever P held (canary throughout: nothing of it may be read into the result)
        e3, e4 = Embedded(pkg, ctx, Q, ld, off), Embedded(pkg, ctx, P, ld, off, blank=True)
        pkg._lib.check(lib.cgamd_block_update_qp(ctx.handle, code, size, ld, s, e3.ptr, e4.ptr, coef["ti"].ptr, coef["tau"].ptr, 1))
        ctx.synchronize()
        e3.check("q, init " + what, want_q0)
        e4.check("p, init " + what, want_q0)
        for e in (ea, eb, ex, eq, e1, e2, e3, e4):
            e.buf.release()
        part.release()
        part2.release()
    for k, v in (("M", M), ("al", al), ("ti", ti), ("tau", tau)):
        assert coef[k].get().tobytes() == v.tobytes(), "the factors are only read"
        coef[k].release()


def test_entries_refuse_what_they_do_not_serve(env):
    pkg, ctx, lib = env
    E = pkg._lib.ERR_INVALID
    buf = pkg.DeviceBuffer(ctx, hostbuf=np.zeros(64))
    p = buf.ptr
    for dtype, size, ld, s in ((2, 4, 4, 2), (3, 4, 4, 2), (1, 0, 4, 2), (1, 5, 4, 2), (1, 4, 4, 1), (1, 4, 4, 17)):
        assert lib.cgamd_block_gram(ctx.handle, dtype, size, ld, s, p, p, p) == E
        assert lib.cgamd_block_update_xw(ctx.handle, dtype, size, ld, s, p, p, p, p, p, p, p) == E
        assert lib.cgamd_block_update_qp(ctx.handle, dtype, size, ld, s, p, p, p, p, 0) == E
    assert lib.cgamd_block_gram(ctx.handle, 1, 4, 4, 2, p, None, p) == E
    buf.release()


def _entries(Cm, s):
    return np.array([Cm[i, j] for i, j in B.pairs(s)])


@pytest.mark.parametrize("s", (2, 9, 16))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_small_steps_bit_for_bit(env, dtype, s):
    pkg, ctx, _ = env
    dtype = np.dtype(dtype)
    eps = B.EPS[dtype]
    A = R.laplace2d(33, 29)
    n = A.shape[0]
    b = np.random.default_rng(11).standard_normal((n, s)).astype(dtype)
    sv = pkg.Solver(ctx, n, A.nnz, A.data.astype(dtype), A.indptr, A.indices, s)
    try:
        sv.set_block(True)
        sv.set_rhs(np.ascontiguousarray(b.T))
        # R0 = b exactly (x0 = 0): the summed R0^T R0, from the restated partials of the handle's padded rows and their restated sum
        ld = sv.ld
        bp = np.zeros((s, ld), dtype)
        bp[:, :n] = b.T
        C = sv.block_state("C")
        _same(_entries(C, s), B.sum_partials(B.gram_partials(bp, bp)), f"{dtype.name} s {s}: R0^T R0 as summed")
        assert np.array_equal(C, C.T)
        st = B.small2(_entries(C, s), None, s, eps)
        for name in ("tau", "tau_inv", "xi"):
            _same(sv.block_state(name), st[name], f"{dtype.name} s {s} set_rhs {name}")
        _same(sv.history()[0], st["delta"].astype(dtype), f"{dtype.name} s {s} delta_0")
        xi, ratio = st["xi"].tolist(), st["ratio"]
        for k in range(1, 4):
            sv.iterate(1)
            G = sv.block_state("G")
            s1 = B.small1(_entries(G, s), xi, s, eps)
            assert s1["status"] == 0
            for name in ("alpha", "M"):
                _same(sv.block_state(name), s1[name], f"{dtype.name} s {s} iteration {k} {name}")
            s2 = B.small2(_entries(sv.block_state("C"), s), xi, s, eps)
            assert s2["status"] == 0
            for name in ("tau", "tau_inv", "xi"):
                _same(sv.block_state(name), s2[name], f"{dtype.name} s {s} iteration {k} {name}")
            _same(sv.history()[k], s2["delta"].astype(dtype), f"{dtype.name} s {s} delta_{k}")
            xi, ratio = s2["xi"].tolist(), min(ratio, s1["ratio"], s2["ratio"])
        status = sv.block_status()
        assert (status["on"], status["status"], status["s"]) == (True, 0, s)
        assert status["min_pivot_ratio"] == ratio
    finally:
        sv.close()
