"""The kernels of preconditioned block CG (csrc/block_pcg.hip) one by one, BIT FOR BIT against the type-true restatement
tests/block_pcg_ref.py.

The two vector kernels run alone through cgamd_block_gram_weighted and cgamd_block_update_qp_z on random data: float32 and float64,
s in {2, 9, 16}, size 957 (four work-groups, the last one ragged) at ld 957 and at ld 960, and sizes 1 and 257 (one row; one row
into the second work-group) at ld = size.  The q / p update runs in its z-form (Z a block) and its m-form (z_k = m_i w_k, no Z) and
with init 0 and 1.  Every block lies in a canary buffer (tests/canary_buffers.py) and the whole buffer is compared: the rows between
size and ld and the bytes around keep theirs, what is only read stays.  The entries below the diagonal of tau^-1 and tau are NaN: the
kernel must not read them.

The small steps run on a handle (33 x 29, A = D^1/2 L D^1/2 of block_pcg_cases, a diagonal M from the caller's array): after set_rhs
and after one iteration the matrices they leave (cgamd_solver_block_state) and the history row are compared bit for bit with the
float64 restatement fed with the device's own summed W^T W and W^T Z; after set_rhs (x0 = 0, so R0 = b exactly) the summed R0^T R0 and
R0^T Z0 themselves are compared with the restated partials and their restated sum."""
import numpy as np
import pytest

import block_pcg_cases as C
import block_pcg_ref as BP
import block_ref as B
from canary_buffers import Embedded

pytestmark = pytest.mark.gpu

LAYOUTS = ((957, 957), (957, 960), (1, 1), (257, 257))
BLOCKS = (2, 9, 16)
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def env(pkg, gpu):
    return pkg, gpu[0], pkg._lib.load()


def _upper(rng, s, dtype):
    m = rng.standard_normal((s, s)).astype(dtype)
    m[np.tril_indices(s, -1)] = np.nan
    return m


def _same(got, want, what):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what}: {int(np.count_nonzero(got != want))} values differ"


@pytest.mark.parametrize("size,ld", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("s", BLOCKS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_vector_kernels_bit_for_bit(env, dtype, s, size, ld):
    pkg, ctx, lib = env
    dtype = np.dtype(dtype)
    code = pkg._lib.DTYPE_CODE[dtype]
    rng = np.random.default_rng(1000 * s + size + ld)
    grid = lib.cgamd_block_gram_grid(size)
    assert grid == B.gram_grid(size)
    W, Z, P = (rng.standard_normal((s, size)).astype(dtype) for _ in range(3))
    m = rng.uniform(0.5, 2.0, size).astype(dtype)
    ti, tau = _upper(rng, s, dtype), _upper(rng, s, dtype)
    tz, tauz = np.triu(np.nan_to_num(ti)), np.triu(np.nan_to_num(tau))     # (the restatement reads the upper triangle only, as stored)
    what = f"{dtype.name} s {s} size {size} ld {ld}"
    coef = {k: pkg.DeviceBuffer(ctx, hostbuf=np.ascontiguousarray(v)) for k, v in (("ti", ti), ("tau", tau))}
    em = Embedded(pkg, ctx, m[None, :], size)
    # the weighted Gram: W and m only read
    ew = Embedded(pkg, ctx, W, ld)
    part = pkg.DeviceBuffer(ctx, hostbuf=np.full(s * (s + 1) // 2 * grid, np.nan))
    pkg._lib.check(lib.cgamd_block_gram_weighted(ctx.handle, code, size, ld, s, ew.ptr, em.ptr, part.ptr))
    ctx.synchronize()
    _same(part.get().reshape(-1, grid), BP.gram_weighted_partials(W, m), "weighted Gram partials " + what)
    ew.check("w " + what)
    em.check("m " + what)
    bufs = [ew, em]
    for form in ("z", "m"):
        for init in (0, 1):
            want_q, want_p = BP.update_qp_z(W, P, Z if form == "z" else None, tz, tauz, init=bool(init), m=m)
            eq, ep = Embedded(pkg, ctx, W, ld), Embedded(pkg, ctx, P, ld, blank=bool(init))       # (init: nothing of P may be read)
            ez = Embedded(pkg, ctx, Z, ld)
            pkg._lib.check(lib.cgamd_block_update_qp_z(ctx.handle, code, size, ld, s, eq.ptr, ep.ptr, ez.ptr if form == "z" else None,
                                                       em.ptr if form == "m" else None, coef["ti"].ptr, coef["tau"].ptr, init))
            ctx.synchronize()
            eq.check(f"q, {form}-form, init {init} " + what, want_q)
            ep.check(f"p, {form}-form, init {init} " + what, want_p)
            ez.check(f"z behind the update, {form}-form " + what)
            em.check(f"m behind the update, {form}-form " + what)
            bufs += [eq, ep, ez]
    for e in bufs:
        e.buf.release()
    part.release()
    for k, v in (("ti", ti), ("tau", tau)):
        assert coef[k].get().tobytes() == v.tobytes(), "the factors are only read"
        coef[k].release()


def test_entries_refuse_what_they_do_not_serve(env):
    pkg, ctx, lib = env
    E = pkg._lib.ERR_INVALID
    buf = pkg.DeviceBuffer(ctx, hostbuf=np.zeros(64))
    p = buf.ptr
    for dtype, size, ld, s in ((2, 4, 4, 2), (3, 4, 4, 2), (1, 0, 4, 2), (1, 5, 4, 2), (1, 4, 4, 1), (1, 4, 4, 17)):
        assert lib.cgamd_block_gram_weighted(ctx.handle, dtype, size, ld, s, p, p, p) == E
        assert lib.cgamd_block_update_qp_z(ctx.handle, dtype, size, ld, s, p, p, p, None, p, p, 0) == E
    assert lib.cgamd_block_gram_weighted(ctx.handle, 1, 4, 4, 2, p, None, p) == E
    assert lib.cgamd_block_update_qp_z(ctx.handle, 1, 4, 4, 2, p, p, p, p, p, p, 0) == E        # both z and m
    assert lib.cgamd_block_update_qp_z(ctx.handle, 1, 4, 4, 2, p, p, None, None, p, p, 0) == E  # neither
    assert b"exactly one" in lib.cgamd_last_error()
    buf.release()


def _entries(Cm, s):
    return np.array([Cm[i, j] for i, j in B.pairs(s)])


@pytest.mark.parametrize("s", BLOCKS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_small_steps_bit_for_bit(env, dtype, s):
    pkg, ctx, _ = env
    dtype = np.dtype(dtype)
    eps = B.EPS[dtype]
    A = C.system("33x29", dtype)
    n = A.shape[0]
    b = C.rhs("33x29", s, dtype)
    m = C.jacobi("33x29", dtype)
    sv = pkg.Solver(ctx, n, A.nnz, A.data.astype(dtype), A.indptr, A.indices, s)
    try:
        sv.set_preconditioner(m)
        sv.set_block_pcg(True)
        sv.set_rhs(np.ascontiguousarray(b.T))
        # R0 = b exactly (x0 = 0): both summed matrices from the restated partials of the handle's padded rows and their restated sum
        ld = sv.ld
        bp, mp = np.zeros((s, ld), dtype), np.zeros(ld, dtype)
        bp[:, :n], mp[:n] = b.T, m
        D, CZ = sv.block_state("C"), sv.block_state("CZ")
        _same(_entries(D, s), B.sum_partials(B.gram_partials(bp, bp)), f"{dtype.name} s {s}: R0^T R0 as summed")
        _same(_entries(CZ, s), B.sum_partials(BP.gram_weighted_partials(bp, mp)), f"{dtype.name} s {s}: R0^T Z0 as summed")
        assert np.array_equal(D, D.T) and np.array_equal(CZ, CZ.T)
        st = BP.small_w(_entries(D, s), _entries(CZ, s), None, s, eps)
        assert st["status"] == 0
        for name in ("tau", "tau_inv", "xi"):
            _same(sv.block_state(name), st[name], f"{dtype.name} s {s} set_rhs {name}")
        _same(sv.history()[0], st["delta"].astype(dtype), f"{dtype.name} s {s} delta_0")
        xi, ratio = st["xi"].tolist(), st["ratio"]
        sv.iterate(1)
        s1 = B.small1(_entries(sv.block_state("G"), s), xi, s, eps)
        assert s1["status"] == 0
        for name in ("alpha", "M"):
            _same(sv.block_state(name), s1[name], f"{dtype.name} s {s} iteration 1 {name}")
        s2 = BP.small_w(_entries(sv.block_state("C"), s), _entries(sv.block_state("CZ"), s), xi, s, eps)
        assert s2["status"] == 0
        for name in ("tau", "tau_inv", "xi"):
            _same(sv.block_state(name), s2[name], f"{dtype.name} s {s} iteration 1 {name}")
        _same(sv.history()[1], s2["delta"].astype(dtype), f"{dtype.name} s {s} delta_1")
        status = sv.block_status()
        assert (status["on"], status["preconditioned"], status["status"], status["s"]) == (True, True, 0, s)
        assert status["min_pivot_ratio"] == min(ratio, s1["ratio"], s2["ratio"])
    finally:
        sv.close()
