"""The two basis kernels of the solution projection (csrc/projection.hip) through their context-level entries, on random data, BIT FOR
BIT against the type-true restatement (tests/projection_ref.py on the helpers of cg_step_ref.py): the dots in the order
include/cgamd.h states, the combination one multiplication and one addition per slot per element.  Every output lies in a buffer
of marker values, and the whole buffer is compared: a masked slot's entry, the padding rows and the columns' tails keep theirs."""
import numpy as np
import pytest

import cg_step_ref as S
import projection_ref as PR
from conftest import ALL_DTYPES, rand_vec

pytestmark = pytest.mark.gpu

MARK = 12345.0
SLOTS = (1, 7, 8, 9, 32)        # across the 8-slot register group
NRHS = (1, 3)


def _sizes(lib, code, dtype):
    E = 16 // np.dtype(dtype).itemsize
    big = 2 * 256 * E + 5 * E + (1 if E > 1 else 0)     # three work-groups of the dots kernel, the last one ragged, a scalar tail
    assert lib.cgamd_projection_dots_grid(code, big) == 3
    return (1, 37, 957, big)


@pytest.fixture(scope="module")
def env(pkg, gpu):
    return pkg, gpu[0], pkg._lib.load()


def _data(dtype, size, ld, slots, nrhs, seed):
    rng = np.random.default_rng(seed)
    W = np.full((slots, nrhs, ld), MARK, dtype)
    v = np.full((nrhs, ld), MARK, dtype)
    W[:, :, :size] = rand_vec(rng, slots * nrhs * size, dtype).reshape(slots, nrhs, size)
    v[:, :size] = rand_vec(rng, nrhs * size, dtype).reshape(nrhs, size)
    c = rand_vec(rng, slots * nrhs, dtype).reshape(slots, nrhs)
    return W, v, c


def _live(slots, mask):
    return [j for j in range(slots) if mask >> j & 1]


def _same(got, want, what):
    assert got.tobytes() == want.tobytes(), f"{what}: {int(np.count_nonzero(got != want))} values differ"


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("which", range(4), ids=("one", "n37", "n957", "three_groups"))
def test_dots_and_combine(env, dtype, which):
    pkg, ctx, lib = env
    dtype = np.dtype(dtype)
    code = pkg._lib.DTYPE_CODE[dtype]
    size = _sizes(lib, code, dtype)[which]
    ld = PR.ld_of(size, dtype)
    E = 16 // dtype.itemsize
    G = lib.cgamd_projection_dots_grid(code, size)
    assert G == PR.dots_grid(dtype, size)
    ops = S.Ops(dtype)
    for slots in SLOTS:
        for nrhs in NRHS:
            masks = [(1 << slots) - 1]
            if slots == 9 and nrhs == 3:
                masks.append(((1 << slots) - 1) & ~(1 << 2))        # one case has a masked slot
            for mask in masks:
                what = f"{dtype.name} size {size} slots {slots} nrhs {nrhs} mask {mask:#x}"
                W, v, c = _data(dtype, size, ld, slots, nrhs, 1000 * which + 10 * slots + nrhs)
                dW, dv, dc = (pkg.DeviceBuffer(ctx, hostbuf=a) for a in (W, v, c))
                # ---- dots
                want = np.full((slots, nrhs), MARK, dtype)
                for j in _live(slots, mask):
                    p = S.group_partials(ops.terms(W[j, :, :size], v[:, :size]), G, E, True)
                    want[j] = S.from_acc(S.prologue_sum(p, 1024, 0), dtype)
                outs = []
                for _ in range(2):                                  # the same bits from a second call
                    dout = pkg.DeviceBuffer(ctx, hostbuf=np.full((slots, nrhs), MARK, dtype))
                    pkg._lib.check(lib.cgamd_projection_dots(ctx.handle, code, size, ld, slots, mask, dW.ptr, nrhs * ld, dv.ptr, nrhs, dout.ptr))
                    outs.append(dout.get().reshape(slots, nrhs))
                _same(outs[0], want, "dots " + what)
                _same(outs[1], outs[0], "dots, second call " + what)
                # ---- combine: sign +1 / -1, with and without v
                for sign in (1, -1):
                    for with_v in (True, False):
                        y = np.zeros((nrhs, size), dtype) if not with_v else v[:, :size].copy()
                        for j in _live(slots, mask):
                            y = ops.axpy(y, c[j], W[j, :, :size]) if sign > 0 else ops.axmy(y, c[j], W[j, :, :size])
                        want_y = np.full((nrhs, ld), MARK, dtype)
                        want_y[:, :size] = y
                        dy = pkg.DeviceBuffer(ctx, hostbuf=np.full((nrhs, ld), MARK, dtype))
                        pkg._lib.check(lib.cgamd_projection_combine(ctx.handle, code, size, ld, slots, mask, dW.ptr, nrhs * ld,
                                                                    dv.ptr if with_v else None, dc.ptr, sign, dy.ptr, nrhs))
                        _same(dy.get().reshape(nrhs, ld), want_y, f"combine sign {sign} v {with_v} " + what)
                # the inputs are only read
                _same(dW.get().reshape(W.shape), W, "W " + what)
                _same(dv.get().reshape(v.shape), v, "v " + what)


def test_refusals(env):
    pkg, ctx, lib = env
    E = pkg._lib.ERR_INVALID
    buf = pkg.DeviceBuffer(ctx, hostbuf=np.zeros(64, np.float64))
    assert lib.cgamd_projection_dots(ctx.handle, 1, 8, 8, 33, 1, buf.ptr, 8, buf.ptr, 1, buf.ptr) == E      # slots
    assert lib.cgamd_projection_dots(ctx.handle, 1, 8, 4, 1, 1, buf.ptr, 8, buf.ptr, 1, buf.ptr) == E       # ld < size
    assert lib.cgamd_projection_combine(ctx.handle, 1, 8, 8, 1, 1, buf.ptr, 8, buf.ptr, buf.ptr, 2, buf.ptr, 1) == E    # sign
    assert lib.cgamd_projection_combine(ctx.handle, 9, 8, 8, 1, 1, buf.ptr, 8, buf.ptr, buf.ptr, 1, buf.ptr, 1) == E    # dtype
