"""The vector kernel of multi-shift CG (csrc/shifts.hip) alone, through cgamd_shift_update on random data, BIT FOR BIT against the
type-true restatement shift_ref.update_bits: xs_j = vadd(xs_j, vmul(al_j, ds_j)), ds_j = vadd(vmul(ze_j, r), vmul(be_j, ds_j)), one
rounding per operation, complex products by components.

Shapes: size in {1, 3, 255, 256, 257, 1027} (below a pack, one work-group exactly, one value more, five work-groups with a ragged one
and a scalar tail), nRHS in {1, 3}, nShifts in {1, 2, 5, 16} (below, at and across the group of four shifts whose loads one thread
keeps in flight, and the most the entry takes).  Every array lies in a canary buffer (tests/canary_buffers.py) with ld > size, and the
whole buffer is compared: the padding rows between size and ld and the bytes before and behind keep theirs, r is only read.  The
forms: 16-byte packs (aligned pointers, ld whole packs); the value-by-value path taken for a pointer one element off a 16-byte
boundary and for an ld that is not whole packs; the non-temporal instantiation (vec_nt = 1).  One zeta of every case with more than
one coefficient is 0 (the r term switched off: what an underflowed zeta does); its d_j still takes beta_j d_j."""
import numpy as np
import pytest

import shift_ref as M
from canary_buffers import Embedded
from conftest import ALL_DTYPES, rand_vec

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 255, 256, 257, 1027)
NRHS = (1, 3)
SHIFTS = (1, 2, 5, 16)


@pytest.fixture(scope="module")
def env(pkg, gpu):
    return pkg, gpu[0], pkg._lib.load()


def _case(dtype, size, nrhs, S, seed):
    rng = np.random.default_rng(seed)
    r = rand_vec(rng, nrhs * size, dtype).reshape(nrhs, size)
    xs = rand_vec(rng, S * nrhs * size, dtype).reshape(S, nrhs, size)
    ds = rand_vec(rng, S * nrhs * size, dtype).reshape(S, nrhs, size)
    al, be, ze = (rand_vec(rng, S * nrhs, dtype).reshape(S, nrhs) for _ in range(3))
    if S > 1 or nrhs > 1:       # (the one case with a single coefficient keeps it)
        ze[S // 2, 0] = 0
    return r, xs, ds, al, be, ze


def _run(env, dtype, size, nrhs, S, ld, off, what):
    pkg, ctx, lib = env
    code = pkg._lib.DTYPE_CODE[np.dtype(dtype)]
    r, xs, ds, al, be, ze = _case(dtype, size, nrhs, S, 7 * size + 3 * nrhs + S)
    want_x, want_d = M.update_bits(r, xs, ds, al, be, ze)
    er = Embedded(pkg, ctx, r, ld, off)
    ex = Embedded(pkg, ctx, xs.reshape(S * nrhs, size), ld, off)        # (j, r) at (j * nRHS + r) * ld
    ed = Embedded(pkg, ctx, ds.reshape(S * nrhs, size), ld, off)
    coef = [pkg.DeviceBuffer(ctx, hostbuf=np.ascontiguousarray(c)) for c in (al, be, ze)]
    pkg._lib.check(lib.cgamd_shift_update(ctx.handle, code, size, ld, nrhs, S, er.ptr, ex.ptr, ed.ptr, coef[0].ptr, coef[1].ptr, coef[2].ptr))
    ctx.synchronize()
    er.check("r " + what)                                               # only read
    ex.check("xs " + what, want_x.reshape(S * nrhs, size))
    ed.check("ds " + what, want_d.reshape(S * nrhs, size))
    for c, h in zip(coef, (al, be, ze)):
        assert c.get().tobytes() == h.tobytes(), "coefficients " + what
        c.release()
    for e in (er, ex, ed):
        e.buf.release()


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_shift_update_bit_for_bit(env, dtype):
    dtype = np.dtype(dtype)
    E = 16 // dtype.itemsize
    for size in SIZES:
        packs = (size + E - 1) // E * E + E             # whole packs, and at least one pack of padding
        for nrhs in NRHS:
            for S in SHIFTS:
                what = f"{dtype.name} size {size} nrhs {nrhs} shifts {S}"
                _run(env, dtype, size, nrhs, S, packs, 0, what + " packs")
                if S == 5:      # a pointer offset by one element: value by value
                    _run(env, dtype, size, nrhs, S, packs, dtype.itemsize, what + " offset pointer")
                if S == 2:      # an ld that is not whole packs (every type but complex128, where a value is a pack)
                    _run(env, dtype, size, nrhs, S, size + 1, 0, what + " ld = size + 1")


@pytest.fixture
def vec_nt(pkg):
    lib = pkg._lib.load()
    pkg._lib.check(lib.cgamd_tune(b"vec_nt", 1))
    yield
    pkg._lib.check(lib.cgamd_tune(b"vec_nt", -1))


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_non_temporal_form_same_bits(env, vec_nt, dtype):
    dtype = np.dtype(dtype)
    E = 16 // dtype.itemsize
    for size in (257, 1027):
        for S in (2, 5):
            _run(env, dtype, size, 3, S, (size + E - 1) // E * E + E, 0, f"{dtype.name} size {size} shifts {S} non-temporal")


def test_refusals(env):
    pkg, ctx, lib = env
    E = pkg._lib.ERR_INVALID
    buf = pkg.DeviceBuffer(ctx, hostbuf=np.zeros(64, np.float64))
    p = buf.ptr
    assert lib.cgamd_shift_update(ctx.handle, 1, 8, 8, 1, 17, p, p, p, p, p, p) == E        # nShifts
    assert lib.cgamd_shift_update(ctx.handle, 1, 8, 4, 1, 1, p, p, p, p, p, p) == E         # ld < size
    assert lib.cgamd_shift_update(ctx.handle, 9, 8, 8, 1, 1, p, p, p, p, p, p) == E         # dtype
    assert lib.cgamd_shift_update(ctx.handle, 1, 8, 8, 0, 1, p, p, p, p, p, p) == E         # nRHS
    assert lib.cgamd_shift_update(ctx.handle, 1, 8, 8, 1, 1, p, None, p, p, p, p) == E      # null
    assert lib.cgamd_shift_update(ctx.handle, 1, 8, 8, 1, 0, None, None, None, None, None, None) == 0       # no shifts: nothing to do
    assert not buf.get().any()
