"""The four streaming kernels of the mixed-precision solve (csrc/mixed.hip) through their stateless entries, element by element and
BIT FOR BIT against the host restatement (tests/mixed_kernel_ref.py), in both forms (16-byte and scalar) and both value types.

Every array of a call lies inside a larger device buffer filled with 0xFF bytes -- a NaN in float and in double -- and the WHOLE buffer
is compared afterwards with what the contract says it holds: the results where the kernel writes, the bytes of before everywhere
else (the hi side's padding rows, masked columns, the bytes before and after the arrays, and every array that is only read).  The norm
is compared on the per-work-group partials and on the result, and also with math.fsum of the same squares within the bound derived in
mixed_kernel_ref.  Which form a call takes is the argument rule of mixed.hip, restated there and asserted here on the pointers and
leading dimensions of the call; the order of the norm's sum differs between the forms (tests/test_mixed_kernel_ref.py), so its bits
also show which form ran."""
import numpy as np
import pytest

import mixed_kernel_ref as K

pytestmark = pytest.mark.gpu

CASES = K.cases()
PRE, POST = 64, 80


class Embedded:
    """nrhs columns of w <= ld float64 / float32 lanes at a leading dimension of ld lanes, `off` bytes behind a 16-byte boundary, inside
    a device buffer of 0xFF bytes that holds nrhs * ld lanes and PRE / POST bytes around them.  rows: the (nrhs, w) lanes to start
    from, or (blank) only their shape and type -- the array then starts as canary throughout, so that whatever the contract says is
    written has to be written"""
    def __init__(self, pkg, ctx, rows, ld, off=0, blank=False):
        rows = np.ascontiguousarray(rows)
        assert rows.shape[1] <= ld
        self.dtype, self.ld, self.nrhs, self.start = rows.dtype, ld, rows.shape[0], PRE + off
        self.before = np.full(PRE + off + self.nrhs * ld * rows.itemsize + POST, 0xFF, np.uint8)
        if not blank:
            self.place(self.before, rows)
        self.buf = pkg.DeviceBuffer(ctx, hostbuf=self.before)
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + self.start

    def place(self, image, rows, only=None):
        item = self.dtype.itemsize
        for r in range(self.nrhs):
            if only is None or only[r]:
                at = self.start + r * self.ld * item
                image[at:at + rows.shape[1] * item] = np.ascontiguousarray(rows[r]).view(np.uint8)

    def expect(self, rows=None, only=None):
        """the image of before with `rows` written over the columns `only` selects (all by default)"""
        image = self.before.copy()
        if rows is not None:
            self.place(image, np.ascontiguousarray(rows, dtype=self.dtype), only)
        return image

    def values(self, w):
        """the first w lanes of column 0 as the device holds them"""
        return self.buf.get()[self.start:self.start + w * self.dtype.itemsize].view(self.dtype)

    def check(self, want, what):
        got = self.buf.get()
        if got.tobytes() != want.tobytes():
            item = self.dtype.itemsize
            at = int(np.flatnonzero(got != want)[0])
            lane = (at - self.start) // item            # (negative: in the bytes before the array)
            a = self.start + lane * item
            raise AssertionError(f"{what}: {int(np.count_nonzero(got != want))} bytes differ, the first in lane {lane % self.ld} of column "
                                 f"{lane // self.ld} (ld {self.ld}): got {got[a:a + item].view(self.dtype)}, want {want[a:a + item].view(self.dtype)}")


_INPUTS = {}


def inputs(c):
    if c["id"] not in _INPUTS:
        _INPUTS[c["id"]] = K.inputs(c)
    return _INPUTS[c["id"]]


@pytest.fixture(scope="module")
def env(pkg, gpu):
    return pkg, gpu[0], pkg._lib.load()


def call(pkg, rc):
    pkg._lib.check(rc)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_accumulate(env, c):
    pkg, ctx, lib = env
    inp, R = inputs(c), c["R"]
    scale = pkg.DeviceBuffer(ctx, hostbuf=inp["scale"])
    for mask in c["masks"]:
        hi = Embedded(pkg, ctx, inp["x_hi"], c["ld_hi"] * R, c["off_hi"])
        lo = Embedded(pkg, ctx, inp["x_lo"], c["ld_lo"] * R, c["off_lo"])
        assert K.takes_vec(hi.ptr, c["ld_hi"] * 8 * R, lo.ptr, c["ld_lo"] * 4 * R, c["nrhs"]) == c["vec"]
        dmask = pkg.DeviceBuffer(ctx, hostbuf=np.asarray(mask, dtype=np.intc))
        call(pkg, lib.cgamd_mixed_accumulate(ctx.handle, K.CODE[c["dt"]], c["size"], pkg._lib.ptr(hi.ptr), c["ld_hi"], pkg._lib.ptr(lo.ptr), c["ld_lo"],
                                             pkg._lib.ptr(scale), pkg._lib.ptr(dmask), c["nrhs"]))
        want = K.accumulate(inp["x_hi"], inp["x_lo"], inp["scale"], mask)
        hi.check(hi.expect(want, only=mask), f"accumulate mask {mask}: x_hi")
        lo.check(lo.expect(), f"accumulate mask {mask}: x_lo is only read")
        # (a masked column is the bytes of before; that an open one is not is what makes the mask's effect visible)
        for r in range(c["nrhs"]):
            assert (want[r].tobytes() == inp["x_hi"][r].tobytes()) == (not mask[r])


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_round_down(env, c):
    pkg, ctx, lib = env
    inp, R = inputs(c), c["R"]
    hi = Embedded(pkg, ctx, inp["r_hi"], c["ld_hi"] * R, c["off_hi"])
    lo = Embedded(pkg, ctx, np.empty((c["nrhs"], c["ld_lo"] * R), np.float32), c["ld_lo"] * R, c["off_lo"], blank=True)
    assert K.takes_vec(hi.ptr, c["ld_hi"] * 8 * R, lo.ptr, c["ld_lo"] * 4 * R, c["nrhs"]) == c["vec"]
    inv = pkg.DeviceBuffer(ctx, hostbuf=inp["inv_scale"])
    call(pkg, lib.cgamd_mixed_round_down(ctx.handle, K.CODE[c["dt"]], c["size"], pkg._lib.ptr(hi.ptr), c["ld_hi"], pkg._lib.ptr(lo.ptr), c["ld_lo"],
                                         pkg._lib.ptr(inv), c["nrhs"]))
    want = K.round_down(inp["r_hi"], inp["inv_scale"], c["ld_lo"] * R)
    assert want.shape[1] == c["ld_lo"] * R and not want[:, c["m"]:].view(np.uint32).any()
    lo.check(lo.expect(want), "round_down: r_lo")
    hi.check(hi.expect(), "round_down: r_hi is only read")


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_round_values(env, c):
    pkg, ctx, lib = env
    vals = inputs(c)["values"][None, :]
    hi = Embedded(pkg, ctx, vals, c["m"], c["off_hi"])
    lo = Embedded(pkg, ctx, np.empty((1, c["m"]), np.float32), c["m"], c["off_lo"], blank=True)
    assert K.round_values_takes_vec(hi.ptr, lo.ptr) == (c["off_hi"] % 16 == 0 and c["off_lo"] % 16 == 0)
    call(pkg, lib.cgamd_mixed_round_values(ctx.handle, K.CODE[c["dt"]], c["size"], pkg._lib.ptr(hi.ptr), pkg._lib.ptr(lo.ptr)))
    lo.check(lo.expect(K.round_values(vals)), "round_values: lo")
    hi.check(hi.expect(), "round_values: hi is only read")


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_norm2(env, c):
    pkg, ctx, lib = env
    inp, R = inputs(c), c["R"]
    G = lib.cgamd_mixed_norm2_grid(K.CODE[c["dt"]], c["size"])
    assert G == K.grid(c["m"])
    for name in ("x_hi", "v"):
        v = Embedded(pkg, ctx, inp[name], c["ld_hi"] * R, c["off_hi"])
        assert K.takes_vec(v.ptr, c["ld_hi"] * 8 * R, None, 0, c["nrhs"]) == c["vec_norm"]
        partials = Embedded(pkg, ctx, np.empty((1, c["nrhs"] * G)), c["nrhs"] * G, blank=True)
        out = Embedded(pkg, ctx, np.empty((1, c["nrhs"])), c["nrhs"], blank=True)
        call(pkg, lib.cgamd_mixed_norm2(ctx.handle, K.CODE[c["dt"]], c["size"], pkg._lib.ptr(v.ptr), c["ld_hi"], c["nrhs"], pkg._lib.ptr(partials.ptr),
                                        pkg._lib.ptr(out.ptr)))
        want_p, want = K.norm2(inp[name], c["vec_norm"])
        partials.check(partials.expect(want_p.reshape(1, -1)), f"norm2({name}): partials")
        out.check(out.expect(want.reshape(1, -1)), f"norm2({name}): result")
        v.check(v.expect(), f"norm2({name}): v is only read")
        got = out.values(c["nrhs"])
        exact = K.norm2_exact(inp[name])
        bound = K.norm2_bound(c["m"], exact)
        print(f"  {c['id']} {name}: |device - fsum| / bound = {np.max(np.abs(got - exact) / bound):.3f}")
        assert np.all(np.abs(got - exact) <= bound), (got, exact, bound)


def test_nothing_is_launched_for_size_zero(env):
    pkg, ctx, lib = env
    c = CASES[3]
    inp = inputs(c)
    hi = Embedded(pkg, ctx, inp["x_hi"], c["ld_hi"])
    lo = Embedded(pkg, ctx, inp["x_lo"], c["ld_lo"])
    one = pkg.DeviceBuffer(ctx, hostbuf=np.ones(1))
    mask = pkg.DeviceBuffer(ctx, hostbuf=np.ones(1, np.intc))
    P = pkg._lib.ptr
    call(pkg, lib.cgamd_mixed_accumulate(ctx.handle, 1, 0, P(hi.ptr), 4, P(lo.ptr), 4, P(one), P(mask), 1))
    call(pkg, lib.cgamd_mixed_round_down(ctx.handle, 1, 0, P(hi.ptr), 4, P(lo.ptr), 4, P(one), 1))
    call(pkg, lib.cgamd_mixed_round_values(ctx.handle, 1, 0, P(hi.ptr), P(lo.ptr)))
    call(pkg, lib.cgamd_mixed_norm2(ctx.handle, 1, 0, P(hi.ptr), 4, 1, P(one), P(one)))
    hi.check(hi.expect(), "size 0: hi")
    lo.check(lo.expect(), "size 0: lo")
    assert one.get().tolist() == [1.0]
