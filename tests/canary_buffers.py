"""Device arrays inside canary buffers, for the tests that compare whole buffers bit for bit (the idea of test_gpu_mixed_kernels.py,
for any value type and for ints): what a kernel must write is compared in all its bits, and so is everything it must leave alone."""
import numpy as np

import spmv_ref as R

PRE, POST = 64, 80


class Embedded:
    """nrhs columns of w <= ld values at a leading dimension of ld values, `off` bytes behind a 16-byte boundary, inside a device
    buffer of 0xFF bytes that holds nrhs * ld values and PRE / POST bytes around them.  blank: the array starts as canary throughout"""
    def __init__(self, pkg, ctx, rows, ld, off=0, blank=False):
        rows = np.ascontiguousarray(rows)
        assert rows.ndim == 2 and rows.shape[1] <= ld
        self.dtype, self.ld, self.nrhs, self.start = rows.dtype, ld, rows.shape[0], PRE + off
        self.before = np.full(PRE + off + self.nrhs * ld * rows.itemsize + POST, 0xFF, np.uint8)
        if not blank:
            self.place(self.before, rows)
        self.buf = pkg.DeviceBuffer(ctx, hostbuf=self.before)
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + self.start

    def place(self, image, rows):
        item = self.dtype.itemsize
        for r in range(self.nrhs):
            at = self.start + r * self.ld * item
            image[at:at + rows.shape[1] * item] = np.ascontiguousarray(rows[r]).view(np.uint8)

    def check(self, what, rows=None):
        """the buffer holds the image of before with `rows` written over the first lanes of every column"""
        want = self.before.copy()
        got = self.buf.get()
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=self.dtype)
            self.place(want, rows)
            if self.dtype.kind in "fc":         # a NaN of the restatement is met by any NaN
                Rt = R.real_type(self.dtype)
                lanes = slice(self.start, self.start + self.nrhs * self.ld * self.dtype.itemsize)
                w, g = want[lanes].view(Rt).reshape(self.nrhs, -1), got[lanes].view(Rt).reshape(self.nrhs, -1)
                k = rows.view(Rt).shape[1]
                both = np.isnan(w[:, :k]) & np.isnan(g[:, :k])
                g[:, :k][both] = w[:, :k][both]
        if got.tobytes() != want.tobytes():
            item = self.dtype.itemsize
            at = int(np.flatnonzero(got != want)[0])
            lane = (at - self.start) // item            # (negative: in the bytes before the array)
            a = self.start + lane * item
            raise AssertionError(f"{what}: {int(np.count_nonzero(got != want))} bytes differ, the first in lane {lane % self.ld} of column "
                                 f"{lane // self.ld} (ld {self.ld}): got {got[a:a + item].view(self.dtype)}, want {want[a:a + item].view(self.dtype)}")
