"""Host-side mirror of the reference's Python solver module (reference cl.py:1-360),
driving hand-written HIP kernels through the C ABI instead of pyopencl.

Same names, argument meaning and return values as the reference for the CG path:

    initialize_cl_environment()                 reference cl.py:16-19
    initialize_cl_environment_with_device(dev)  reference cl.py:21-24
    get_gpu_devices()                           reference cl.py:26-31
    load_and_build_kernels(ctx, n_rhs)          reference cl.py:33-42
    CG(ctx, queue, kernels, size, non_zeros, a_values, b_values, a_pointers,
       a_cols, x, n_rhs, n_iterations, device=None)            reference cl.py:44-200
    conjugate_gradient_multi_gpu(<same>, device)                reference cl.py:203-360

Differences a caller can observe (all documented in INTEGRATION.md):
  * nothing is JIT-compiled: the kernels are precompiled for gfx950, so
    load_and_build_kernels is cheap and independent of n_rhs;
  * the value type follows a_values.dtype (complex64 at the reference's call sites,
    p_h-PY_C-CL.py:1926-1933; float32/float64/complex128 also work) instead of the
    module-level IS_COMPLEX switch;
  * errors raise CgAmdError instead of being printed and ignored.
There is no CPU fallback: without the HIP library or a GPU these functions raise.
"""
import ctypes
import threading

import numpy as np

from . import _lib
from ._lib import CgAmdError, check, ptr  # noqa: F401

# module constants of the reference (cl.py:5-7); values are those of the CDNA4 build
IS_COMPLEX = True
WAVE_SIZE = 64
LOCAL_SIZE = 4 * WAVE_SIZE


class Device:
    """A HIP device (stands for a pyopencl.Device)."""

    def __init__(self, index):
        self.index = int(index)
        buf = ctypes.create_string_buffer(256)
        check(_lib.load().cgamd_device_name(self.index, buf, 256))
        self.name = buf.value.decode()

    def __repr__(self):
        return f"<Device {self.index}: {self.name}>"


class Context:
    """Owns a cgamd_ctx (device + HIP stream + workspace). Stands for pyopencl.Context."""

    def __init__(self, device=0):
        self.device = device.index if isinstance(device, Device) else int(device)
        h = ctypes.c_void_p()
        check(_lib.load().cgamd_ctx_create(self.device, ctypes.byref(h)))
        self.handle = h
        self._lib = _lib.load()

    def set_stream(self, stream):
        """Run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""
        check(self._lib.cgamd_ctx_set_stream(self.handle, ctypes.c_void_p(int(stream))))

    @property
    def stream(self):
        return self._lib.cgamd_ctx_stream(self.handle) or 0

    def synchronize(self):
        check(self._lib.cgamd_ctx_synchronize(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cgamd_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CommandQueue:
    """Stands for pyopencl.CommandQueue: the in-order HIP stream of a Context."""

    def __init__(self, ctx):
        self.ctx = ctx

    def flush(self):
        pass

    def finish(self):
        self.ctx.synchronize()


class DeviceBuffer:
    """Device memory owned through the C ABI (stands for pyopencl.Buffer)."""

    def __init__(self, ctx, nbytes=None, hostbuf=None, dtype=None):
        self.ctx = ctx
        self._lib = _lib.load()
        if hostbuf is not None:
            hostbuf = np.ascontiguousarray(hostbuf)
            nbytes = hostbuf.nbytes
            dtype = hostbuf.dtype
        self.nbytes = int(nbytes)
        self.dtype = np.dtype(dtype) if dtype is not None else np.dtype(np.uint8)
        p = ctypes.c_void_p()
        check(self._lib.cgamd_malloc(ctx.handle, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value
        if hostbuf is not None and self.nbytes:
            check(self._lib.cgamd_memcpy_h2d(ctx.handle, p, ptr(hostbuf), self.nbytes))

    def get(self, out=None):
        if out is None:
            out = np.empty(self.nbytes // self.dtype.itemsize, dtype=self.dtype)
        check(self._lib.cgamd_memcpy_d2h(self.ctx.handle, ptr(out), ctypes.c_void_p(self.ptr), self.nbytes))
        return out

    def release(self):
        if getattr(self, "ptr", None) and getattr(self.ctx, "handle", None):
            self._lib.cgamd_free(self.ctx.handle, ctypes.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def transpose(ctx, dtype, rows, cols, src, dst):
    """dst[c*rows + r] = src[r*cols + c] on the device: RHS-major [n_rhs][size] <-> row-major [size][n_rhs]"""
    check(_lib.load().cgamd_transpose(ctx.handle, _lib.DTYPE_CODE[np.dtype(dtype)], int(rows), int(cols), ptr(src), ptr(dst)))


def get_gpu_devices():
    """reference cl.py:26-31 -- list of GPU devices."""
    n = _lib.load().cgamd_device_count()
    if n < 0:
        raise CgAmdError(-n, _lib.load().cgamd_last_error().decode())
    return [Device(i) for i in range(n)]


def initialize_cl_environment():
    """reference cl.py:16-19 -- (ctx, queue) on the default device."""
    ctx = Context(0)
    return ctx, CommandQueue(ctx)


def initialize_cl_environment_with_device(device):
    """reference cl.py:21-24."""
    ctx = Context(device)
    return ctx, CommandQueue(ctx)


# ---- the five kernels, as callables on DeviceBuffers -------------------------------------------
_TORCH_NAMES = {"torch.float32": np.float32, "torch.float64": np.float64,
                "torch.complex64": np.complex64, "torch.complex128": np.complex128}


def _code(buf):
    dt = buf.dtype
    if str(dt) in _TORCH_NAMES:          # torch tensors are accepted wherever a DeviceBuffer is
        dt = _TORCH_NAMES[str(dt)]
    return _lib.DTYPE_CODE[np.dtype(dt)]


class _Kernels(dict):
    """{'axpy','aypx','spmv','sub','vdot'} -> callables (reference cl.py:36-42).

    spmv(queue, size, a_values, a_pointers, a_cols, x, y, n_rhs=None)
    vdot(queue, a, b, result, size, n_rhs=None)        result: DeviceBuffer of n_rhs values
    axpy(queue, x, y, a, a_sign, size, n_rhs=None)     a: DeviceBuffer of n_rhs values
    aypx(queue, x, y, a, size, n_rhs=None)
    sub(queue, a, b, result, size, n_rhs=None)
    """

    def __init__(self, ctx, n_rhs):
        lib = _lib.load()
        self.ctx, self.n_rhs = ctx, int(n_rhs)
        h = ctx.handle

        def spmv(queue, size, a_values, a_pointers, a_cols, x, y, n_rhs=None):
            nnz = (a_cols.numel() if hasattr(a_cols, "numel") else a_cols.nbytes // 4)
            check(lib.cgamd_spmv(h, _code(a_values), int(size), nnz, ptr(a_values), ptr(a_pointers), ptr(a_cols),
                                 ptr(x), ptr(y), n_rhs or self.n_rhs))

        def vdot(queue, a, b, result, size, n_rhs=None):
            check(lib.cgamd_vdot(h, _code(a), int(size), ptr(a), ptr(b), ptr(result), n_rhs or self.n_rhs))

        def axpy(queue, x, y, a, a_sign, size, n_rhs=None):
            check(lib.cgamd_axpy(h, _code(y), int(size), ptr(x), ptr(y), ptr(a), int(a_sign), n_rhs or self.n_rhs))

        def aypx(queue, x, y, a, size, n_rhs=None):
            check(lib.cgamd_aypx(h, _code(y), int(size), ptr(x), ptr(y), ptr(a), n_rhs or self.n_rhs))

        def sub(queue, a, b, result, size, n_rhs=None):
            check(lib.cgamd_sub(h, _code(a), int(size), ptr(a), ptr(b), ptr(result), n_rhs or self.n_rhs))

        super().__init__(axpy=axpy, aypx=aypx, spmv=spmv, sub=sub, vdot=vdot)


def load_and_build_kernels(ctx, n_rhs):
    """reference cl.py:33-42.  Nothing is compiled here: the gfx950 code objects ship in libcgamd.so."""
    return _Kernels(ctx, n_rhs)


# ---- persistent solver ------------------------------------------------------------------------
def _set_preconditioner_batched(self, m):
    """one M per system on a batched handle; the length of a host array is checked before the library is asked"""
    if m is None:
        check(self._lib.cgamd_solver_set_preconditioner_batched(self.handle, None, 0))
        return
    if isinstance(m, str) and m == "jacobi":
        check(self._lib.cgamd_solver_set_preconditioner_batched_jacobi(self.handle))
        return
    if isinstance(m, tuple) and len(m) == 2 and isinstance(m[0], str) and m[0] == "line":
        check(self._lib.cgamd_solver_set_preconditioner_batched_line(self.handle, int(m[1])))
        return
    if isinstance(m, tuple) and len(m) in (2, 3) and isinstance(m[0], str) and m[0] == "multigrid":
        dims = tuple(int(d) for d in m[1]) + (1,) * (3 - len(m[1]))
        opts = dict(m[2]) if len(m) == 3 else {}
        unknown = set(opts) - {"smooth_steps", "over_correction", "min_rows"}
        if len(dims) != 3 or unknown:
            raise ValueError('("multigrid", (nx, ny, nz)[, {"smooth_steps": 1, "over_correction": 1.6, "min_rows": 512}])')
        check(self._lib.cgamd_solver_set_preconditioner_batched_multigrid(self.handle, dims[0], dims[1], dims[2],
                                                                          int(opts.get("smooth_steps", 0)),
                                                                          float(opts.get("over_correction", 0.0)),
                                                                          int(opts.get("min_rows", 0))))
        return
    if isinstance(m, (list, tuple)) and len(m) == self.n_rhs and all(hasattr(a, "diagonal") and hasattr(a, "nnz") for a in m):
        if any(a.shape != (self.size, self.size) or a.nnz > self.size for a in m):
            raise ValueError('a list of matrices on a batched handle gives their diagonals: n_rhs matrices of size x size with '
                             'nnz <= size each; the lines of the systems\' own matrices are ("line", stride)')
        m = np.stack([np.asarray(a.diagonal()) for a in m])
    if isinstance(m, np.ndarray) or (isinstance(m, (list, tuple)) and not isinstance(m, str)):
        try:
            flat = np.asarray(m).reshape(-1)
        except (TypeError, ValueError):
            flat = None
        if flat is None or flat.dtype == object or flat.size != self.n_rhs * self.size:
            raise ValueError(f"a batched handle of {self.n_rhs} systems takes a preconditioner of {self.n_rhs} * {self.size} = "
                             f"{self.n_rhs * self.size} diagonal entries (system r at [r * size:(r + 1) * size]), or \"jacobi\", "
                             f'or ("line", stride)')
        m = np.ascontiguousarray(flat, dtype=self.dtype)
        check(self._lib.cgamd_solver_set_preconditioner_batched(self.handle, ptr(m), 0))
        return
    if isinstance(m, int) or hasattr(m, "data_ptr") or hasattr(m, "ptr"):      # a device buffer of n_rhs * size values
        check(self._lib.cgamd_solver_set_preconditioner_batched(self.handle, ptr(m), 1))
        return
    raise ValueError('a batched handle takes one preconditioner per system: None, "jacobi", ("line", stride), ("multigrid", dims), n_rhs * size '
                     'diagonal entries (host array or device buffer) or a list of n_rhs diagonal matrices; for the tridiagonal '
                     'part of every system use ("line", stride)')


class Solver:
    """Matrix-resident CG handle: the reference re-uploads the matrix and re-JITs
    its kernels on every call (clcg.c:142-214, cl.py:45-46,73-84); here only b goes up and x comes down."""

    def __init__(self, ctx, size, non_zeros, a_values, a_pointers, a_cols, n_rhs=1, flags=0, dtype=None, batched=False, hermitian=False, long_rows=False):
        """batched=True: n_rhs systems on one pattern (cgamd_solver_create_batched) -- a_values holds n_rhs * non_zeros entries,
        the values of system r at a_values[r * non_zeros:(r + 1) * non_zeros] in the order of a_cols, and right-hand side r
        belongs to system r.
        hermitian=True (flag HERMITIAN): the matrix is complex Hermitian positive definite -- CG with the conjugated inner product
        <a, b> = sum conj(a_i) b_i instead of the reference's unconjugated recurrence, which does not converge on such a matrix.
        history() is then r^H r (real, >= 0).  Real value types: accepted, changes nothing.
        long_rows=True (flag SPLIT_LONG_ROWS): rows too long for the block SpMV forms (hubs of a graph Laplacian) are cut across
        work-groups and every other row keeps those forms; accepted everywhere, without effect where the split does not apply (the
        property `long_rows` tells)."""
        if long_rows:
            flags = int(flags) | _lib.SPLIT_LONG_ROWS
        if hermitian:
            flags = int(flags) | _lib.HERMITIAN
        self.ctx = ctx
        self._lib = _lib.load()
        self.batched = bool(batched)
        self.non_zeros = int(non_zeros)
        on_device = self._on_device = bool(flags & _lib.MATRIX_ON_DEVICE)
        if self.batched:
            self._check_batched_values(a_values, int(n_rhs))
        if not on_device:
            self.dtype = np.dtype(dtype) if dtype is not None else np.dtype(a_values.dtype)
            a_values = np.ascontiguousarray(a_values, dtype=self.dtype)
            a_pointers = np.ascontiguousarray(a_pointers, dtype=np.intc)
            a_cols = np.ascontiguousarray(a_cols, dtype=np.intc)
        else:
            if dtype is None:
                raise ValueError("dtype is required for device-resident matrices")
            self.dtype = np.dtype(dtype)
        self._keep = (a_values, a_pointers, a_cols)      # borrowed device arrays must outlive the handle
        self.size, self.n_rhs = int(size), int(n_rhs)
        h = ctypes.c_void_p()
        create = self._lib.cgamd_solver_create_batched if self.batched else self._lib.cgamd_solver_create
        check(create(ctx.handle, _lib.DTYPE_CODE[self.dtype], self.size, int(non_zeros), ptr(a_values), ptr(a_pointers), ptr(a_cols),
                     self.n_rhs, int(flags), ctypes.byref(h)))
        self.handle = h

    def _check_batched_values(self, a_values, n_rhs):
        """a batched handle's value array holds n_rhs * non_zeros entries (arrays whose length can be read; a bare address cannot)"""
        count = a_values.numel() if hasattr(a_values, "numel") else getattr(a_values, "size", None)
        if isinstance(a_values, DeviceBuffer):
            count = a_values.nbytes // a_values.dtype.itemsize
        if count is not None and not callable(count) and int(count) != n_rhs * self.non_zeros:
            raise ValueError(f"a batched handle of {n_rhs} systems takes {n_rhs} * {self.non_zeros} = {n_rhs * self.non_zeros} "
                             f"values (the values of system r at [r * non_zeros:(r + 1) * non_zeros]), got {int(count)}")

    @property
    def systems(self):
        """systems of a batched handle (each right-hand side has a matrix of its own), 0 for every other handle"""
        return self._lib.cgamd_solver_systems(self.handle)

    @property
    def hermitian(self):
        """1 when the handle runs the conjugated recurrence (created with hermitian=True / HERMITIAN on a complex type), else 0"""
        return self._lib.cgamd_solver_hermitian(self.handle)

    LONG_ROWS_FIELDS = ("heavy_blocks", "segments", "segment", "body_kind", "body_lanes", "scratch_bytes")

    @property
    def long_rows(self):
        """what the SPLIT_LONG_ROWS form of this handle runs on (cgamd_solver_long_rows), as a dict: heavy 256-row blocks, segments,
        entries per segment, the body's kind (5 row-block, 7 chunked) and lanes per row, bytes of piece scratch; all 0 where the flag
        is not set or does not apply"""
        out = (ctypes.c_int * len(self.LONG_ROWS_FIELDS))()
        got = self._lib.cgamd_solver_long_rows(self.handle, out, len(out))
        if got < 0:
            check(-got)
        return dict(zip(self.LONG_ROWS_FIELDS, (int(v) for v in out)))

    def hermitian_scalars(self):
        """(alpha, beta) of the last iteration of a hermitian handle, n_rhs values each (development accessor: step_state describes
        the other loops and refuses these handles)"""
        a, b = np.empty(self.n_rhs, dtype=self.dtype), np.empty(self.n_rhs, dtype=self.dtype)
        check(self._lib.cgamd_solver_hermitian_scalars(self.handle, ptr(a), ptr(b)))
        return a, b

    def reload_matrix(self, a_values, a_pointers, a_cols):
        """new values / pattern of the same size and non-zero count from HOST arrays into a handle that owns its matrix
        (what the stateless cg() does between calls, include/cgamd.h); a batched handle takes n_rhs * non_zeros values"""
        a_values = np.ascontiguousarray(a_values, dtype=self.dtype)
        if self.batched:
            self._check_batched_values(a_values, self.n_rhs)
        a_pointers = np.ascontiguousarray(a_pointers, dtype=np.int32)
        a_cols = np.ascontiguousarray(a_cols, dtype=np.int32)
        check(self._lib.cgamd_solver_reload_matrix(self.handle, ptr(a_values), ptr(a_pointers), ptr(a_cols)))

    def refresh_values(self, a_values=None):
        """new VALUES on the same pattern (cgamd_solver_refresh_values): the codes of the SpMV and a preconditioner built from the
        matrix follow them; the next call must be set_rhs.  None: the borrowed device array (flags MATRIX_ON_DEVICE) was changed in
        place -- the only form such a handle takes besides the borrowed array itself.  A handle that owns its matrix takes a numpy
        array (host route) or a torch device tensor / DeviceBuffer (copied on the device); a batched one n_rhs * non_zeros values."""
        if a_values is None:
            if not self._on_device:
                raise ValueError("refresh_values: a handle that owns its matrix takes the new values (a host array or a device buffer); "
                                 "None means 'the borrowed device array changed in place'")
            if getattr(self._keep[0], "is_cuda", False):
                import torch
                torch.cuda.synchronize()        # torch rewrote the tensor on ITS stream; the library reads it on the context's
            check(self._lib.cgamd_solver_refresh_values(self.handle, None, 0))
            return
        if isinstance(a_values, int) or hasattr(a_values, "data_ptr") or hasattr(a_values, "ptr"):
            if getattr(a_values, "is_cuda", True) is False:
                a_values = a_values.numpy()
            else:
                if self.batched and not self._on_device:
                    self._check_batched_values(a_values, self.n_rhs)
                elif not self._on_device and hasattr(a_values, "numel") and int(a_values.numel()) != self.non_zeros:
                    raise ValueError(f"refresh_values: {int(a_values.numel())} values, the matrix has {self.non_zeros} non-zeros")
                if hasattr(a_values, "is_cuda"):
                    import torch
                    torch.cuda.synchronize()    # torch wrote the tensor on ITS stream; the library reads it on the context's
                check(self._lib.cgamd_solver_refresh_values(self.handle, ptr(a_values), 1))
                return
        a_values = np.ascontiguousarray(a_values, dtype=self.dtype)
        if self.batched:
            self._check_batched_values(a_values, self.n_rhs)
        elif a_values.size != self.non_zeros:
            raise ValueError(f"refresh_values: {a_values.size} values, the matrix has {self.non_zeros} non-zeros")
        check(self._lib.cgamd_solver_refresh_values(self.handle, ptr(a_values), 0))

    @property
    def last_refresh(self):
        """what the last refresh_values did (cgamd_solver_last_refresh): 0 nothing to do, 1 dictionaries rewritten in place (arrays and
        graphs kept), 2 value / joint / row codes built again, 3 the values do not qualify (the SpMV reads aValues)"""
        return self._lib.cgamd_solver_last_refresh(self.handle)

    @property
    def graph_captures(self):
        """iteration graphs captured since the handle was created (cgamd_solver_graph_captures): unchanged across calls that replay
        the graphs the handle has, e.g. across a refresh_values that rewrote the dictionaries only"""
        return self._lib.cgamd_solver_graph_captures(self.handle)

    def set_rhs(self, b, x0=None, on_device=False):
        if not on_device:
            b = np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=self.dtype)
            if x0 is not None:
                x0 = np.ascontiguousarray(np.asarray(x0).reshape(-1), dtype=self.dtype)
        check(self._lib.cgamd_solver_set_rhs(self.handle, ptr(b), ptr(x0), int(on_device)))

    # ---- multi-shift CG (include/cgamd.h "Multi-shift CG"): all (A + sigma_j I) x_j = b on the one SpMV of A x = b
    MAX_SHIFTS = 16

    def _shift_values(self, sigmas):
        """`sigmas` as the array cgamd_solver_set_shifts takes: 1 ... 16 finite values of the handle's type.  ValueError otherwise,
        before anything touches the device."""
        s = np.asarray(sigmas).reshape(-1)
        if s.size < 1 or s.size > self.MAX_SHIFTS:
            raise ValueError(f"1 ... {self.MAX_SHIFTS} shifts, got {s.size}")
        if self.dtype.kind != "c" and np.iscomplexobj(s) and np.any(s.imag != 0):
            raise ValueError("complex shifts need a complex handle")
        s = np.ascontiguousarray(s.real if self.dtype.kind != "c" else s, dtype=self.dtype)
        if not np.all(np.isfinite(s)):
            raise ValueError("every shift must be finite")
        return s

    def set_shifts(self, sigmas):
        """From the next set_rhs on the handle also solves (A + sigma_j I) x_j = b for every sigma_j (cgamd_solver_set_shifts), with
        the SpMV of the seed system alone; the seed's x and history keep their bits.  None or an empty list removes the shifts.
        Needs x0 = None and no preconditioner; the shifts are shared by all right-hand sides."""
        if sigmas is None or np.size(sigmas) == 0:
            check(self._lib.cgamd_solver_set_shifts(self.handle, None, 0))
            return
        s = self._shift_values(sigmas)
        check(self._lib.cgamd_solver_set_shifts(self.handle, ptr(s), int(s.size)))

    def shifts(self):
        """number of shifts in force"""
        got = self._lib.cgamd_solver_shifts(self.handle)
        if got < 0:
            check(-got)
        return got

    def x_shifted(self):
        """the shifted solutions, shape (shifts, n_rhs, size)"""
        out = np.empty((max(self.shifts(), 1), self.n_rhs, self.size), dtype=self.dtype)
        for j in range(self.shifts()):
            check(self._lib.cgamd_solver_get_x_shifted(self.handle, j, ptr(out[j]), 0))
        return out[:self.shifts()]

    def shift_history(self):
        """zeta_k^j, the factor between the residual of shifted system j and the seed's, r_k^j = zeta_k^j r_k, for k = 0..iterations:
        shape (iterations + 1, shifts, n_rhs).  delta_k^j = zeta_k^j ** 2 * history()[k] (unconjugated, like the history)."""
        n, S = self.iterations_done() + 1, self.shifts()
        out = np.empty((n, max(S, 1), self.n_rhs), dtype=self.dtype)
        got = self._lib.cgamd_solver_shift_history(self.handle, ptr(out), n)
        if got < 0:
            check(-got)
        return out[:got, :S]

    SHIFT_SCALARS = ("theta", "zeta", "alpha", "beta")

    def shift_scalars(self, which):
        """development entry (cgamd_solver_shift_scalars): the last iteration's theta / zeta (float64 / complex128) or alpha_j / beta_j
        (the handle's type), shape (shifts, n_rhs)"""
        idx = self.SHIFT_SCALARS.index(which) if isinstance(which, str) else int(which)
        acc = np.complex128 if self.dtype.kind == "c" else np.float64
        out = np.empty((max(self.shifts(), 1), self.n_rhs), dtype=acc if idx < 2 else self.dtype)
        check(self._lib.cgamd_solver_shift_scalars(self.handle, idx, ptr(out)))
        return out[:self.shifts()]

    def solve_shifted(self, b, sigmas, iterations=None, tol=None, maxit=1000, check_every=8):
        """A x = b and (A + sigma_j I) x_j = b in one solve: `iterations` iterations, or with `tol` (a scalar or n_rhs values) until
        the SEED's sqrt(|r.r|) falls below it, per right-hand side (iterate_until).  For positive shifts of a positive-definite matrix
        the shifted systems have then converged too; otherwise read shift_history().  Returns (x, xs, its): xs of shape
        (shifts, n_rhs, size), its the iterations of every right-hand side.  The shifts stay in force."""
        if (iterations is None) == (tol is None):
            raise ValueError("give either iterations or tol")
        if iterations is not None and int(iterations) < 0:
            raise ValueError("iterations must not be negative")
        if tol is not None:
            self._tolerances(tol)
        sigmas = self._shift_values(sigmas)
        self.set_shifts(sigmas)
        self.set_rhs(b, None)
        if tol is None:
            self.iterate(int(iterations))
            its = np.full(self.n_rhs, int(iterations), dtype=np.intc)
        else:
            its = self.iterate_until(tol, maxit, check_every)
        return self.x(), self.x_shifted(), its

    # ---- block CG (include/cgamd.h "Block CG"): the n_rhs right-hand sides of one real SPD matrix share one Krylov space
    MAX_BLOCK = 16

    def _block_check(self):
        """what block CG asks of the handle that Python can see: a real type and 2 ... 16 right-hand sides.  ValueError otherwise,
        before anything touches the device"""
        if np.dtype(self.dtype).kind == "c":
            raise ValueError("block CG serves the real value types")
        if not 2 <= self.n_rhs <= self.MAX_BLOCK:
            raise ValueError(f"block CG takes the handle's n_rhs = 2 ... {self.MAX_BLOCK} right-hand sides as its block, got {self.n_rhs}")

    def _block_tolerances(self, b, tol):
        """(b as the handle takes it, the absolute tolerance of every column): tol is relative to |b_j|, a scalar or n_rhs values"""
        t = self._tolerances(tol)
        b = np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=self.dtype)
        if b.size != self.n_rhs * self.size:
            raise ValueError(f"b must hold n_rhs x size = {self.n_rhs} x {self.size} values, got {b.size}")
        nb = np.linalg.norm(b.reshape(self.n_rhs, self.size).astype(np.float64), axis=1)
        return b, np.maximum(np.broadcast_to(t, (self.n_rhs,)) * nb, np.finfo(np.float64).tiny)

    def set_block(self, on=True):
        """From the next set_rhs on the handle runs block CG on its n_rhs right-hand sides (cgamd_solver_set_block): one Krylov space
        for all columns, fewer iterations than any single solve, six launches per iteration.  Real types, 2 ... 16 right-hand sides,
        no preconditioner and no shifts.  on=False returns the handle to the bits of one that never had it."""
        if on:
            self._block_check()
        check(self._lib.cgamd_solver_set_block(self.handle, 1 if on else 0))

    def block_status(self):
        """{"on", "status" (0 running or stopped, 1 G failed, 2 W^T W failed, 3 NaN), "iteration" (of that event), "s",
        "min_pivot_ratio", "preconditioned"} (cgamd_solver_block_status; waits for the handle's stream).  With set_block_pcg on,
        "preconditioned" is True and status 2 means W^T Z failed"""
        info = (ctypes.c_int * 4)()
        ratio = ctypes.c_double(0.0)
        check(self._lib.cgamd_solver_block_status(self.handle, info, ctypes.byref(ratio)))
        return {"on": bool(info[0]), "status": int(info[1]), "iteration": int(info[2]), "s": int(info[3]), "min_pivot_ratio": float(ratio.value),
                "preconditioned": info[0] == 2}

    def block_state(self, which):
        """development entry (cgamd_solver_block_state): one s x s matrix in float64 -- "xi", "G", "alpha", "tau", "C" (W^T W as summed),
        "tau_inv" (tau^-1), "M" (alpha xi) or, with set_block_pcg on, "CZ" (W^T Z as summed)"""
        idx = {"xi": 0, "G": 1, "alpha": 2, "tau": 3, "C": 4, "tau_inv": 5, "M": 6, "CZ": 7}[which]
        out = np.empty((self.n_rhs, self.n_rhs), dtype=np.float64)
        check(self._lib.cgamd_solver_block_state(self.handle, idx, ptr(out)))
        return out

    def solve_block(self, b, x0=None, tol=1e-6, maxit=1000, check_every=8):
        """A X = B by block CG to |r_j| <= tol |b_j| for every column (tol: a scalar or n_rhs values): all columns stop in the first
        iteration in which each satisfies its own tolerance.  Where the block breaks down -- duplicate or linearly dependent
        right-hand sides -- the solve finishes on the same handle with the ordinary per-column loop from the X reached, each column's
        tolerance still relative to the ORIGINAL |b_j|, so the answer is a converged one either way.  Returns (x, info): info["path"]
        is "block" or "block+columns", with the iterations of each part, the breakdown record and the smallest pivot ratio.
        Block CG stays on."""
        self._block_check()
        if int(maxit) < 0 or int(check_every) < 0:
            raise ValueError("maxit and check_every must not be negative")
        b, tol_abs = self._block_tolerances(b, tol)
        self.set_block(True)
        self.set_rhs(b, x0)
        its = self.iterate_until(tol_abs, maxit, check_every)
        st = self.block_status()
        info = {"path": "block", "block_iterations": int(its[0]), "column_iterations": None, "status": st["status"],
                "breakdown_iteration": st["iteration"], "min_pivot_ratio": st["min_pivot_ratio"]}
        if st["status"] == 0:
            return self.x(), info
        x = self.x()
        self.set_block(False)
        try:
            self.set_rhs(b, x)
            info["column_iterations"] = self.iterate_until(tol_abs, max(int(maxit) - int(its[0]), 0), check_every)
            info["path"] = "block+columns"
            x = self.x()
        finally:
            self.set_block(True)
        return x, info

    # ---- preconditioned block CG (include/cgamd.h "Preconditioned block CG"): the shared Krylov space with the M in force inside
    def set_block_pcg(self, on=True):
        """From the next set_rhs on the handle runs block CG on its n_rhs right-hand sides WITH the preconditioner in force inside the
        recurrence (cgamd_solver_set_block_pcg): install M first (set_preconditioner), then turn this on; while it is on M cannot
        be replaced or removed.  Real types, 2 ... 16 right-hand sides, no shifts; set_block and set_block_pcg exclude each other.
        on=False returns the handle to the bits of the scalar PCG handle it was."""
        if on:
            self._block_check()
        check(self._lib.cgamd_solver_set_block_pcg(self.handle, 1 if on else 0))

    def solve_block_pcg(self, b, M, x0=None, tol=1e-6, maxit=1000, check_every=8):
        """A X = B by preconditioned block CG to |r_j| <= tol |b_j| for every column (tol: a scalar or n_rhs values).  M as in
        set_preconditioner / pcg; None keeps the M already in force, and raises ValueError when there is none.  All columns stop in the
        first iteration in which each satisfies its own tolerance.  Where the block breaks down -- dependent right-hand sides, or an M
        that is not positive definite on the block -- the block is turned off and the solve finishes column by column on the same
        handle with the scalar PCG loop (solve_until's) from the X reached, M still in force, each column's tolerance relative to the
        ORIGINAL |b_j|.  Returns (x, info) like solve_block: info["path"] is "block" or "block+columns".  The mode and M stay on."""
        self._block_check()
        if int(maxit) < 0 or int(check_every) < 0:
            raise ValueError("maxit and check_every must not be negative")
        b, tol_abs = self._block_tolerances(b, tol)
        if M is not None:
            was_on = self.block_status()["preconditioned"]
            self.set_block_pcg(False)       # (M is part of the block's state: it is replaced with the mode off)
            try:
                self.set_preconditioner(M)
            except Exception:               # an M that is refused: the mode comes back over the M that is still in force
                if was_on and self._lib.cgamd_solver_preconditioner_source(self.handle) != 0:
                    self.set_block_pcg(True)
                raise
        elif self._lib.cgamd_solver_preconditioner_source(self.handle) == 0:
            raise ValueError("solve_block_pcg: M is None and no preconditioner is in force")
        self.set_block_pcg(True)
        self.set_rhs(b, x0)
        its = self.iterate_until(tol_abs, maxit, check_every)
        st = self.block_status()
        info = {"path": "block", "block_iterations": int(its[0]), "column_iterations": None, "status": st["status"],
                "breakdown_iteration": st["iteration"], "min_pivot_ratio": st["min_pivot_ratio"]}
        if st["status"] == 0:
            return self.x(), info
        x = self.x()
        self.set_block_pcg(False)
        try:
            self.set_rhs(b, x)
            info["column_iterations"] = self.iterate_until(tol_abs, max(int(maxit) - int(its[0]), 0), check_every)
            info["path"] = "block+columns"
            x = self.x()
        finally:
            self.set_block_pcg(True)
        return x, info

    # ---- solution projection (include/cgamd.h "Solution projection"): start each solve from the span of the earlier ones
    def enable_projection(self, capacity, drop_tol=0.0):
        """Keep up to `capacity` (1 ... 32) A-orthonormal vectors per right-hand-side column spanning the recent solutions
        (cgamd_solver_projection_enable); 0 disables the feature and frees the storage.  A vector whose A-norm squared is not above
        drop_tol^2 |<x, A x>| is not stored.  refresh_values and reload_matrix clear the basis."""
        check(self._lib.cgamd_solver_projection_enable(self.handle, int(capacity), float(drop_tol)))
        self._projection_capacity = int(capacity)

    def projection_count(self):
        """slots held, 0 ... capacity"""
        got = self._lib.cgamd_solver_projection_count(self.handle)
        if got < 0:
            check(-got)
        return got

    def projection_clear(self):
        check(self._lib.cgamd_solver_projection_clear(self.handle))

    def set_rhs_projected(self, b, on_device=False):
        """set_rhs(b, x0) with x0 the A-projection of the solution onto the span of the vectors held (x0 = 0 with none)"""
        if not on_device:
            b = np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=self.dtype)
        check(self._lib.cgamd_solver_set_rhs_projected(self.handle, ptr(b), int(on_device)))

    def projection_update(self):
        """Add what the solve found beyond the span (after iterate / iterate_until of a right-hand side set by set_rhs_projected);
        returns the `added` flags, one bool per right-hand side.  The next call on the handle must be a set_rhs of either kind."""
        added = np.zeros(self.n_rhs, dtype=np.intc)
        check(self._lib.cgamd_solver_projection_update(self.handle, added.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return added != 0

    PROJECTION_STATES = ("slot", "x0", "alpha", "c", "nu_s")

    def projection_state(self, which, slot=0):
        """development entry (cgamd_solver_projection_state).  which 0 / "slot": vector `slot`, (n_rhs, size); 1 / "x0": the last guess,
        (n_rhs, size); 2 / "alpha", 3 / "c": (capacity, n_rhs) of the handle's type; 4 / "nu_s": (2, n_rhs) float64 / complex128"""
        idx = self.PROJECTION_STATES.index(which) if isinstance(which, str) else int(which)
        cap = getattr(self, "_projection_capacity", 0)
        acc = np.complex128 if self.dtype.kind == "c" else np.float64
        if idx in (0, 1):
            out = np.empty((self.n_rhs, self.size), dtype=self.dtype)
        elif idx in (2, 3):
            out = np.empty((max(cap, 1), self.n_rhs), dtype=self.dtype)
        else:
            out = np.empty((2, self.n_rhs), dtype=acc)
        check(self._lib.cgamd_solver_projection_state(self.handle, idx, int(slot), ptr(out)))
        return out

    def set_preconditioner(self, m):
        """The reference's PCG preconditioner `M` (helmFE_var.py:546-586), chosen by the reference's own rule:
        * None: plain CG again.
        * "jacobi": 1/diag(A) of the handle's own matrix, built on the device (cgamd_solver_set_preconditioner_jacobi), then the
          diagonal branch.
        * ("line", stride): the tridiagonal M of the handle's own matrix, its entries at column - row in {-stride, 0, +stride}
          (stride 1: x-lines, nx: y-lines, nx * ny: z-lines), extracted, factored and planned on the device
          (cgamd_solver_set_preconditioner_line); the spsolve branch below without the host work.  Both follow reload_matrix.
        * ("multigrid", (nx, ny, nz)) or ("multigrid", (nx, ny, nz), {"smooth_steps": 1, "over_correction": 1.6, "min_rows": 512}):
          one aggregation-multigrid V-cycle on the grid the rows number x fastest (nx * ny * nz == size; 2-D: (nx, ny) or nz = 1),
          the hierarchy built on the device from the handle's matrix (cgamd_solver_set_preconditioner_multigrid): the
          preconditioner for isotropic stencil systems, where it cuts the iteration count by a multiple.  Follows reload_matrix and
          refresh_values.  mg_levels() lists the hierarchy.
        * "amg" or ("amg", {"passes": 3, "strength": 0.25, "smooth_steps": 1, "over_correction": 1.6, "min_rows": 512}): the same
          V-cycle on aggregates matched from the matrix itself on the device (cgamd_solver_set_preconditioner_amg): no grid
          needed -- a Matrix-Market file, a permuted grid matrix, a mesh -- and anisotropy is followed, not crossed.  Follows
          reload_matrix and refresh_values (aggregates included).  mg_levels() and mg_aggregates(level) list the hierarchy.
        * a 1-D array (1/diag(A) for Jacobi), a device buffer, or a scipy sparse M with nnz <= size: the diagonal branch,
          z = M.dot(r);
        * a scipy sparse M with nnz > size: the spsolve branch, z solves M z = r.  M must be tridiagonal along one grid axis: all
          its stored non-zeros on |i - j| in {0, 1} (e.g. the reference driver's `Htrid` on a grid of more than 10 nodes per
          line), or all on |i - j| in {0, s} for one s > 1 (the line preconditioner along another axis of a grid numbered x
          fastest: s = nx for y-lines, nx * ny for z-lines).  It is factored once on the host without pivoting (a zero pivot
          raises CgAmdError) and solved on the device, by line sweeps (s = 1) or one thread per line (s > 1).  Such handles
          run a launched loop only (no resident loop, no device-side stop).
        Any other M raises ValueError.  Takes effect at the next set_rhs; history() keeps returning r.r.

        A batched handle takes one M per system (cgamd_solver_set_preconditioner_batched*): None, "jacobi" (1 / diag(A_r)),
        ("line", stride) (the lines of every A_r, one segment plan for all), ("multigrid", dims[, opts]) (one V-cycle per system on a
        hierarchy of its own over shared aggregates, cgamd_solver_set_preconditioner_batched_multigrid), a host array of n_rhs * size entries (1-D, or
        (n_rhs, size): row r multiplies the residual of system r), a device buffer of that many, or a list of n_rhs scipy matrices
        with nnz <= size each (their diagonals)."""
        if self.batched:
            _set_preconditioner_batched(self, m)
            return
        if m is None:
            check(self._lib.cgamd_solver_set_preconditioner(self.handle, None, 0))
            return
        named_amg = isinstance(m, str) and m == "amg"
        if named_amg or (isinstance(m, tuple) and len(m) == 2 and m[0] == "amg"):
            opts = {} if named_amg else dict(m[1])
            if set(opts) - {"passes", "strength", "smooth_steps", "over_correction", "min_rows"}:
                raise ValueError('"amg" or ("amg", {"passes": 3, "strength": 0.25, "smooth_steps": 1, "over_correction": 1.6, "min_rows": 512})')
            check(self._lib.cgamd_solver_set_preconditioner_amg(self.handle, int(opts.get("passes", 0)), float(opts.get("strength", 0.0)),
                                                                int(opts.get("smooth_steps", 0)), float(opts.get("over_correction", 0.0)),
                                                                int(opts.get("min_rows", 0))))
            return
        if isinstance(m, str):
            if m != "jacobi":
                raise ValueError('preconditioner by name: "jacobi", "amg" or ("line", stride)')
            check(self._lib.cgamd_solver_set_preconditioner_jacobi(self.handle))
            return
        if isinstance(m, tuple) and len(m) == 2 and m[0] == "line":
            check(self._lib.cgamd_solver_set_preconditioner_line(self.handle, int(m[1])))
            return
        if isinstance(m, tuple) and len(m) in (2, 3) and m[0] == "multigrid":
            dims = tuple(int(d) for d in m[1]) + (1,) * (3 - len(m[1]))
            opts = dict(m[2]) if len(m) == 3 else {}
            unknown = set(opts) - {"smooth_steps", "over_correction", "min_rows"}
            if len(dims) != 3 or unknown:
                raise ValueError('("multigrid", (nx, ny, nz)[, {"smooth_steps": 1, "over_correction": 1.6, "min_rows": 512}])')
            check(self._lib.cgamd_solver_set_preconditioner_multigrid(self.handle, dims[0], dims[1], dims[2], int(opts.get("smooth_steps", 0)),
                                                                      float(opts.get("over_correction", 0.0)), int(opts.get("min_rows", 0))))
            return
        if hasattr(m, "diagonal") and hasattr(m, "nnz"):          # scipy sparse, as the reference passes it
            if m.shape != (self.size, self.size):
                raise ValueError("preconditioner M must be size x size")
            if m.nnz > m.shape[0]:
                self._set_tridiag(m)
                return
            m = m.diagonal()
        on_device = not isinstance(m, np.ndarray) and not isinstance(m, (list, tuple))
        if not on_device:
            m = np.ascontiguousarray(np.asarray(m).reshape(-1), dtype=self.dtype)
            if m.size != self.size:
                raise ValueError("preconditioner diagonal must have `size` entries")
        check(self._lib.cgamd_solver_set_preconditioner(self.handle, ptr(m), int(on_device)))

    def mg_levels(self):
        """the multigrid hierarchy in force: a list of dicts (rows, nnz, nx, ny, nz, lmax), level 0 first; [] without one.  On a
        batched handle lmax is the list of the n_rhs per-system bounds"""
        out = []
        for l in range(max(0, self._lib.cgamd_solver_mg_levels(self.handle))):
            info = (ctypes.c_longlong * 6)()
            check(self._lib.cgamd_solver_mg_level(self.handle, l, info))
            out.append({"rows": int(info[0]), "nnz": int(info[1]), "nx": int(info[2]), "ny": int(info[3]), "nz": int(info[4]),
                        "lmax": float(np.array([info[5]], dtype=np.int64).view(np.float64)[0])})
            if self.batched:
                out[-1]["lmax"] = [float(v) for v in self.mg_level_bounds(l)]
        return out

    def mg_level_bounds(self, level):
        """lmax of every system of a level of the hierarchy in force (one value on a handle that is not batched), doubles"""
        out = (ctypes.c_double * (self.n_rhs if self.batched else 1))()
        check(self._lib.cgamd_solver_mg_level_bounds(self.handle, int(level), out, len(out)))
        return np.array(out[:], dtype=np.float64)

    def mg_level_matrix(self, level):
        """(indptr, indices, data) of a level of the multigrid hierarchy, copied to the host (development accessor: tests); on a
        batched handle data has shape (n_rhs, nnz), row r the values of system r"""
        info = self.mg_levels()[level]
        ip, ix = np.empty(info["rows"] + 1, np.int32), np.empty(info["nnz"], np.int32)
        da = np.empty((self.n_rhs, info["nnz"]) if self.batched else info["nnz"], self.dtype)
        check(self._lib.cgamd_solver_mg_level_matrix(self.handle, int(level), ptr(ip), ptr(ix), ptr(da)))
        return ip, ix, da

    def mg_aggregates(self, level):
        """(agg, n_coarse): the map of the rows of `level` to the rows of level + 1 of the hierarchy in force (an algebraic
        hierarchy's stored map or a grid hierarchy's boxes), copied to the host (development accessor: tests)"""
        agg = np.empty(self.mg_levels()[level]["rows"], np.int32)
        nc = ctypes.c_int(0)
        check(self._lib.cgamd_solver_mg_aggregates(self.handle, int(level), ptr(agg), ctypes.byref(nc)))
        return agg, int(nc.value)

    def mg_apply(self, r):
        """z = one V-cycle of r: n_rhs * size values, host array in and out (development accessor: tests)"""
        r = np.ascontiguousarray(np.asarray(r).reshape(-1), dtype=self.dtype)
        if r.size != self.n_rhs * self.size:
            raise ValueError("mg_apply takes n_rhs * size values")
        rd, zd = DeviceBuffer(self.ctx, hostbuf=r), DeviceBuffer(self.ctx, nbytes=r.nbytes, dtype=self.dtype)
        try:
            check(self._lib.cgamd_solver_mg_apply(self.handle, ptr(rd), ptr(zd)))
            return zd.get()
        finally:
            rd.release()
            zd.release()

    def mg_level_state(self, level, which):
        """one piece of what a level of the hierarchy in force holds (include/cgamd.h cgamd_solver_mg_level_state; development
        accessor: tests).  which 0: a dict (n, nu, ld, steps, algebraic); 1: dinv, n values; 2 / 3: c0 / c1, doubles; 4: the member
        lists, (rows of the next level, 8) ints"""
        dtype = {1: self.dtype, 2: np.float64, 3: np.float64}.get(which, np.intc)
        count = ctypes.c_longlong(0)
        probe = np.empty(1, dtype)
        rc = self._lib.cgamd_solver_mg_level_state(self.handle, int(level), int(which), ptr(probe), 0, ctypes.byref(count))
        if rc != 0 and count.value == 0:
            check(rc)
        out = np.empty(count.value, dtype)
        check(self._lib.cgamd_solver_mg_level_state(self.handle, int(level), int(which), ptr(out), out.size, ctypes.byref(count)))
        if which == 0:
            return dict(zip(("n", "nu", "ld", "steps", "algebraic"), (int(v) for v in out)))
        return out.reshape(-1, 8) if which == 4 else out

    def mg_level_spmv(self, level, x_dev, w_dev):
        """w = A_level x as the V-cycle launches it, on device vectors of n_rhs * ld values at the level's leading dimension
        (development accessor: tests); last_spmv_form() then reports what ran"""
        check(self._lib.cgamd_solver_mg_level_spmv(self.handle, int(level), ptr(x_dev), ptr(w_dev)))

    def _set_tridiag(self, m):
        """the three diagonals of a sparse M with nnz > size into cgamd_solver_set_preconditioner_tridiag, or, when they lie at
        distance s > 1, into cgamd_solver_set_preconditioner_tridiag_strided"""
        coo = m.tocoo()
        dist = np.unique(np.abs(coo.row.astype(np.int64) - coo.col)[coo.data != 0])
        far = dist[dist > 1]
        if far.size > 1 or (far.size == 1 and 1 in dist):
            raise ValueError("only a diagonal or tridiagonal M is supported: stored non-zeros on |i - j| <= 1, or on |i - j| in "
                             "{0, s} for one stride s (the strided tridiagonal form); M has them at distances "
                             f"{dist[:8].tolist()} (the reference's general spsolve branch is out of scope)")
        n = self.size
        lower, diag, upper = np.zeros(n, self.dtype), np.zeros(n, self.dtype), np.zeros(n, self.dtype)
        diag[:] = m.diagonal(0)
        if far.size == 1:
            s = int(far[0])
            lower[s:] = m.diagonal(-s)
            upper[:-s] = m.diagonal(s)
            check(self._lib.cgamd_solver_set_preconditioner_tridiag_strided(self.handle, s, ptr(lower), ptr(diag), ptr(upper), 0))
            return
        if n > 1:
            lower[1:] = m.diagonal(-1)
            upper[:-1] = m.diagonal(1)
        check(self._lib.cgamd_solver_set_preconditioner_tridiag(self.handle, ptr(lower), ptr(diag), ptr(upper), 0))

    def iterate(self, n_iterations):
        check(self._lib.cgamd_solver_iterate(self.handle, int(n_iterations)))

    def replace_residual(self, r):
        """Residual replacement with the direction kept (cgamd_solver_replace_residual): r := `r`, x := 0, delta := r.r (rho := r.z
        with a diagonal M), d stays; the iteration count and the history restart and every right-hand side is active again.  iterate()
        and iterate_until() then continue the recurrence from (0, r, d).  r: n_rhs * size values of the handle's type -- a device
        array (torch tensor, DeviceBuffer, address), or a numpy array, which is uploaded first (the call then waits for the stream)."""
        if isinstance(r, np.ndarray):
            buf = DeviceBuffer(self.ctx, hostbuf=np.ascontiguousarray(r.reshape(-1), dtype=self.dtype))
            try:
                check(self._lib.cgamd_solver_replace_residual(self.handle, ptr(buf)))
                self.ctx.synchronize()
            finally:
                buf.release()
            return
        check(self._lib.cgamd_solver_replace_residual(self.handle, ptr(r)))

    def iterate_timed(self, n_iterations):
        """n_iterations plain-launch iterations with HIP events around every SpMV: (avg SpMV ms, avg iteration ms)"""
        a, b = ctypes.c_float(), ctypes.c_float()
        check(self._lib.cgamd_solver_iterate_timed(self.handle, int(n_iterations), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def x(self, out=None):
        if out is None:
            out = np.empty(self.size * self.n_rhs, dtype=self.dtype)
        on_device = not isinstance(out, np.ndarray)
        check(self._lib.cgamd_solver_get_x(self.handle, ptr(out), int(on_device)))
        if on_device:
            self.ctx.synchronize()      # the copy ran on the solver's stream; make it visible to the caller's
        return out

    def iterations_done(self):
        return int(self._lib.cgamd_solver_iterations_done(self.handle))

    def history(self):
        """delta_k = r_k . r_k (unconjugated; a hermitian handle: r_k^H r_k, imaginary part +0) for k = 0..iterations; shape
        (iterations+1, n_rhs)."""
        n = self._lib.cgamd_solver_iterations_done(self.handle) + 1
        out = np.empty((n, self.n_rhs), dtype=self.dtype)
        got = self._lib.cgamd_solver_history(self.handle, ptr(out), n)
        if got < 0:
            check(-got)
        return out[:got]

    def solve(self, b, x0=None, n_iterations=10):
        self.set_rhs(b, x0)
        self.iterate(n_iterations)
        return self.x(), self.history()

    def spmv(self, x, y, fused_dot=False):
        check(self._lib.cgamd_solver_spmv(self.handle, ptr(x), ptr(y), int(fused_dot)))

    SPMV_FAMILIES = ("stream", "rowblock", "vc", "vcp", "chunked", "spmm", "batched")
    SPMV_FAMILIES_EXTRA = ("rowcode", "rowpair")      # family numbers from len(SPMV_FAMILIES) on
    SPMV_FAMILIES_SPLIT = ("split",)                  # family 9, SPLIT_LONG_ROWS (a tuple of its own: the two above are pinned by tests)
    SPMV_FORM_FIELDS = ("family", "vec", "width", "index_bits", "value_codes", "nt", "fused", "wide", "grid", "partials")

    def last_spmv_form(self):
        """what this thread's last SpMV launch really was (include/cgamd.h cgamd_last_spmv_form), as a dict: family by name, `width` =
        batch length / lanes per row / SpMM group width, `index_bits` 0 / 8 / 16, `value_codes` 0 / 1 (own stream) / 2 (joint) / 3 (one row-pattern
        byte per row)"""
        out = (ctypes.c_int * len(self.SPMV_FORM_FIELDS))()
        got = self._lib.cgamd_last_spmv_form(out, len(out))
        if got < 0:
            check(-got)
        return self._named_form(out)

    def _named_form(self, fields):
        form = dict(zip(self.SPMV_FORM_FIELDS, (int(v) for v in fields)))
        names = self.SPMV_FAMILIES + self.SPMV_FAMILIES_EXTRA + self.SPMV_FAMILIES_SPLIT
        form["family"] = names[form["family"]] if form["family"] >= 0 else None
        return form

    SPMV_FORM_INPUTS = 62

    def spmv_form(self, fused=True, with_inputs=False):
        """the form the SpMV of this handle's launched loop will take (include/cgamd.h cgamd_solver_spmv_form), in the layout of
        last_spmv_form(); nothing is launched.  with_inputs: (form, the ints of the call, plan and tuning the decision read)"""
        out = (ctypes.c_int * len(self.SPMV_FORM_FIELDS))()
        inputs = (ctypes.c_int * self.SPMV_FORM_INPUTS)()
        got = self._lib.cgamd_solver_spmv_form(self.handle, 1 if fused else 0, inputs, len(inputs), out, len(out))
        if got < 0:
            check(-got)
        form = self._named_form(out)
        return (form, [int(v) for v in inputs]) if with_inputs else form

    def dot_partials(self):
        """the d.q partials of the last spmv(..., fused_dot=True): (n_rhs, partials per right-hand side), float64 / complex128"""
        per = ctypes.c_int()
        probe = np.empty(1, np.complex128)
        self._lib.cgamd_solver_dot_partials(self.handle, ptr(probe), 0, ctypes.byref(per))      # too small on purpose: the count
        out = np.empty((self.n_rhs, per.value), dtype=np.complex128 if self.dtype.kind == "c" else np.float64)
        check(self._lib.cgamd_solver_dot_partials(self.handle, ptr(out), out.size, ctypes.byref(per)))
        return out

    STEP_PLAN_FIELDS = ("n", "ld", "vgrid", "n_partials", "kdq", "krr", "fold", "alpha2", "vec", "vec_nt", "x_lag")
    STEP_STATES = ("part_rr", "part_rz", "alpha", "beta", "delta", "rho2", "iter")

    def step_plan(self):
        """what the vector and scalar launches of this handle use now (include/cgamd.h cgamd_solver_step_plan), as a dict of ints"""
        out = (ctypes.c_int * len(self.STEP_PLAN_FIELDS))()
        got = self._lib.cgamd_solver_step_plan(self.handle, out, len(out))
        if got < 0:
            check(-got)
        return dict(zip(self.STEP_PLAN_FIELDS, (int(v) for v in out)))

    def step_state(self, which):
        """one piece of the iteration's state, copied from the device after its stream has drained (cgamd_solver_step_state):
        "part_rr" / "part_rz": (n_rhs, vgrid) float64 / complex128; "alpha", "beta", "delta": (n_rhs,) and "rho2": (2, n_rhs) of the
        handle's type; "iter": the iteration counter as an int"""
        idx = self.STEP_STATES.index(which)
        count = ctypes.c_longlong()
        probe = np.empty(1, np.complex128)
        self._lib.cgamd_solver_step_state(self.handle, idx, ptr(probe), 0, ctypes.byref(count))      # too small on purpose: the count
        if count.value < 1:
            check(self._lib.cgamd_solver_step_state(self.handle, idx, ptr(probe), 0, ctypes.byref(count)))
        acc = np.complex128 if self.dtype.kind == "c" else np.float64
        out = np.empty(count.value, dtype=acc if idx < 2 else np.intc if idx == 6 else self.dtype)
        check(self._lib.cgamd_solver_step_state(self.handle, idx, ptr(out), out.size, ctypes.byref(count)))
        if idx == 6:
            return int(out[0])
        return out.reshape((self.n_rhs, -1) if idx < 2 else (2, self.n_rhs) if idx == 5 else (self.n_rhs,))

    ROWMAJOR_PLAN_FIELDS = ("n", "rc", "nh", "tq_fused", "tq_plain", "strips", "nwg_fused", "nwg_plain", "vgrid", "nt_axpy_dot", "nt_aypx_x",
                            "kdq", "krr", "paced_fused", "paced_plain", "lead", "n_partials")

    def rowmajor_plan(self):
        """what the launches of this handle's row-major loop use now (include/cgamd.h cgamd_solver_rowmajor_plan), as a dict of ints"""
        out = (ctypes.c_int * len(self.ROWMAJOR_PLAN_FIELDS))()
        got = self._lib.cgamd_solver_rowmajor_plan(self.handle, out, len(out))
        if got < 0:
            check(-got)
        return dict(zip(self.ROWMAJOR_PLAN_FIELDS, (int(v) for v in out)))

    def spmm_rowmajor(self, x, y, n_rhs):
        """Y[size][n_rhs] = A X on the matrix cores; x, y ROW-MAJOR device arrays, n_rhs in {16, 32}, f32/f64"""
        check(self._lib.cgamd_solver_spmm_rowmajor(self.handle, ptr(x), ptr(y), int(n_rhs)))

    def vector(self, which):
        """device pointer of one of the handle's own vectors; right-hand side k starts at k * self.ld values"""
        return self._lib.cgamd_solver_vector(self.handle, {"x": 0, "r": 1, "d": 2, "q": 3}[which])

    @property
    def ld(self):
        return self._lib.cgamd_solver_ld(self.handle)

    @property
    def preconditioner_source(self):
        """0: no preconditioner; 1: from the caller's arrays; 2: from the handle's matrix, built on the device; 3: from the matrix,
        extracted on the device and factored by the host route (long segments)"""
        return self._lib.cgamd_solver_preconditioner_source(self.handle)

    @property
    def spmv_bytes(self):
        return self._lib.cgamd_solver_spmv_bytes(self.handle)

    @property
    def index_codes(self):
        """distinct (column - row) offsets when the SpMV reads one-byte column codes instead of aCols, else 0"""
        return self._lib.cgamd_solver_index_codes(self.handle)

    @property
    def value_codes(self):
        """distinct matrix entries behind the one-byte value codes of the SpMV (0 = the kernel reads aValues)"""
        return self._lib.cgamd_solver_value_codes(self.handle)

    @property
    def joint_codes(self):
        """distinct (offset, value) pairs when the SpMV reads one joint code byte per non-zero, else 0"""
        return self._lib.cgamd_solver_joint_codes(self.handle)

    @property
    def row_codes(self):
        """distinct row patterns when the SpMV reads one pattern byte per row (no per-non-zero bytes, no row pointers), else 0"""
        return self._lib.cgamd_solver_row_codes(self.handle)

    @property
    def row_pipe(self):
        """row blocks whose gathers the row-coded SpMV keeps in flight per wave (1, 2 or 4); 0 when another form runs"""
        return self._lib.cgamd_solver_row_pipe(self.handle)

    @property
    def row_pairs(self):
        """distinct row-pair patterns when the row-coded SpMV takes two rows per lane (one byte per pair of rows, one 16-byte gather
        per slot), else 0"""
        return self._lib.cgamd_solver_row_pairs(self.handle)

    @property
    def spmv_schedule(self):
        """how the row- or pair-coded SpMV deals its 1024-row super blocks to the XCDs: {"kind": "plane" (the plane-matched table) or
        "cycle" (block-cyclic, tuning key spmv_cycle), "grid": work-groups per launch, "unit_rows": the handle's largest stride in rows};
        grid and unit_rows are 0 when another SpMV form runs"""
        kind, grid, unit = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_longlong(0)
        check(self._lib.cgamd_solver_spmv_schedule(self.handle, ctypes.byref(kind), ctypes.byref(grid), ctypes.byref(unit)))
        return {"kind": "plane" if kind.value == 1 else "cycle", "grid": grid.value, "unit_rows": unit.value}

    def iter_bytes(self, fused=False):
        return self._lib.cgamd_solver_iter_bytes(self.handle, int(fused))

    @property
    def spmv_moved_bytes(self):
        """bytes the handle's SpMV really moves per launch (index bytes as the kernel reads them): what a roofline fraction is priced on"""
        return self._lib.cgamd_solver_spmv_moved_bytes(self.handle)

    @property
    def iter_moved_bytes(self):
        """bytes one iteration of the handle's launched loop moves (its own vector passes, its own index bytes)"""
        return self._lib.cgamd_solver_iter_moved_bytes(self.handle)

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None) and not getattr(self, "_borrowed", False):
            self._lib.cgamd_solver_destroy(self.handle)     # (the two handles of a MixedSolver belong to it)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


    def solve_tol(self, b, x0=None, tol=1e-5, maxit=1000, check_every=8):
        """Tolerance-stopping variant of the reference's NumPy sub-solver (p_h-PY_C-CL.py:1338-1369, UseCG==5), which breaks
        at the first iteration with sqrt(|r.r|) < tol.  The residual history stays on the device and is read back every
        `check_every` iterations (one small read-back instead of the reference's per-iteration host reductions), more often
        as the residual nears the tolerance (_run_to_tol); when a check still overshot the first iteration that met the
        tolerance, the solve is re-run for exactly that many iterations, so x is the iterate the reference returns and not one
        from past convergence (where d.q can reach 0 and alpha 0/0).
        Returns (x, iterations_run, history).  Single right-hand side."""
        if self.n_rhs != 1:
            raise ValueError("solve_tol handles one right-hand side")
        if self._lib.cgamd_solver_loop_launches(self.handle) < 2:
            # resident loop: the stop happens on the device, in the iteration the reference stops in (no read-backs, no re-run)
            self.set_rhs(b, x0)
            run_ = ctypes.c_int(0)
            st = self._lib.cgamd_solver_iterate_tol(self.handle, int(maxit), float(tol), ctypes.byref(run_))
            if st == 0:
                return self.x(), int(run_.value), self.history()
            if st != _lib.ERR_STATE:        # only "the resident loop is not available for this call" falls back; a GPU failure is reported
                check(st)

        its = self._run_to_tol(b, x0, tol, int(maxit), int(check_every))
        return self.x(), its, self.history()

    def _run_to_tol(self, b, x0, tol, maxit, check_every):
        """Host-driven tolerance stop for the launched loops: iterate in chunks, read the residual history back after each,
        and leave x at the FIRST iteration whose sqrt(|r.r|) is below tol (or NaN).  The chunk shrinks as the residual nears
        the tolerance (the decay rate of the last chunk predicts how many iterations are left), down to single iterations,
        so the loop normally ends exactly there; when a chunk still overshot, the solve is re-run for exactly that many
        iterations.  Returns the number of iterations run."""
        self.set_rhs(b, x0)
        done, step, its = 0, max(1, check_every), maxit
        while done < maxit:
            s_ = min(step, maxit - done)
            self.iterate(s_)
            done += s_
            norms = np.sqrt(np.abs(self.history()[:, 0]))
            hit = np.nonzero(~(norms[1:] >= tol))[0]                # below tol, or NaN
            if hit.size:
                its = int(hit[0]) + 1
                break
            cur, start = float(norms[-1]), float(norms[-1 - s_])
            step = max(1, check_every)
            if 0.0 < cur < start and tol > 0:
                togo = np.log(tol / cur) / (np.log(cur / start) / s_)     # iterations left at the last chunk's rate
                if togo < 2 * step:
                    step = max(1, int(togo / 2))
        if self.iterations_done() != its:
            self.set_rhs(b, x0)
            self.iterate(its)
        return its

    def _tolerances(self, tol):
        """`tol` as the float64 array cgamd_solver_iterate_until takes: one tolerance for all right-hand sides or n_rhs of them, all
        positive.  ValueError otherwise, before anything touches the device."""
        t = np.ascontiguousarray(np.asarray(tol, dtype=np.float64).reshape(-1))
        if t.size not in (1, self.n_rhs):
            raise ValueError(f"tol must be a scalar or have n_rhs = {self.n_rhs} entries, got {t.size}")
        if not np.all(t > 0):
            raise ValueError("every tolerance must be positive")
        return t

    def iterate_until(self, tol, maxit, check_every=8):
        """At most `maxit` more iterations with a stop per right-hand side ON THE DEVICE (cgamd_solver_iterate_until): right-hand
        side r stops in the first iteration whose sqrt(|r.r|) is not >= tol[r] (or NaN) and keeps the x of exactly that iteration
        while the others run on.  tol: a scalar or n_rhs values.  The host looks at one device word per `check_every` iterations,
        one chunk behind the device; the result does not depend on it.  Returns the iterations of every right-hand side since
        set_rhs (int array of n_rhs).  May be repeated; once a right-hand side has stopped, iterate() raises until the next
        set_rhs."""
        t = self._tolerances(tol)
        if int(maxit) < 0 or int(check_every) < 0:
            raise ValueError("maxit and check_every must not be negative")
        its = np.zeros(self.n_rhs, dtype=np.intc)
        check(self._lib.cgamd_solver_iterate_until(self.handle, int(maxit), t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(t.size),
                                                   int(check_every), its.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return its

    def solve_until(self, b, x0=None, tol=1e-5, maxit=1000, check_every=8, project=False):
        """The reference's tolerance-stopping sub-solver (p_h-PY_C-CL.py:1338-1369; with a preconditioner set, PCG's stop,
        helmFE_var.py:580-584) for ALL right-hand sides of the handle in one solve, batched handles included: each stops on its own
        tolerance (`tol`: a scalar or n_rhs values) in the iteration the reference stops in, and its x is the iterate of that
        iteration.  Returns (x, iterations per right-hand side, history); the history column of a right-hand side that stopped
        early repeats its last entry down to the last row.
        project=True (enable_projection first): the solve starts from the projection onto the span of the earlier solutions instead
        of x0, which must be None, and the basis is updated from its result (set_rhs_projected, iterate_until, projection_update)."""
        self._tolerances(tol)
        if project:
            if x0 is not None:
                raise ValueError("project=True chooses the initial guess: x0 must be None")
            self.set_rhs_projected(b)
            its = self.iterate_until(tol, maxit, check_every)
            out = self.x(), its, self.history()
            self.projection_update()
            return out
        self.set_rhs(b, x0)
        its = self.iterate_until(tol, maxit, check_every)
        return self.x(), its, self.history()

    def pcg(self, b, M=None, x0=None, tol=1e-6, maxit=1000, check_every=8, project=False):
        """`PCG(A, b, M, x, tol, maxit)` of the reference (helmFE_var.py:546-586) for M = None, a diagonal M, a tridiagonal
        sparse M along any grid axis (the spsolve branch) or "jacobi" / ("line", stride) / ("multigrid", dims) / "amg" built from the matrix (see set_preconditioner): stops when sqrt(|r.r|) < tol, returns (x, i) with i the 0-based
        index of the last iteration run, like the reference.  The residual history stays on the device and is read back every
        `check_every` iterations; x is taken at the first iteration that met the tolerance by re-running exactly that many
        iterations when the check overshot it.
        project=True (enable_projection first): the solve starts from the projection onto the span of the earlier solutions instead
        of x0, which must be None, stops on the device (iterate_until), and the basis is updated from its result."""
        if self.n_rhs != 1:
            raise ValueError("pcg handles one right-hand side")
        if project and x0 is not None:
            raise ValueError("project=True chooses the initial guess: x0 must be None")
        self.set_preconditioner(M)
        try:
            if project:
                self.set_rhs_projected(b)
                its = self.iterate_until(tol, int(maxit), check_every) if int(maxit) > 0 else np.zeros(1, np.intc)
                x = self.x()
                self.projection_update()
                return x, int(its[0]) - 1
            if int(maxit) > 0 and self._lib.cgamd_solver_loop_launches(self.handle) < 2:
                self.set_rhs(b, x0)             # resident loop (with a diagonal M: the chip-wide groups): the stop happens on the device
                run_ = ctypes.c_int(0)
                st = self._lib.cgamd_solver_iterate_tol(self.handle, int(maxit), float(tol), ctypes.byref(run_))
                if st == 0:
                    return self.x(), int(run_.value) - 1
                if st != _lib.ERR_STATE:
                    check(st)
            its = self._run_to_tol(b, x0, tol, int(maxit), int(check_every))
            return self.x(), its - 1
        finally:
            self.set_preconditioner(None)


class MixedInfo:
    """what MixedSolver.solve reports, per right-hand side: `iterations` (inner iterations of the segments the column was open in),
    `resnorm` (sqrt|r.r| of the TRUE fp64 / complex128 residual of the x returned), `status` (0 reached the tolerance, 1 the budget ran
    out, 2 a non-finite residual), `scales` (the power of two its residual was scaled by); `replacements`: the segments run"""

    def __init__(self, iterations, resnorm, status, replacements, scales):
        self.iterations, self.resnorm, self.status, self.replacements, self.scales = iterations, resnorm, status, int(replacements), scales

    def __repr__(self):
        return (f"MixedInfo(iterations={self.iterations.tolist()}, resnorm={self.resnorm.tolist()}, status={self.status.tolist()}, "
                f"replacements={self.replacements}, scales={self.scales.tolist()})")


class MixedSolver:
    """Mixed-precision CG (cgamd_mixed_*, include/cgamd.h): the recurrence in float32 / complex64 on `.inner`, x and the true residual
    in float64 / complex128 on `.outer`, joined by residual replacement with the search direction kept -- an fp64-accurate answer at
    close to the fp32 loop's byte rate.  a_values: float64 or complex128.  flags: NO_GRAPH, MATRIX_ON_DEVICE (dtype= is then required;
    the lo copy of the values is taken at creation, a changed matrix needs a new MixedSolver).  Preconditioners go on the inner
    handle: `m.inner.set_preconditioner("jacobi")` or a diagonal; line preconditioners are refused by solve()."""

    def __init__(self, ctx, size, non_zeros, a_values, a_pointers, a_cols, n_rhs=1, flags=0, dtype=None):
        self.ctx = ctx
        self._lib = _lib.load()
        on_device = bool(int(flags) & _lib.MATRIX_ON_DEVICE)
        if not on_device:
            self.dtype = np.dtype(dtype) if dtype is not None else np.dtype(a_values.dtype)
            a_values = np.ascontiguousarray(a_values, dtype=self.dtype)
            a_pointers = np.ascontiguousarray(a_pointers, dtype=np.intc)
            a_cols = np.ascontiguousarray(a_cols, dtype=np.intc)
        else:
            if dtype is None:
                raise ValueError("dtype is required for device-resident matrices")
            self.dtype = np.dtype(dtype)
        self._keep = (a_values, a_pointers, a_cols)
        self.size, self.n_rhs, self.non_zeros = int(size), int(n_rhs), int(non_zeros)
        h = ctypes.c_void_p()
        check(self._lib.cgamd_mixed_create(ctx.handle, _lib.DTYPE_CODE[self.dtype], self.size, self.non_zeros, ptr(a_values), ptr(a_pointers),
                                           ptr(a_cols), self.n_rhs, int(flags), ctypes.byref(h)))
        self.handle = h
        lo = np.dtype(np.complex64 if self.dtype.kind == "c" else np.float32)
        self.outer = self._wrap(self._lib.cgamd_mixed_outer(h), self.dtype, on_device)
        self.inner = self._wrap(self._lib.cgamd_mixed_inner(h), lo, True)

    def _wrap(self, handle, dtype, on_device):
        s = Solver.__new__(Solver)
        s.ctx, s._lib, s.batched, s.non_zeros, s._on_device, s.dtype = self.ctx, self._lib, False, self.non_zeros, on_device, dtype
        s._keep, s.size, s.n_rhs, s._borrowed = (), self.size, self.n_rhs, True
        s.handle = ctypes.c_void_p(handle)
        return s

    def solve(self, b, x0=None, tol=1e-10, maxit=1000, delta=0.1, max_segment=0, check_every=8):
        """Solve to sqrt|r.r| < tol (a scalar or n_rhs values, ABSOLUTE, on the true residual) within `maxit` inner iterations; returns
        (x, MixedInfo).  delta: the drop of the inner residual after which it is replaced; max_segment: cap of a segment's iterations
        (0 = none).  The result does not depend on check_every."""
        t = np.ascontiguousarray(np.asarray(tol, dtype=np.float64).reshape(-1))
        if t.size not in (1, self.n_rhs):
            raise ValueError(f"tol must be a scalar or have n_rhs = {self.n_rhs} entries, got {t.size}")
        if not np.all(t > 0):
            raise ValueError("every tolerance must be positive")
        b = np.ascontiguousarray(np.asarray(b).reshape(-1), dtype=self.dtype)
        if b.size != self.size * self.n_rhs:
            raise ValueError(f"b holds {b.size} values, the handle takes n_rhs * size = {self.size * self.n_rhs}")
        x = np.zeros_like(b) if x0 is None else np.array(np.asarray(x0).reshape(-1), dtype=self.dtype, order="C", copy=True)
        if x.size != b.size:
            raise ValueError(f"x0 holds {x.size} values, b {b.size}")
        its, status = np.zeros(self.n_rhs, dtype=np.intc), np.zeros(self.n_rhs, dtype=np.intc)
        res, scales = np.zeros(self.n_rhs), np.zeros(self.n_rhs)
        repl = ctypes.c_int(0)
        pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        check(self._lib.cgamd_mixed_solve(self.handle, ptr(b), ptr(x), 0, t.ctypes.data_as(pd), int(t.size), int(maxit), float(delta),
                                          int(max_segment), int(check_every), its.ctypes.data_as(pi), res.ctypes.data_as(pd),
                                          status.ctypes.data_as(pi), ctypes.byref(repl)))
        check(self._lib.cgamd_mixed_scales(self.handle, scales.ctypes.data_as(pd)))
        return x, MixedInfo(its, res, status, repl.value, scales)

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self._lib.cgamd_mixed_destroy(self.handle)
        self.handle = None
        for s in (getattr(self, "outer", None), getattr(self, "inner", None)):
            if s is not None:
                s.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _shared_pattern(P):
    """(indptr, indices, stacked data) of matrices on one pattern; ValueError when an item's pattern differs from that of P[0]"""
    indptr, indices = np.asarray(P[0].indptr), np.asarray(P[0].indices)
    for p, A in enumerate(P):
        if not hasattr(A, "indptr"):
            raise ValueError(f"sub-domain matrix {p} is no CSR matrix (it has no indptr)")
        if not (np.array_equal(np.asarray(A.indptr), indptr) and np.array_equal(np.asarray(A.indices), indices)):
            raise ValueError(f"sub-domain matrix {p} does not share the sparsity pattern of matrix 0 (indptr / indices differ): a "
                             "batched handle carries ONE pattern; bring the matrices into canonical CSR form (sorted indices, "
                             "explicit zeros where one of them has an entry) or solve them on handles of their own")
    return indptr, indices, np.concatenate([np.asarray(A.data).ravel() for A in P])


def solve_subdomains(ctx, P0, residuals, n_iterations, dtype=np.csingle, solver=None, preconditioner=None, tol=None,
                     return_iterations=False, project=False):
    """The batched sub-domain solve of the reference's Additive-Schwarz preconditioner `as_prec`.

    * UseCG in {2, 3} (p_h-PY_C-CL.py:1918-1937, 1938-1953): all n_my sub-domains share ONE matrix P[0] -- P0: scipy CSR (or
      (indptr, indices, data)).  Their residuals are stacked RHS-major into one b, solved with n_rhs = n_my and a fixed number of
      iterations, and split back.
    * VarCoeff / UseCG == 4 (p_h-PY_C-CL.py:1970-1985): every sub-domain has its own P[p] on the same grid -- P0: a list or tuple
      of len(residuals) CSR matrices (items with .indptr) on ONE sparsity pattern.  Their `data` are stacked into one batched handle
      (Solver(..., batched=True)): one upload, one launch sequence for all sub-domains instead of the reference's loop of
      single-system cg() calls.  ValueError, before anything touches the device, when an item's indptr / indices differ from P[0]'s.
    residuals: list of arrays.  Pass `solver` (a Solver built for P0 with n_rhs = len(residuals); for a list of matrices a batched
    one, whose values are then reloaded from the list) to keep the allocations and the pattern resident across the outer GMRES
    iterations -- the reference re-uploads everything on every call (clcg.c:202-211).
    preconditioner (a list of matrices only): one M per sub-domain, as Solver.set_preconditioner takes it on a batched handle --
    "jacobi", ("line", stride), ("multigrid", dims[, opts]), n_my * size diagonal entries or a list of diagonal matrices.  It is set before the solve and removed
    after it, also on the caller's `solver`.  ValueError for a shared matrix or a solver that is not batched.
    tol (a scalar or one value per sub-domain): every sub-domain stops on its own, on the device, in the first iteration whose
    sqrt(|r.r|) is below its tolerance -- the reference's `CG(P[0], z[p].ravel(), tol=CGtol, maxit=CGMaxIT)` per sub-domain
    (p_h-PY_C-CL.py:1916-1921) in one batched solve (Solver.iterate_until); n_iterations is then the cap.  tol=None: exactly
    n_iterations iterations for all, as before.  ValueError for a tol of another length, before anything touches the device.
    project=True: the persistent `solver=` (required; Solver.enable_projection first) starts every sub-domain from the projection onto
    the span of its earlier solutions and updates its basis afterwards.  (A list of matrices is reloaded on every call, which clears
    the basis: the option pays for one shared matrix.)
    Returns a list of complex arrays shaped like the inputs (`x[p*size:(p+1)*size].astype(complex)`); with return_iterations=True
    the pair (that list, the iterations of every sub-domain as an int array)."""
    n_my = len(residuals)
    if project and solver is None:
        raise ValueError("solve_subdomains: project=True needs a persistent solver= (the basis lives in the handle)")
    if tol is not None:
        tol = np.ascontiguousarray(np.asarray(tol, dtype=np.float64).reshape(-1))
        if tol.size not in (1, n_my):
            raise ValueError(f"solve_subdomains: tol must be a scalar or have one entry per sub-domain ({n_my}), got {tol.size}")
        if not np.all(tol > 0):
            raise ValueError("solve_subdomains: every tolerance must be positive")
    batched = isinstance(P0, (list, tuple)) and len(P0) > 0 and hasattr(P0[0], "indptr")
    if preconditioner is not None and (not batched or (solver is not None and not getattr(solver, "batched", False))):
        raise ValueError("solve_subdomains: a preconditioner per sub-domain needs a list of sub-domain matrices and a batched Solver "
                         "(one matrix shared by all residuals: Solver.pcg, or Solver.set_preconditioner on a handle of your own)")
    if batched:
        if len(P0) != n_my:
            raise ValueError(f"{len(P0)} sub-domain matrices for {n_my} residuals")
        indptr, indices, data = _shared_pattern(P0)
        if solver is not None and not getattr(solver, "batched", False):
            raise ValueError("a list of sub-domain matrices needs a batched Solver (Solver(..., batched=True))")
    elif hasattr(P0, "indptr"):
        indptr, indices, data = P0.indptr, P0.indices, P0.data
    else:
        indptr, indices, data = P0
    size = len(indptr) - 1
    b_values = np.zeros(size * n_my, dtype=dtype)
    for p in range(n_my):
        b_values[p * size:(p + 1) * size] = np.asarray(residuals[p]).ravel()
    own = solver is None
    if own:
        solver = Solver(ctx, size, len(indices), np.asarray(data, dtype=dtype), indptr, indices, n_my, batched=batched)
    elif batched:
        solver.reload_matrix(np.asarray(data, dtype=dtype), indptr, indices)
    try:
        if preconditioner is not None:
            solver.set_preconditioner(preconditioner)
        if project:
            solver.set_rhs_projected(b_values)
        else:
            solver.set_rhs(b_values, None)
        if tol is None:
            solver.iterate(n_iterations)
            its = np.full(n_my, int(n_iterations), dtype=np.intc)
        else:
            its = solver.iterate_until(tol, n_iterations)
        x = solver.x()
        if project:
            solver.projection_update()
    finally:
        if own:
            solver.close()
        elif preconditioner is not None:
            solver.set_preconditioner(None)
    out = [x[p * size:(p + 1) * size].astype(complex).reshape(np.shape(residuals[p])) for p in range(n_my)]
    return (out, its) if return_iterations else out


# ---- reference entry points --------------------------------------------------------------------
def CG(ctx, queue, kernels, size, non_zeros, a_values, b_values, a_pointers, a_cols, x, n_rhs, n_iterations,
       device=None, return_history=False):
    """reference cl.py:44-200: exactly n_iterations iterations of (CO)CG on n_rhs right-hand sides.

    a_values/b_values/x: 1-D arrays of the value type (np.csingle at the reference's call sites),
    a_pointers/a_cols: np.intc.  b_values and x are RHS-major (element i of RHS r at i + r*size).
    x is the initial guess on input and receives the solution (cl.py:188); it is also returned.
    """
    dt = np.dtype(a_values.dtype)
    if dt not in _lib.DTYPE_CODE:
        raise TypeError(f"unsupported value type {dt}")
    if not (isinstance(x, np.ndarray) and x.dtype == dt and x.flags.c_contiguous):
        raise TypeError("x must be a C-contiguous numpy array of the matrix value type (it is filled in place)")
    s = Solver(ctx, size, non_zeros, a_values, a_pointers, a_cols, n_rhs)
    try:
        s.set_rhs(b_values, x)
        s.iterate(n_iterations)
        s.x(out=x.reshape(-1))
        hist = s.history() if return_history else None
    finally:
        s.close()
    return (x, hist) if return_history else x


_device_contexts = {}
_device_contexts_lock = threading.Lock()


def _context_on(device):
    """a cached Context on `device` (a Device or an index) -- used when a caller names a device that its ctx is not on"""
    index = device.index if isinstance(device, Device) else int(device)
    with _device_contexts_lock:
        ctx = _device_contexts.get(index)
        if ctx is None or not getattr(ctx, "handle", None):
            ctx = _device_contexts[index] = Context(index)
        return ctx


def conjugate_gradient_multi_gpu(ctx, queue, kernels, size, non_zeros, a_values, b_values, a_pointers, a_cols, x,
                                 n_rhs, n_iterations, device):
    """reference cl.py:203-360: the per-device worker of the RHS-sharded multi-GPU mode
    (p_h-PY_C-CL-multi-GPU.py:2123-2181).  Each device gets the whole matrix and a slice of the
    right-hand sides; there is no inter-GPU communication.  `device` selects where the solve runs: the reference passes
    the device its ctx/queue were built for (multi-GPU.py:2136-2137,2160-2163); when ctx lives on another device a cached
    context on `device` is used instead.  Thread-safe per (ctx, queue): ctypes releases the GIL during the calls, every
    handle carries its own configuration snapshot and stream, so one Python thread per device runs concurrently, as in
    the reference.  (The row-partitioned RCCL solver lives in .dist.)"""
    if device is not None:
        index = device.index if isinstance(device, Device) else int(device)
        if index != ctx.device:
            ctx = _context_on(index)
    return CG(ctx, queue, kernels, size, non_zeros, a_values, b_values, a_pointers, a_cols, x, n_rhs, n_iterations,
              device=device)


def distribute_workloads_on_devices(devices, n_subdomain):
    """reference p_h-PY_C-CL-multi-GPU.py:2123-2142: split n_subdomain right-hand sides over the devices (the first
    n_subdomain % n_gpus devices take one more) and build one (ctx, queue, kernels) per device.
    -> {device: (start, end, ctx, queue, kernels)}.  `devices` may name the same physical device several times
    (distinct Device objects): each entry gets its own context, stream and thread."""
    n_gpus = len(devices)
    tasks_per_process, extra_tasks = divmod(n_subdomain, n_gpus)
    distribution, start = {}, 0
    for i in range(n_gpus):
        end = start + tasks_per_process + (1 if i < extra_tasks else 0)
        ctx, queue = initialize_cl_environment_with_device(devices[i])
        kernels = load_and_build_kernels(ctx, end - start)
        distribution[devices[i]] = (start, end, ctx, queue, kernels)
        start = end
    return distribution


def distribute_computations_with_threads(size, non_zeros, a_values, b_values, a_pointers, a_cols, x_values, n_rhs,
                                         n_iterations, workloads):
    """reference p_h-PY_C-CL-multi-GPU.py:2144-2181: one threading.Thread per workload entry; thread `dev` solves the
    right-hand sides [start, end) with the whole matrix on its device (conjugate_gradient_multi_gpu) and copies its
    slice of the solution back into x_values under a lock.  Returns x_values.  An exception in a worker is re-raised
    here after all threads have been joined (the reference lets the thread die silently)."""
    lock = threading.Lock()
    errors = []

    def worker(dev):
        try:
            start, end, ctx, queue, kernels = workloads[dev]
            if end <= start:
                return
            b = np.ascontiguousarray(b_values[start * size:end * size])
            x = np.ascontiguousarray(x_values[start * size:end * size])
            result_x = conjugate_gradient_multi_gpu(ctx, queue, kernels, size, non_zeros, a_values, b, a_pointers, a_cols, x,
                                                    end - start, n_iterations, dev)
            with lock:
                x_values[start * size:end * size] = result_x
        except BaseException as e:      # noqa: BLE001 -- reported by the joining thread
            with lock:
                errors.append(e)

    threads = [threading.Thread(target=worker, args=(dev,)) for dev in workloads]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return x_values


def solve_rhs_sharded(devices, size, non_zeros, a_values, b_values, a_pointers, a_cols, x_values, n_rhs, n_iterations):
    """The reference's multi-GPU mode in one call (`UseCG == 6`, p_h-PY_C-CL-multi-GPU.py:1934-1944): matrix replicated,
    right-hand sides sharded over `devices`, one thread each, no inter-GPU communication."""
    workloads = distribute_workloads_on_devices(devices, n_rhs)
    try:
        return distribute_computations_with_threads(size, non_zeros, a_values, b_values, a_pointers, a_cols, x_values,
                                                    n_rhs, n_iterations, workloads)
    finally:
        for _, _, ctx, _, _ in workloads.values():
            ctx.close()


def cg(size, non_zeros, a_values, b_values, a_pointers, a_cols, x, n_rhs, n_iterations, is_complex):
    """The C entry cg() (reference clcg.h:3-5) through libcgamd.so, same argument order.
    a_values/b_values/x must be float32 (or complex64 viewed as such when is_complex)."""
    lib = _lib.load()
    lib.cg(int(size), int(non_zeros), ptr(a_values), ptr(b_values), ptr(a_pointers), ptr(a_cols), ptr(x), int(n_rhs),
           int(n_iterations), int(is_complex))
    return x
