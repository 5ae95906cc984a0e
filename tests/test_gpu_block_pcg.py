"""Preconditioned block CG on the GPU (cgamd_solver_set_block_pcg, csrc/block_pcg.hip): the shared Krylov space with an M in force.

Systems (tests/block_pcg_cases.py): A = D^1/2 L D^1/2 on 33 x 29 (957 rows, padded inside the handle) and 64 x 64, D = 10^u with u
uniform in [0, 2], s in {2, 9, 16} right-hand sides (default_rng(11)), float32 and float64.  The reference is tests/block_pcg_ref.py
(the recurrence in numpy with the kernels' own orders, itself held to separate PCG solves by tests/test_block_pcg_ref.py), on the
matrix, the right-hand sides and 1 / diag(A) AS ROUNDED to the handle's type.

JACOBI, ten iterations.  The yardstick is test_gpu_block.py's: the restatement run in float32 against itself run in float64, row by
row: D_k = max_j |delta_k[j] - delta64_k[j]| / delta64_k[j] and D_X = max_j |x_j - x64_j|_2 / |x64_j|_2; the GPU is within 4 D_k of the
float64 run in every history row and within 4 D_X in X.  float64: every delta_k within 1e-10 relative, X within 1e-9.
Measured D_k (float32, k = 0 .. 10; the smallest and the largest row of every case) and D_X:
    33 x 29  s =  2   D_k 2.5e-08 .. 2.7e-07   D_X 1.7e-07        64 x 64  s =  2   D_k 2.7e-08 .. 5.4e-07   D_X 1.5e-07
    33 x 29  s =  9   D_k 1.9e-08 .. 5.9e-07   D_X 2.9e-07        64 x 64  s =  9   D_k 5.6e-08 .. 4.6e-07   D_X 2.2e-07
    33 x 29  s = 16   D_k 3.2e-08 .. 8.5e-07   D_X 4.5e-07        64 x 64  s = 16   D_k 5.6e-08 .. 8.3e-07   D_X 3.0e-07
(measured on the MI355X, the GPU's error against the float64 run is D_k itself in every row of every case (ratio 1.0) and D_X in X:
its sums run in the restatement's order and 1 / diag(A) is formed as the host forms it; in float64 its history and X equal the
restatement's exactly, D_k = D_X = 0.)
Bits: a second run, iterate(3); iterate(7), CGAMD_NO_GRAPH, iterate_until with check_every 1 against 8; loop_launches == 7.

MULTIGRID, AMG, LINE: a stepped replay.  Three iterations on the handle; the same three driven from the development entries -- the
SpMV accessor, cgamd_block_gram, _update_xw, cgamd_solver_mg_apply (the line sweep: one set_rhs of a scratch handle, whose z0 lands in
d) and _update_qp_z, the small steps from block_pcg_ref -- and X, Q, P and the history bit for bit equal.  The loop is exactly the
composition of its parts; the V-cycle has bit tests of its own.

TOLERANCES (float32 1e-4 |b_j|, float64 1e-8 |b_j|; the cases of block_pcg_cases.TOL_CASES): all columns stop in the first iteration
in which each meets its own, read off the handle's history; the count is the restatement's, +-1; the true residual (float64 on the
host) is at most 2 tol |b_j| (test_block_pcg_ref.py confirms that the restatement alone meets it in every case); and in the cases
of block_pcg_cases.AHEAD -- on this system all of TOL_CASES: Jacobi at s = 2, 9, 16 on both grids, multigrid at s = 9 on both grids,
line at s = 2 on 33 x 29, where the restatement is ahead of the slowest separate PCG solve by 7 to 123 iterations -- solve_block_pcg
needs strictly fewer iterations than the slowest column of the same handle's scalar PCG solve_until.
Then: a duplicated column breaks down in set_rhs (status 2, iteration 0) and solve_block_pcg falls back; on = 0 gives the bits of a
scalar PCG handle that never had it; the refusals, both directions; refresh_values keeps the mode and rebuilds M.
Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import block_pcg_cases as C
import block_pcg_ref as BP
import block_ref as B

pytestmark = pytest.mark.gpu

BLOCKS = (2, 9, 16)
ITERS = 10
JACOBI = [(g, s, d) for g in C.GRIDS for s in BLOCKS for d in C.DTYPES]
JACOBI_IDS = [f"{g}-s{s}-{np.dtype(d).name}" for g, s, d in JACOBI]
REPLAY = [(k, g, s, d) for k, g in (("multigrid", "33x29"), ("multigrid", "64x64"), ("amg", "33x29"), ("line", "33x29")) for s in (2, 9) for d in C.DTYPES]
TOLS = [(k, g, s, d) for k, g, s in C.TOL_CASES for d in C.DTYPES]

_REF = {}


def ids(cases):
    return [f"{k}-{g}-s{s}-{np.dtype(d).name}" for k, g, s, d in cases]


def precond(kind, name):
    """what Solver.set_preconditioner takes"""
    return {"jacobi": "jacobi", "amg": "amg", "line": ("line", 1), "multigrid": ("multigrid", C.GRIDS[name] + (1,))}[kind]


def make(pkg, ctx, name, dtype, s, kind=None, flags=0, scale=1.0):
    A = C.system(name, dtype)
    sv = pkg.Solver(ctx, A.shape[0], A.nnz, (scale * A.data).astype(dtype), A.indptr, A.indices, s, flags=flags)
    if kind:
        sv.set_preconditioner(precond(kind, name))
    return sv


def dev(b):
    """(n, s) -> the handle's RHS-major block"""
    return np.ascontiguousarray(b.T).reshape(-1)


def run(s, b, pieces=(ITERS,)):
    s.set_rhs(dev(b))
    for k in pieces:
        s.iterate(k)
    return s.x().reshape(s.n_rhs, -1).T.copy(), s.history()


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int(np.count_nonzero(a != b))} values differ"


def true_residual(name, dtype, b, x, scale=1.0):
    b64, x64 = b.astype(np.float64), x.astype(np.float64)
    return np.linalg.norm(b64 - scale * (C.system(name, dtype) @ x64), axis=0) / np.linalg.norm(b64, axis=0)


def ref(kind, name, s, dtype, wide=False, tol=None):
    """block_pcg_ref.bpcg once per case: ITERS iterations (tol None) or to the tolerance; wide: the same inputs in float64"""
    dtype = np.dtype(dtype)
    key = (kind, name, s, dtype.name, wide, tol)
    if key not in _REF:
        b = C.rhs(name, s, dtype)
        run_in = np.dtype(np.float64) if wide else dtype
        M = C.host_precond(kind, name, dtype)
        if wide:
            M = M.astype(np.float64)      # (Jacobi only: the same diagonal, carried in float64)
        nb = np.linalg.norm(b.astype(np.float64), axis=0)
        _REF[key] = BP.bpcg(C.system(name, dtype), b.astype(run_in), M, tol=None if tol is None else tol * nb, maxit=ITERS if tol is None else 400,
                            dtype=run_in)
    return _REF[key]


@pytest.mark.parametrize("name,s,dtype", JACOBI, ids=JACOBI_IDS)
def test_jacobi_ten_iterations_against_the_restatement_and_the_bits(pkg, gpu, name, s, dtype):
    ctx, L = gpu[0], pkg._lib
    dtype = np.dtype(dtype)
    b = C.rhs(name, s, dtype)
    nb = np.linalg.norm(b.astype(np.float64), axis=0)
    sv = make(pkg, ctx, name, dtype, s, "jacobi")
    ng = make(pkg, ctx, name, dtype, s, "jacobi", flags=L.NO_GRAPH)
    try:
        sv.set_block_pcg(True)
        ng.set_block_pcg(True)
        assert L.load().cgamd_solver_loop_launches(sv.handle) == 7
        x, h = run(sv, b)
        assert h.shape == (ITERS + 1, s) and sv.iterations_done() == ITERS
        narrow, wide = ref("jacobi", name, s, dtype), ref("jacobi", name, s, dtype, wide=True)
        hw = wide["history"]
        Dk = np.max(np.abs(narrow["history"].astype(np.float64) - hw) / hw, axis=1)
        DX = np.max(np.linalg.norm(narrow["X"].astype(np.float64) - wide["X"], axis=0) / np.linalg.norm(wide["X"], axis=0))
        eh = np.max(np.abs(h.astype(np.float64) - hw) / hw, axis=1)
        ex = np.max(np.linalg.norm(x.astype(np.float64) - wide["X"], axis=0) / np.linalg.norm(wide["X"], axis=0))
        print(name, s, dtype.name, "D_k", Dk.min(), "..", Dk.max(), "D_X", DX, "| GPU history", eh.max(), "worst ratio",
              np.max(eh / Dk) if dtype.itemsize == 4 else "-", "x", ex)
        if dtype.itemsize == 4:
            assert np.all(eh <= 4 * Dk), (eh, Dk)
            assert ex <= 4 * DX
        else:
            assert eh.max() < 1e-10 and ex < 1e-9
        st = sv.block_status()
        assert (st["on"], st["preconditioned"], st["status"], st["s"]) == (True, True, 0, s) and st["min_pivot_ratio"] > 0.1
        x2, h2 = run(sv, b)
        same(x2, x, "a second run: x"); same(h2, h, "a second run: history")
        x3, h3 = run(sv, b, pieces=(3, 7))
        same(x3, x, "iterate(3); iterate(7): x"); same(h3, h, "iterate(3); iterate(7): history")
        x4, h4 = run(ng, b)
        same(x4, x, "CGAMD_NO_GRAPH: x"); same(h4, h, "CGAMD_NO_GRAPH: history")
        # iterate_until: a tolerance the ten iterations do not reach, so both runs go their ten; then one they do reach
        got = {}
        for ce in (1, 8):
            sv.set_rhs(dev(b))
            its = sv.iterate_until(1e-30 * nb, ITERS, ce)
            got[ce] = (its.copy(), sv.x().reshape(s, -1).T.copy(), sv.history())
        assert np.all(got[1][0] == ITERS) and np.all(got[8][0] == ITERS)
        for ce in (1, 8):
            same(got[ce][1], x, f"iterate_until, check_every {ce}: x"); same(got[ce][2], h, f"iterate_until, check_every {ce}: history")
    finally:
        sv.close()
        ng.close()


def _read(pkg, ctx, sv, which):
    """one of the handle's own blocks, (s, size): the first `size` rows of every column at the handle's stride"""
    ctx.synchronize()                   # (the handle's stream is the context's)
    out = np.empty((sv.n_rhs, sv.ld), dtype=sv.dtype)
    pkg._lib.check(pkg._lib.load().cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), ctypes.c_void_p(sv.vector(which)), out.nbytes))
    return np.ascontiguousarray(out[:, :sv.size])


class Parts:
    """the development entries on host blocks (s, size): every call uploads, launches one entry and reads back"""
    def __init__(self, pkg, ctx, aux, kind):
        self.pkg, self.ctx, self.lib, self.aux, self.kind = pkg, ctx, pkg._lib.load(), aux, kind
        self.s, self.n, self.dtype = aux.n_rhs, aux.size, np.dtype(aux.dtype)
        self.code = pkg._lib.DTYPE_CODE[self.dtype]
        self.grid = self.lib.cgamd_block_gram_grid(self.n)
        self.held = []

    def up(self, a):
        buf = self.pkg.DeviceBuffer(self.ctx, hostbuf=np.ascontiguousarray(a))
        self.held.append(buf)
        return buf

    def down(self, buf, shape):
        self.ctx.synchronize()
        return buf.get().reshape(shape)

    def spmm(self, P):
        x, y = self.up(P), self.up(np.zeros_like(P))
        self.aux.spmv(x, y)
        return self.down(y, P.shape)

    def gram(self, a, b):
        part = self.up(np.full(self.s * (self.s + 1) // 2 * self.grid, np.nan))
        self.pkg._lib.check(self.lib.cgamd_block_gram(self.ctx.handle, self.code, self.n, self.n, self.s, self.up(a).ptr, self.up(b).ptr, part.ptr))
        return B.sum_partials(self.down(part, (-1, self.grid)))

    def xw(self, P, AP, X, Q, M, al):
        x, q = self.up(X), self.up(Q)
        part = self.up(np.full(self.s * (self.s + 1) // 2 * self.grid, np.nan))
        self.pkg._lib.check(self.lib.cgamd_block_update_xw(self.ctx.handle, self.code, self.n, self.n, self.s, self.up(P).ptr, self.up(AP).ptr, x.ptr, q.ptr,
                                                           self.up(M.astype(self.dtype)).ptr, self.up(al.astype(self.dtype)).ptr, part.ptr))
        return self.down(x, X.shape), self.down(q, Q.shape), B.sum_partials(self.down(part, (-1, self.grid)))

    def minv(self, W):
        if self.kind == "line":         # z0 of the scalar loop's set_rhs from x0 = 0: r0 = W exactly, p0 = z0 in d
            self.aux.set_rhs(W.reshape(-1))
            return _read(self.pkg, self.ctx, self.aux, "d")
        return self.aux.mg_apply(W.reshape(-1)).reshape(W.shape)

    def qp(self, W, P, Z, ti, tau, init):
        q, p = self.up(W), self.up(P)
        self.pkg._lib.check(self.lib.cgamd_block_update_qp_z(self.ctx.handle, self.code, self.n, self.n, self.s, q.ptr, p.ptr, self.up(Z).ptr, None,
                                                             self.up(ti.astype(self.dtype)).ptr, self.up(tau.astype(self.dtype)).ptr, int(init)))
        return self.down(q, W.shape), self.down(p, P.shape)

    def release(self):
        for buf in self.held:
            buf.release()


@pytest.mark.parametrize("kind,name,s,dtype", REPLAY, ids=ids(REPLAY))
def test_stepped_replay_bit_for_bit(pkg, gpu, kind, name, s, dtype):
    ctx, L = gpu[0], pkg._lib
    dtype = np.dtype(dtype)
    eps = B.EPS[dtype]
    b = C.rhs(name, s, dtype)
    sv, aux = make(pkg, ctx, name, dtype, s, kind), make(pkg, ctx, name, dtype, s, kind)
    parts = Parts(pkg, ctx, aux, kind)
    try:
        sv.set_block_pcg(True)
        launches = L.load().cgamd_solver_loop_launches(sv.handle)
        assert launches > 7 and launches - 7 == L.load().cgamd_solver_loop_launches(aux.handle) - (5 if kind != "line" else 3)
        x, h = run(sv, b, pieces=(3,))
        Qd, Pd = _read(pkg, ctx, sv, "r"), _read(pkg, ctx, sv, "d")
        # the same three iterations from the parts (x0 = 0: R0 = B - A 0 = B exactly)
        R0 = np.ascontiguousarray(b.T)
        X = np.zeros_like(R0)
        Z = parts.minv(R0)
        st = BP.small_w(parts.gram(R0, R0), parts.gram(R0, Z), None, s, eps)
        assert st["status"] == 0
        hist = [st["delta"].astype(dtype)]
        xi = st["xi"].tolist()
        Q, P = parts.qp(R0, R0, Z, st["tau_inv"], st["tau"], True)
        for _ in range(3):
            AP = parts.spmm(P)
            s1 = B.small1(parts.gram(P, AP), xi, s, eps)
            assert s1["status"] == 0
            X, W, dv = parts.xw(P, AP, X, Q, s1["M"], s1["alpha"])
            Z = parts.minv(W)
            s2 = BP.small_w(dv, parts.gram(W, Z), xi, s, eps)
            assert s2["status"] == 0
            hist.append(s2["delta"].astype(dtype))
            xi = s2["xi"].tolist()
            Q, P = parts.qp(W, P, Z, s2["tau_inv"], s2["tau"], False)
        same(h, np.array(hist), "history"); same(x, X.T, "X"); same(Qd, Q, "Q"); same(Pd, P, "P")
        res = true_residual(name, dtype, b, x)
        print(kind, name, s, dtype.name, "launches", launches, "residual after 3 iterations", float(res.max()))
    finally:
        parts.release()
        sv.close()
        aux.close()


@pytest.mark.parametrize("kind,name,s,dtype", TOLS, ids=ids(TOLS))
def test_tolerance_stop_and_solve_block_pcg(pkg, gpu, kind, name, s, dtype):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    tol = C.TOL[dtype]
    b = C.rhs(name, s, dtype)
    nb = np.linalg.norm(b.astype(np.float64), axis=0)
    sv = make(pkg, ctx, name, dtype, s, kind)
    try:
        sv.set_block_pcg(True)
        got = {}
        for ce in (1, 8):
            sv.set_rhs(dev(b))
            its = sv.iterate_until(tol * nb, 400, ce)
            got[ce] = (its.copy(), sv.x().copy(), sv.history())
        its, x, h = got[8]
        assert np.array_equal(got[1][0], its)
        same(got[1][1], x, "check_every 1 against 8: x"); same(got[1][2], h, "check_every 1 against 8: history")
        assert np.all(its == its[0]) and sv.iterations_done() == its[0] and h.shape[0] == its[0] + 1
        below = ~(np.sqrt(np.abs(h.astype(np.float64))) >= tol * nb)
        first = int(np.nonzero(np.all(below[1:], axis=1))[0][0]) + 1
        want = ref(kind, name, s, dtype, tol=tol)["iterations"]
        print(kind, name, s, dtype.name, "iterations", int(its[0]), "block_pcg_ref", want)
        assert its[0] == first
        assert abs(int(its[0]) - want) <= 1
        with pytest.raises(pkg._lib.CgAmdError):        # the columns have stopped: iterate() asks for set_rhs
            sv.iterate(1)
        xb, info = sv.solve_block_pcg(dev(b), None, tol=tol, maxit=400)
        res = true_residual(name, dtype, b, xb.reshape(s, -1).T)
        assert sv.block_status()["preconditioned"]
        sv.set_block_pcg(False)
        _, its_single, _ = sv.solve_until(dev(b), tol=tol * nb, maxit=400)
        print(kind, name, s, dtype.name, "solve_block_pcg", info, "residual / tol", float(np.max(res / tol)), "solve_until", its_single.tolist())
        assert info["path"] == "block" and info["status"] == 0 and info["block_iterations"] == its[0]
        same(xb, x, "solve_block_pcg against set_rhs; iterate_until")
        assert np.all(res <= 2 * tol)
        if (kind, name, s) in C.AHEAD:
            assert info["block_iterations"] < int(its_single.max())
    finally:
        sv.close()


def test_solve_block_pcg_installs_m_and_asks_for_one(pkg, gpu):
    ctx = gpu[0]
    dtype = np.dtype(np.float64)
    b = C.rhs("33x29", 4, dtype)
    sv = make(pkg, ctx, "33x29", dtype, 4)
    try:
        with pytest.raises(ValueError):
            sv.solve_block_pcg(dev(b), None)
        x1, info1 = sv.solve_block_pcg(dev(b), "jacobi", tol=1e-8)
        x2, info2 = sv.solve_block_pcg(dev(b), None, tol=1e-8)                  # the M in force
        same(x1, x2, "M given against M kept")
        with pytest.raises(ValueError):                                        # an M that is refused leaves the mode on, over the M in force
            sv.solve_block_pcg(dev(b), "no such preconditioner", tol=1e-8)
        assert sv.block_status()["preconditioned"]
        same(sv.solve_block_pcg(dev(b), None, tol=1e-8)[0], x1, "after a refused M")
        x3, info3 = sv.solve_block_pcg(dev(b), ("line", 1), tol=1e-8)          # replaced with the mode on: off, M, on again
        assert info1["path"] == info3["path"] == "block" and info3["block_iterations"] < info1["block_iterations"]
        assert np.all(true_residual("33x29", dtype, b, x3.reshape(4, -1).T) <= 2e-8)
    finally:
        sv.close()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_duplicate_column_breaks_down_and_solve_block_pcg_falls_back(pkg, gpu, dtype):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    tol = C.TOL[dtype]
    b = C.rhs("33x29", 4, dtype)
    b[:, 3] = b[:, 1]
    sv = make(pkg, ctx, "33x29", dtype, 4, "jacobi")
    try:
        sv.set_block_pcg(True)
        x, h = run(sv, b, pieces=(5,))
        st = sv.block_status()
        print(dtype.name, st)
        assert (st["status"], st["iteration"]) == (2, 0) and st["min_pivot_ratio"] <= 4 * B.EPS[dtype]
        assert not np.any(x) and sv.iterations_done() == 0       # frozen in set_rhs: X is x0, finite
        np.testing.assert_allclose(sv.history()[0].astype(np.float64), np.sum(b.astype(np.float64) ** 2, axis=0), rtol=1e-6)
        xb, info = sv.solve_block_pcg(dev(b), None, tol=tol, maxit=400)
        res = true_residual("33x29", dtype, b, xb.reshape(4, -1).T)
        print(dtype.name, info, "residual / tol", float(np.max(res / tol)))
        assert info["path"] == "block+columns" and info["status"] == 2 and info["breakdown_iteration"] == 0
        assert info["block_iterations"] == 0 and np.all(info["column_iterations"] > 0)
        assert np.all(np.isfinite(xb)) and np.all(res <= 2 * tol)
        assert sv.block_status()["preconditioned"]               # the mode stays on: an independent block runs it again
        b2 = C.rhs("33x29", 4, dtype)
        xb2, info2 = sv.solve_block_pcg(dev(b2), None, tol=tol, maxit=400)
        assert info2["path"] == "block" and np.all(true_residual("33x29", dtype, b2, xb2.reshape(4, -1).T) <= 2 * tol)
    finally:
        sv.close()


def _scalar(s, b, tol):
    """a scalar PCG solve of the handle: 12 iterations, then the per-column stop"""
    s.set_rhs(dev(b))
    s.iterate(12)
    out = [s.x().copy(), s.history()]
    s.set_rhs(dev(b))
    out += [s.iterate_until(tol, 400, 8).copy(), s.x().copy(), s.history()]
    return out


@pytest.mark.parametrize("kind", ("jacobi", "multigrid", "line"))
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_turned_off_the_handle_has_the_bits_of_a_scalar_pcg_handle(pkg, gpu, dtype, kind):
    ctx, lib = gpu[0], pkg._lib.load()
    dtype = np.dtype(dtype)
    b = C.rhs("33x29", 4, dtype)
    tol = C.TOL[dtype] * np.linalg.norm(b.astype(np.float64), axis=0)
    never, sv = make(pkg, ctx, "33x29", dtype, 4, kind), make(pkg, ctx, "33x29", dtype, 4, kind)
    try:
        want = _scalar(never, b, tol)
        sv.set_block_pcg(True)
        run(sv, b)
        sv.solve_block_pcg(dev(b), None, tol=C.TOL[dtype])
        V, n = dtype.itemsize, 957
        moved = sv.iter_moved_bytes
        sv.set_block_pcg(False)
        assert not sv.block_status()["on"]
        with pytest.raises(pkg._lib.CgAmdError):        # r and d held Q and P: set_rhs comes first
            sv.iterate(1)
        for u, v in zip(_scalar(sv, b, tol), want):
            same(u, v, "after set_block_pcg(False)")
        assert lib.cgamd_solver_loop_launches(sv.handle) == lib.cgamd_solver_loop_launches(never.handle)
        assert sv.iter_moved_bytes == never.iter_moved_bytes and sv.iter_bytes() == never.iter_bytes()
        if kind == "jacobi":            # 15 passes per right-hand side and m twice, the scalar loop 12 and no share in m ... per its own model
            assert moved - (never.iter_moved_bytes - 12 * n * V * 4) == 15 * n * V * 4 + 2 * n * V
        if kind == "multigrid":         # 17 against the scalar loop's 12, the V-cycle priced alike
            assert moved - never.iter_moved_bytes == 5 * n * V * 4
    finally:
        never.close()
        sv.close()


def test_refusals_both_directions(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    dtype = np.dtype(np.float64)
    A = C.system("33x29", dtype)
    b = C.rhs("33x29", 4, dtype)
    tol = 1e-8 * np.linalg.norm(b, axis=0)

    def refused(s, reason, block=b):
        t = 1e-6 * np.linalg.norm(np.abs(block).astype(np.float64), axis=0)
        before = _scalar(s, block, t)
        assert lib.cgamd_solver_set_block_pcg(s.handle, 1) == L.ERR_STATE, reason
        assert reason.encode() in lib.cgamd_last_error(), (reason, lib.cgamd_last_error())
        assert not s.block_status()["on"]
        for u, v in zip(_scalar(s, block, t), before):
            same(u, v, reason)
        s.close()

    # what set_block_pcg refuses: no preconditioner, and what set_block refuses
    refused(make(pkg, ctx, "33x29", dtype, 4), "no preconditioner")
    refused(make(pkg, ctx, "33x29", dtype, 1, "jacobi"), "2 ... 16", b[:, :1])
    refused(make(pkg, ctx, "33x29", np.float32, 17, "jacobi"), "2 ... 16", C.rhs("33x29", 17, np.float32))
    bat = pkg.Solver(ctx, 957, A.nnz, np.tile(A.data, 4), A.indptr, A.indices, 4, batched=True)
    bat.set_preconditioner("jacobi")
    refused(bat, "batched")
    sh = make(pkg, ctx, "33x29", dtype, 4)
    sh.set_shifts([0.5])
    assert lib.cgamd_solver_set_block_pcg(sh.handle, 1) == L.ERR_STATE and b"shifts" in lib.cgamd_last_error()
    sh.close()
    for ct, herm in ((np.complex64, False), (np.complex128, True)):
        cs = pkg.Solver(ctx, 957, A.nnz, (A.data + (0 if herm else 0.2j) * A.data).astype(ct), A.indptr, A.indices, 4, hermitian=herm)
        cs.set_preconditioner("jacobi")
        assert lib.cgamd_solver_set_block_pcg(cs.handle, 1) == L.ERR_STATE and b"real value types" in lib.cgamd_last_error()
        cs.close()
    # the pinned direction stays: set_block refuses a handle with a preconditioner, the preconditioner entries one with set_block on
    pre = make(pkg, ctx, "33x29", dtype, 4, "jacobi")
    assert lib.cgamd_solver_set_block(pre.handle, 1) == L.ERR_STATE and b"preconditioner" in lib.cgamd_last_error()
    pre.close()
    # the two modes exclude each other
    plain = make(pkg, ctx, "33x29", dtype, 4)
    plain.set_block(True)
    for on in (0, 1):
        assert lib.cgamd_solver_set_block_pcg(plain.handle, on) == L.ERR_STATE and b"exclude each other" in lib.cgamd_last_error()
    assert plain.block_status()["on"] and not plain.block_status()["preconditioned"]
    plain.close()
    # with the mode on: everything block CG refuses, and every set_preconditioner* entry, removal with NULL too
    sv = make(pkg, ctx, "33x29", dtype, 4, "jacobi")
    try:
        sv.set_block_pcg(True)
        sv.enable_projection(2)
        x, hist = run(sv, b)
        h, p, one = sv.handle, L.ptr, np.ones(957)
        its = ctypes.c_int()
        calls = {
            "set_block": lambda: lib.cgamd_solver_set_block(h, 1),
            "set_block off": lambda: lib.cgamd_solver_set_block(h, 0),
            "set_preconditioner": lambda: lib.cgamd_solver_set_preconditioner(h, p(one), 0),
            "set_preconditioner NULL": lambda: lib.cgamd_solver_set_preconditioner(h, None, 0),
            "set_preconditioner_tridiag": lambda: lib.cgamd_solver_set_preconditioner_tridiag(h, p(one), p(4 * one), p(one), 0),
            "set_preconditioner_tridiag_strided": lambda: lib.cgamd_solver_set_preconditioner_tridiag_strided(h, 33, p(one), p(4 * one), p(one), 0),
            "set_preconditioner_line": lambda: lib.cgamd_solver_set_preconditioner_line(h, 1),
            "set_preconditioner_jacobi": lambda: lib.cgamd_solver_set_preconditioner_jacobi(h),
            "set_preconditioner_multigrid": lambda: lib.cgamd_solver_set_preconditioner_multigrid(h, 33, 29, 1, 0, 0.0, 0),
            "set_preconditioner_amg": lambda: lib.cgamd_solver_set_preconditioner_amg(h, 0, 0.0, 0, 0.0, 0),
            "set_shifts": lambda: lib.cgamd_solver_set_shifts(h, p(np.ones(1)), 1),
            "iterate_tol": lambda: lib.cgamd_solver_iterate_tol(h, 5, 1e-3, ctypes.byref(its)),
            "replace_residual": lambda: lib.cgamd_solver_replace_residual(h, sv.vector("q")),
        }
        for who, call in calls.items():
            assert call() == L.ERR_STATE, who
            assert b"block CG is on" in lib.cgamd_last_error(), (who, lib.cgamd_last_error())
            same(sv.x().reshape(4, -1).T, x, who + ": x"); same(sv.history(), hist, who + ": history")
            st = sv.block_status()
            assert st["on"] and st["preconditioned"] and sv.iterations_done() == ITERS
        sv.iterate(2)                                   # and it goes on
        for _ in range(2):                              # the projected start only chooses x0
            sv.set_rhs_projected(dev(b))
            its_p = sv.iterate_until(tol, 400, 8)
            xp = sv.x().reshape(4, -1).T
            sv.projection_update()
            assert sv.block_status()["status"] == 0 and np.all(true_residual("33x29", dtype, b, xp) <= 2e-8)
        print("projected restart of the same right-hand sides: iterations", its_p.tolist())
    finally:
        sv.close()


@pytest.mark.parametrize("kind", ("jacobi", "multigrid"))
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
def test_refresh_values_keeps_the_mode_and_rebuilds_m(pkg, gpu, dtype, kind):
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    s, tol = 4, C.TOL[dtype]
    A = C.system("33x29", dtype)
    b = C.rhs("33x29", s, dtype)
    sv = make(pkg, ctx, "33x29", dtype, s, kind)
    fresh = make(pkg, ctx, "33x29", dtype, s, kind, scale=1.5)
    try:
        sv.set_block_pcg(True)
        run(sv, b)
        sv.refresh_values((1.5 * A.data).astype(dtype))
        st = sv.block_status()
        assert st["on"] and st["preconditioned"]
        x, info = sv.solve_block_pcg(dev(b), None, tol=tol, maxit=400)
        res = true_residual("33x29", dtype, b, x.reshape(s, -1).T, scale=1.5)
        assert info["path"] == "block" and np.all(res <= 2 * tol)
        xf, info_f = fresh.solve_block_pcg(dev(b), None, tol=tol, maxit=400)
        same(x, xf, "refreshed against a handle created with the new values")      # (an M of the OLD values would give other bits)
        assert info_f["block_iterations"] == info["block_iterations"]
    finally:
        sv.close()
        fresh.close()
