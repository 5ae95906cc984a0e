"""Solution projection on the device (include/cgamd.h "Solution projection") on the 957-row systems of tests/projection_ref.py:
the layering over cgamd_solver_set_rhs, the basis against the type-true restatement, what it is for, the ring, the state rules,
batched handles and columns that stop at different iterations."""
import ctypes

import numpy as np
import pytest

import projection_ref as PR
from conftest import ALL_DTYPES

pytestmark = pytest.mark.gpu

N = PR.NX * PR.NY
MAXIT = 4000


def make(pkg, ctx, dtype, nrhs=1, flags=0, **kw):
    ip, ix, da = PR.system(dtype)
    return pkg.Solver(ctx, N, len(ix), da, ip, ix, nrhs, flags=flags, **kw)


def device_vector(pkg, ctx, s, which):
    lib = pkg._lib.load()
    out = np.empty(s.n_rhs * s.ld, s.dtype)
    pkg._lib.check(lib.cgamd_ctx_synchronize(ctx.handle))
    pkg._lib.check(lib.cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), ctypes.c_void_p(s.vector(which)), out.nbytes))
    return out


def block(kind, ts, dtype):
    return np.stack([PR.rhs(kind, t, dtype) for t in ts])


def tols(B, dtype):
    return np.array([PR.stop_tol(b, dtype) for b in B])


def solve_projected(s, B, tol):
    """one projected solve by hand, with everything the tests read: a record in the format of projection_ref.run_sequence"""
    s.set_rhs_projected(B.reshape(-1))
    x0 = s.projection_state("x0")
    hist0 = s.history()[0].copy()
    its = s.iterate_until(tol, MAXIT)
    x = s.x().reshape(s.n_rhs, N)
    added = s.projection_update()
    cap = s._projection_capacity
    nus = s.projection_state("nu_s")
    return {"x0": x0, "x": x, "its": its, "hist0": hist0, "added": added, "count": s.projection_count(), "alpha": s.projection_state("alpha"),
            "c": s.projection_state("c"), "nu": nus[0], "s": nus[1], "W": np.stack([s.projection_state("slot", j) for j in range(cap)])}


def column(rec, r=0):
    """column r of a device record as a single-column record of the reference"""
    return {"alpha": rec["alpha"][:, r], "c": rec["c"][:, r], "s": rec["s"][r], "W": rec["W"][:, r], "added": bool(rec["added"][r])}


# ---- layering --------------------------------------------------------------------------------------------------------------------------
LAYER = [(dt, nrhs, None) for dt in ALL_DTYPES for nrhs in (1, 3)] + [(np.float64, 1, "jacobi"), (np.float64, 1, ("multigrid", (PR.NX, PR.NY)))]


@pytest.mark.parametrize("dtype,nrhs,pre", LAYER, ids=[f"{np.dtype(d).name}-{n}-{p if isinstance(p, (str, type(None))) else p[0]}" for d, n, p in LAYER])
def test_projected_set_rhs_is_set_rhs_with_the_guess(pkg, gpu, dtype, nrhs, pre):
    ctx = gpu[0]
    s = make(pkg, ctx, dtype, nrhs)
    try:
        if pre is not None:
            s.set_preconditioner(pre)
        s.enable_projection(4, 0.0)
        for t in range(2):              # two vectors held
            B = block("moving", range(t, t + nrhs), dtype)
            solve_projected(s, B, tols(B, dtype))
        assert s.projection_count() == 2
        B = block("moving", range(2, 2 + nrhs), dtype)
        s.set_rhs_projected(B.reshape(-1))
        x0 = s.projection_state("x0")
        assert np.any(x0 != 0)
        got = [device_vector(pkg, ctx, s, w) for w in ("x", "r", "d")] + [s.history()[0].copy()]
        s.set_rhs(B.reshape(-1), x0.reshape(-1))
        want = [device_vector(pkg, ctx, s, w) for w in ("x", "r", "d")] + [s.history()[0].copy()]
        for g, w, name in zip(got, want, ("x", "r", "d", "history row 0")):
            assert g.tobytes() == w.tobytes(), name
    finally:
        s.close()


# ---- the basis against the reference -----------------------------------------------------------------------------------------------------
BASIS = [("span3", np.float64), ("span3", np.float32), ("span3", np.complex64), ("moving", np.float64), ("moving", np.float32)]


@pytest.mark.parametrize("kind,dtype", BASIS, ids=[f"{k}-{np.dtype(d).name}" for k, d in BASIS])
def test_basis_follows_the_type_true_reference(pkg, gpu, kind, dtype):
    """K = 4, 9 solves.  The device's stored vectors, alpha and c against the type-true reference fed the device's own iterates, in the
    measure of projection_ref.distance; the bound is 4 times the distance between the type-true and the wide reference on the same
    sequence (both fed the CPU's iterates), measured here on the host before anything is compared.  The run for this change measured
    that reference distance at: span3 float64 1.94e-16, float32 9.00e-08, complex64 1.32e-07; moving float64 1.65e-12, float32 8.96e-04
    (moving: every vector is the small difference x - x0, so the roundings of x0 weigh more).  The device stood at 3.0e-16, 4.0e-08,
    8.1e-08, 2.6e-12 and 2.3e-05 from the type-true reference, in that order, with a defect of at most 5 eps.  |W^T A W - I| of the device's vectors, formed on the host in wide arithmetic, stays
    below 64 eps."""
    ctx = gpu[0]
    dtype = np.dtype(dtype)
    drop = PR.drop_tol(dtype) if kind == "span3" else 0.0
    true = PR.run_sequence(kind, dtype, 4, drop, 9)
    wide = PR.run_sequence(kind, dtype, 4, drop, 9, exact_order=False, work_dtype=PR.acc_type(dtype), feed=[r["x"] for r in true])
    allowed = 4 * PR.distance(true, wide)
    s = make(pkg, ctx, dtype)
    try:
        s.enable_projection(4, drop)
        dev = []
        for t in range(9):
            B = block(kind, [t], dtype)
            dev.append(solve_projected(s, B, tols(B, dtype)))
        ref = PR.run_sequence(kind, dtype, 4, drop, 9, feed=[r["x"][0] for r in dev])
        got = [column(r) for r in dev]
        far = PR.distance(got, ref)
        helper = PR.Projection(PR.system(dtype), N, 1, dtype, 4, drop)
        defect = max(helper.gram_defect(W=r["W"][:r["count"]]) for r in dev)
        print(f"{kind} {dtype.name}: device to type-true {far:.3e}, type-true to wide {allowed / 4:.3e} (allowed {allowed:.3e}); "
              f"defect / eps {defect / PR.eps(dtype):.2f}; iterations {[int(r['its'][0]) for r in dev]}")
        assert [r["added"] for r in got] == [r["added"] for r in ref]
        assert [r["count"] for r in dev] == [r["count"] for r in ref]
        assert defect < 64 * PR.eps(dtype)
        assert far <= allowed
    finally:
        s.close()


# ---- what it is for ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda d: np.dtype(d).name)
def test_span3_solves_start_converged(pkg, gpu, dtype):
    ctx = gpu[0]
    s = make(pkg, ctx, dtype)
    try:
        s.enable_projection(4, PR.drop_tol(dtype))
        for t in range(9):
            b = PR.rhs("span3", t, dtype)
            tol = PR.stop_tol(b, dtype)
            _, zero, _ = s.solve_until(b, tol=tol, maxit=MAXIT)
            _, its, hist = s.solve_until(b, tol=tol, maxit=MAXIT, project=True)
            print(np.dtype(dtype).name, "solve", t, "iterations", int(its[0]), "from zero", int(zero[0]), "history row 0 / tol^2", abs(hist[0, 0]) / tol ** 2)
            if t >= 3:
                assert 5 * int(its[0]) <= int(zero[0])
                assert abs(hist[0, 0]) <= 100 * tol ** 2
        assert s.projection_count() == 3
    finally:
        s.close()


# ---- the ring ----------------------------------------------------------------------------------------------------------------------------
def test_ring_of_two(pkg, gpu):
    ctx = gpu[0]
    dtype = np.dtype(np.float64)
    s = make(pkg, ctx, dtype)
    try:
        s.enable_projection(2, 0.0)
        slots = [s.projection_state("slot", j).copy() for j in range(2)]
        for t in range(5):
            B = block("moving", [t], dtype)
            rec = solve_projected(s, B, tols(B, dtype))
            assert rec["added"][0] and rec["count"] == min(t + 1, 2)
            now = [rec["W"][j] for j in range(2)]
            assert now[t % 2].tobytes() != slots[t % 2].tobytes()              # the slot written
            assert now[1 - t % 2].tobytes() == slots[1 - t % 2].tobytes()      # the other keeps its bits
            slots = [w.copy() for w in now]
    finally:
        s.close()


# ---- state rules -------------------------------------------------------------------------------------------------------------------------
def test_state_rules(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    dtype = np.dtype(np.float64)
    ip, ix, da = PR.system(dtype)
    s = make(pkg, ctx, dtype)
    b = PR.rhs("moving", 0, dtype)
    its = np.zeros(1, np.intc)
    t = np.array([PR.stop_tol(b, dtype)])
    until = lambda: lib.cgamd_solver_iterate_until(s.handle, 10, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, 8, its.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    try:
        assert lib.cgamd_solver_set_rhs_projected(s.handle, L.ptr(b), 0) == L.ERR_STATE      # before enable
        assert s.projection_count() == 0
        for cap, drop in ((-1, 0.0), (33, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf"))):
            assert lib.cgamd_solver_projection_enable(s.handle, cap, drop) == L.ERR_INVALID
        s.enable_projection(4, 0.0)
        s.set_rhs(b)
        s.iterate(5)
        assert lib.cgamd_solver_projection_update(s.handle, None) == L.ERR_STATE             # after a plain set_rhs
        s.set_rhs_projected(b)
        s.iterate(30)
        assert list(s.projection_update()) == [True]
        x = s.x()                                                                           # x stays readable
        assert np.all(np.isfinite(x)) and s.projection_count() == 1
        assert lib.cgamd_solver_iterate(s.handle, 1) == L.ERR_STATE                          # iterate after an update
        assert until() == L.ERR_STATE
        assert lib.cgamd_solver_projection_update(s.handle, None) == L.ERR_STATE             # a double update
        s.set_rhs(b)                                                                        # a set_rhs of either kind is next
        s.iterate(2)
        s.set_rhs_projected(b)
        s.iterate(2)
        s.projection_update()
        assert s.projection_count() == 2
        s.projection_clear()
        assert s.projection_count() == 0
        s.set_rhs_projected(b)
        assert not np.any(s.projection_state("x0"))
        s.iterate(20)
        s.projection_update()
        assert s.projection_count() == 1
        s.refresh_values(da)
        assert s.projection_count() == 0                                                    # orthonormal for the old matrix
        s.set_rhs_projected(b)
        s.iterate(20)
        s.projection_update()
        s.reload_matrix(da, ip, ix)
        assert s.projection_count() == 0
        s.set_preconditioner("jacobi")                                                      # a preconditioner does not clear it
        s.set_rhs_projected(b)
        s.iterate(20)
        s.projection_update()
        s.set_preconditioner(None)
        assert s.projection_count() == 1
        s.enable_projection(0)
        assert s.projection_count() == 0
        assert lib.cgamd_solver_set_rhs_projected(s.handle, L.ptr(b), 0) == L.ERR_STATE
    finally:
        s.close()


def test_hermitian_and_row_major_handles_are_refused(pkg, gpu):
    ctx, lib, L = gpu[0], pkg._lib.load(), pkg._lib
    h = make(pkg, ctx, np.complex64, hermitian=True)
    try:
        assert lib.cgamd_solver_projection_enable(h.handle, 4, 0.0) == L.ERR_STATE
        assert b"CGAMD_HERMITIAN" in lib.cgamd_last_error()
    finally:
        h.close()
    dtype = np.dtype(np.float64)
    L.check(lib.cgamd_tune(b"spmm_rowmajor", 2))             # fp64 x 16 keeps its right-hand sides interleaved under this knob
    try:
        rm = make(pkg, ctx, dtype, 16)
    finally:
        L.check(lib.cgamd_tune(b"spmm_rowmajor", 1))
    try:
        b = np.tile(PR.rhs("moving", 0, dtype), 16)
        rm.set_rhs(b)
        assert lib.cgamd_solver_layout(rm.handle) == 1
        rm.iterate(10)
        want = (rm.x().copy(), rm.history().copy())
        assert lib.cgamd_solver_projection_enable(rm.handle, 4, 0.0) == L.ERR_STATE
        assert lib.cgamd_solver_set_rhs_projected(rm.handle, L.ptr(b), 0) == L.ERR_STATE
        assert rm.projection_count() == 0
        rm.set_rhs(b)
        rm.iterate(10)
        assert rm.x().tobytes() == want[0].tobytes() and rm.history().tobytes() == want[1].tobytes()
    finally:
        rm.close()


# ---- batched handles -----------------------------------------------------------------------------------------------------------------------
def test_batched_handle_keeps_a_basis_per_system(pkg, gpu):
    ctx = gpu[0]
    dtype = np.dtype(np.float64)
    mats = [PR.system(dtype, scale) for scale in (1.0, 2.0, 3.0)]
    ip, ix, _ = mats[0]
    s = pkg.Solver(ctx, N, len(ix), np.concatenate([m[2] for m in mats]), ip, ix, 3, batched=True)
    try:
        s.enable_projection(3, 0.0)
        for t in range(3):
            B = block("moving", (t, t + 3, t + 6), dtype)
            rec = solve_projected(s, B, tols(B, dtype))
            assert all(rec["added"])
        helper = PR.Projection(mats, N, 3, dtype, 3, 0.0)
        defect = helper.gram_defect(W=rec["W"])
        wrong = PR.Projection(mats[::-1], N, 3, dtype, 3, 0.0).gram_defect(W=rec["W"])
        print("batched: defect / eps", defect / PR.eps(dtype), "against the other systems' matrices", wrong)
        assert defect < 64 * PR.eps(dtype)
        assert wrong > 0.5              # column 0 against 3 A: its Gram matrix is 3 I
    finally:
        s.close()


# ---- columns that stop at different iterations ---------------------------------------------------------------------------------------------
def test_update_uses_the_frozen_iterate_of_every_column(pkg, gpu):
    """three columns with tolerances 1e-2, 1e-5 and 1e-8 |b|: they stop far apart, and the update must take each column's x as
    iterate_until froze it.  The device's vectors against the type-true reference fed those iterates, within the bound of
    test_basis_follows_the_type_true_reference for the moving sequence in float64."""
    ctx = gpu[0]
    dtype = np.dtype(np.float64)
    true = PR.run_sequence("moving", dtype, 4, 0.0, 9)
    wide = PR.run_sequence("moving", dtype, 4, 0.0, 9, exact_order=False, work_dtype=PR.acc_type(dtype), feed=[r["x"] for r in true])
    allowed = 4 * PR.distance(true, wide)
    s = make(pkg, ctx, dtype, 3)
    ref = PR.Projection(PR.system(dtype), N, 3, dtype, 4, 0.0)
    try:
        s.enable_projection(4, 0.0)
        far = 0.0
        for t in range(3):
            B = block("moving", (t, t + 1, t + 2), dtype)
            tol = np.array([1e-2, 1e-5, 1e-8]) * np.linalg.norm(B, axis=1)
            rec = solve_projected(s, B, tol)
            assert rec["its"][0] < rec["its"][1] < rec["its"][2]
            ref.guess(B)
            added = ref.update(rec["x"])
            assert list(added) == list(rec["added"])
            for r in range(3):
                got = column(rec, r)
                want = {"alpha": ref.alpha[:, r], "c": ref.c[:, r], "s": ref.s[r], "W": ref.W[:, r, :N]}
                far = max(far, PR.distance([got], [want]))
        print(f"frozen iterates: device to type-true {far:.3e}, allowed {allowed:.3e}")
        assert far <= allowed
    finally:
        s.close()


# ---- the Python entries that take project=True ---------------------------------------------------------------------------------------------
def test_pcg_and_solve_subdomains_project(pkg, gpu):
    """span3 through Solver.pcg(project=True) with Jacobi and through solve_subdomains(solver=, project=True) with two sub-domains on one
    matrix: from the fourth call on the solves start converged (one iteration), and the answers solve the systems"""
    ctx = gpu[0]
    dtype = np.dtype(np.float64)
    mat = PR.system(dtype)
    s = make(pkg, ctx, dtype)
    try:
        with pytest.raises(ValueError):
            s.pcg(PR.rhs("span3", 0, dtype), x0=np.zeros(N), project=True)
        s.enable_projection(4, PR.drop_tol(dtype))
        for t in range(6):
            b = PR.rhs("span3", t, dtype)
            tol = PR.stop_tol(b, dtype)
            x, last = s.pcg(b, M="jacobi", tol=tol, maxit=MAXIT, project=True)
            assert np.linalg.norm(b - PR.matvec(mat, x[None, :])[0]) <= 10 * tol
            assert last >= 50 if t < 3 else last == 0, (t, last)
        assert s.projection_count() == 3
    finally:
        s.close()
    s2 = make(pkg, ctx, dtype, 2)
    try:
        with pytest.raises(ValueError):
            pkg.solve_subdomains(ctx, mat, [np.zeros(N)] * 2, MAXIT, dtype=dtype, project=True)      # needs a persistent solver
        s2.enable_projection(4, PR.drop_tol(dtype))
        for t in range(5):
            res = [PR.rhs("span3", t, dtype), PR.rhs("span3", t + 5, dtype)]
            tol = [PR.stop_tol(b, dtype) for b in res]
            out, its = pkg.solve_subdomains(ctx, mat, res, MAXIT, dtype=dtype, solver=s2, tol=tol, return_iterations=True, project=True)
            for b, x, t_ in zip(res, out, tol):
                assert np.linalg.norm(b - PR.matvec(mat, x.real[None, :])[0]) <= 10 * t_
            assert all(its >= 50) if t < 3 else all(its == 1), (t, its)
        assert s2.projection_count() == 3
    finally:
        s2.close()
