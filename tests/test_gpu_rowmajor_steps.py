"""The row-major CG loop kernel by kernel (csrc/rowmajor.hip and the row-major branches of csrc/solver.cpp) against the host restatement
tests/rowmajor_ref.py: spmm_rm_kernel with and without its fused d.q partials, rm_dot, rm_axpy_dot, rm_aypx_x, and cg_delta0 / cg_alpha /
cg_beta on the partial counts of these launches.

q = A x is NOT restated (the rounding inside the matrix-core instructions is not modelled, rowmajor_ref docstring).  It is held exactly
-- bit for bit against integer arithmetic where every product and partial sum is an integer the format holds -- and, on random values,
inside gamma_L(u) S + L 2^-63 S of the np.longdouble product, rows without entries exactly +0.  Behind q everything is BIT FOR BIT: the
d.q partials (strip -> work-group assignment, lane row order, shuffle and wave order, layout), alpha, r, the r.r partials, delta, beta,
x, d, the history row and the counter, after set_rhs and after every iteration; iterate(3) in one call (the captured path) must return
the bits of three single calls.  tests/test_rowmajor_ref.py proves on the CPU, on these very inputs, that each plausible mistake changes
a compared bit or breaks a bound.

Every case FIRST asserts Solver.rowmajor_plan() -- read from the functions and fields the launch sites read -- against the plan it is
written for (rowmajor_ref.host_plan: NH, TQ, strips, grids, NT forms, pacing), so a moved threshold cannot turn it into a test of another
instance.  The last test asserts that all 14 SpMM instances ((type, width) x TQ 5 / 8) ran with and without the fused dot.

SpMM alone (cgamd_solver_spmm_rowmajor on a handle created under spmm_rowmajor = 2, integer and random values, every (type, width)):
n = 1, 15, 16, 17, 100 (7 strips: XCDs without a strip), 129; the 5-point grid 39 x 39 (1521 rows, last strip one row, TQ 5); the 9-point
grid (quads of 36 entries: a second round of TQ 8 in every interior strip); the random pattern of 1543 rows (unsorted columns, empty rows,
an empty quad, an empty strip, quads of 32 and 33 entries, a row of 77).  The three large systems under the default grid (random: 16
waves per XCD for 12 or 13 strips -- idle waves, unpaced; the grids: 12 waves for 12 strips, one step per wave, the pacing rule at its
threshold) and under dev.spmm_wgs = 1 (4 waves per XCD, 3 or 4 steps per wave: both pipeline buffers, the clamped look-ahead loads, paced;
the random system leaves the step loop by both exits).  dev.spmm_lead -1 / 0 / 1 and dev.spmm_ynt 0 / 1 / 2 give the same bits.  Y lies
between 16 guard rows of a pattern that must come back untouched.

The loop (5-point grid and random pattern, every (type, width)): integer B without a first guess, one iteration; random B and X0, three
iterations one by one and in one call, under the default vector grid, vec_grid = 2 (more than 12 grid-stride rounds, the last one
partial) and vec_nt = 0 / 3 (both forms of the two NT kernels); n = 1 and n = 17 with 16 right-hand sides (fewer packs than a wave has
threads), one iteration.

NOT covered: the cg_alpha2 path of these launches (16384 partials need a block of more than 250 MB), the 4 GiB offset limit, NaN / Inf in
dead matrix-core slots."""
import ctypes
import time

import numpy as np
import pytest

import cg_step_ref as C
import rowmajor_ref as M
import spmv_ref as R

pytestmark = pytest.mark.gpu

IDS = [f"{dt}x{w}" for dt, w in M.WIDTHS]
SEEN = set()        # (dt, nrhs, TQ, fused) of every SpMM launch a case asserted and made
RATIOS = {}         # (dt, TQ) -> largest |q - q_exact| / bound seen on the device (DESIGN.md quotes them)
LARGE = tuple(M.SYSTEMS)


def _expected_instances():
    return {(dt, w, tq, fused) for dt, w in M.WIDTHS for tq in (5, 8) for fused in (False, True)}


class hip_guard:
    """a CGAMD_ERR_HIP ends the session: nothing more is started on a device a kernel faulted on"""
    def __init__(self, pkg, label):
        self.pkg, self.label = pkg, label

    def __enter__(self):
        return self

    def __exit__(self, et, e, tb):
        if et is not None and issubclass(et, self.pkg.CgAmdError) and e.status == self.pkg._lib.ERR_HIP:
            pytest.exit(f"HIP error in {self.label}, the session ends here: {e}", returncode=3)
        return False


def make_handle(pkg, ctx, ip, ix, da, dtype, nrhs, knobs):
    """a handle created under spmm_rowmajor = 2 and the case's knobs (a handle keeps the configuration it was created under)"""
    lib = pkg._lib.load()
    k = {"spmm_rowmajor": 2}
    k.update(knobs or {})
    try:
        for key, v in k.items():
            assert key in M.TUNE_DEFAULTS, key
            pkg._lib.check(lib.cgamd_tune(key.encode(), int(v)))
        return pkg.Solver(ctx, len(ip) - 1, len(ix), np.ascontiguousarray(da), ip, ix, nrhs, dtype=dtype)
    finally:
        for key in k:
            pkg._lib.check(lib.cgamd_tune(key.encode(), M.TUNE_DEFAULTS[key]))


def assert_plan(pkg, s, ip, dtype, nrhs, knobs, label):
    lib = pkg._lib.load()
    assert lib.cgamd_solver_layout(s.handle) == 1 and lib.cgamd_solver_loop_launches(s.handle) == 5, label
    plan, want = s.rowmajor_plan(), M.host_plan(ip, dtype, nrhs, knobs)
    assert plan == want, f"{label}: the handle launches {plan}, the case is written for {want}"
    return plan


def _note(dt, tq, ratio):
    RATIOS[dt, tq] = max(RATIOS.get((dt, tq), 0.0), float(ratio))


def _ratios():
    return ", ".join(f"{k[0]}/TQ{k[1]}={v:.3g}" for k, v in sorted(RATIOS.items()))


# ---- SpMM alone -------------------------------------------------------------------------------------------------------------------------------
def guard_pattern(rows, rc_values, dtype):
    v = (np.arange(rows * rc_values) % 251 + 1000).astype(R.real_type(dtype))
    return R._join(v, -v, dtype) if R.is_complex(dtype) else v.astype(dtype)


def device_spmm(pkg, ctx, s, X, dtype, nrhs, label):
    """Y = A X through cgamd_solver_spmm_rowmajor: X (nrhs, n) -> (nrhs, n); 16 guard rows before and after Y must stay what they were"""
    n = X.shape[1]
    g = 16 * nrhs
    xb = pkg.DeviceBuffer(ctx, hostbuf=np.ascontiguousarray(X.T))
    fill = guard_pattern(n + 32, nrhs, dtype)
    yb = pkg.DeviceBuffer(ctx, hostbuf=fill)
    try:
        s.spmm_rowmajor(xb, int(yb.ptr) + g * np.dtype(dtype).itemsize, nrhs)
        got = yb.get()
    finally:
        xb.release()
        yb.release()
    assert R.bit_equal(got[:g], fill[:g]) and R.bit_equal(got[g + n * nrhs:], fill[g + n * nrhs:]), f"{label}: the SpMM wrote outside Y"
    return np.ascontiguousarray(got[g:g + n * nrhs].reshape(n, nrhs).T)


SPMM_CASES = [(str(n), {}) for n in M.SMALL_N] + [(name, k) for name in LARGE for k in ({}, {"dev.spmm_wgs": 1})]


@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
@pytest.mark.parametrize("name,knobs", SPMM_CASES, ids=[n + ("-wgs1" if k else "") for n, k in SPMM_CASES])
def test_spmm_alone(pkg, gpu, name, knobs, dt, nrhs):
    ctx, queue, kernels = gpu
    dtype = M.DT[dt]
    label = f"spmm {name} {dt}x{nrhs} {knobs}"
    t0 = time.time()
    with hip_guard(pkg, label):
        for kind, check in (("int", M.check_q_exact), ("rand", M.check_q_bound)):
            ip, ix, da, X = M.spmm_inputs(name, dt, nrhs, kind)
            n = len(ip) - 1
            s = make_handle(pkg, ctx, ip, ix, da, dtype, nrhs, knobs)
            try:
                s.set_rhs(np.zeros(n * nrhs, dtype), None)          # the handle is row-major from its first set_rhs on
                plan = assert_plan(pkg, s, ip, dtype, nrhs, knobs, label)
                got = device_spmm(pkg, ctx, s, X, dtype, nrhs, label)
                SEEN.add((dt, nrhs, plan["tq_plain"], False))
                ratio = check(got, ip, ix, da, X, dtype, f"{label} {kind}")
                if kind == "rand":
                    _note(dt, plan["tq_plain"], ratio)
            finally:
                s.close()
    print(f"{label}: {time.time() - t0:.2f} s; q error / bound so far {_ratios()}")


@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
def test_spmm_lead_and_store_policy_change_no_bit(pkg, gpu, dt, nrhs):
    """the pacing is advisory and the store policy a cache hint: on the paced sweep of the random system (dev.spmm_wgs = 1) every lead and
    every policy returns the bits of the default"""
    ctx, queue, kernels = gpu
    dtype = M.DT[dt]
    ip, ix, da, X = M.spmm_inputs("random", dt, nrhs, "rand")
    n = len(ip) - 1
    label = f"spmm knobs {dt}x{nrhs}"
    out = {}
    with hip_guard(pkg, label):
        for extra in ({}, {"dev.spmm_lead": -1}, {"dev.spmm_lead": 1}, {"dev.spmm_ynt": 0}, {"dev.spmm_ynt": 1}, {"dev.spmm_ynt": 2}):
            knobs = {"dev.spmm_wgs": 1}
            knobs.update(extra)
            s = make_handle(pkg, ctx, ip, ix, da, dtype, nrhs, knobs)
            try:
                s.set_rhs(np.zeros(n * nrhs, dtype), None)
                plan = assert_plan(pkg, s, ip, dtype, nrhs, knobs, f"{label} {extra}")
                assert plan["paced_plain"] == (0 if extra.get("dev.spmm_lead") == -1 else 8) and plan["lead"] == (1 if extra.get("dev.spmm_lead") == 1 else 3)
                out[tuple(extra.items())] = device_spmm(pkg, ctx, s, X, dtype, nrhs, f"{label} {extra}")
                SEEN.add((dt, nrhs, plan["tq_plain"], False))
            finally:
                s.close()
    base = out[()]
    _note(dt, 8, M.check_q_bound(base, ip, ix, da, X, dtype, label))
    for k, v in out.items():
        assert R.bit_equal(v, base), f"{label}: {dict(k)} changes bits of Y"


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------
def _read(pkg, ctx, s, name, n, nrhs, dtype):
    out = np.empty((n, nrhs), dtype=dtype)
    pkg._lib.check(pkg._lib.load().cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), ctypes.c_void_p(s.vector(name)), out.nbytes))
    return np.ascontiguousarray(out.T)


def device_state(pkg, ctx, s, n, nrhs, dtype, after_iteration):
    """what rowmajor_ref.RmSteps.state() names, read from the handle (vectors come back as (nrhs, n))"""
    it = s.step_state("iter")                   # (drains the handle's stream)
    out = {k: _read(pkg, ctx, s, k, n, nrhs, dtype) for k in ("x", "r", "d", "q")}
    out.update(part_rr=s.step_state("part_rr"), delta=s.step_state("delta"), iter=np.array([it]), history=s.history())
    if after_iteration:
        out.update(alpha=s.step_state("alpha"), beta=s.step_state("beta"), part_dq=s.dot_partials())
    return out


def compare(label, got, want):
    bad = []
    for k, w in want.items():
        g, w = np.asarray(got[k]), np.asarray(w)
        if R.bit_equal(g, w):
            continue
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append(f"{k}: device {g.dtype}{g.shape}, host {w.dtype}{w.shape}")
            continue
        diff = np.argwhere((R.bits(g) != R.bits(w)).reshape(w.shape + (-1,)).any(axis=-1))
        first = tuple(diff[0])
        bad.append(f"{k}: {len(diff)} of {w.size} values differ, first at {list(first)}: device {g[first]!r}, host {w[first]!r}")
    assert not bad, f"{label}:\n  " + "\n  ".join(bad)


def check_state_entries(pkg, s, plan, nrhs):
    """step_state and dot_partials serve the row-major handle with the counts of ITS launches; step_plan keeps refusing it"""
    lib = pkg._lib.load()
    assert s.step_state("part_rr").shape == (nrhs, plan["vgrid"])
    count = ctypes.c_longlong(-1)
    buf = np.zeros(4)
    for which in (1, 5):        # no r.z partials, no rho buffer
        assert lib.cgamd_solver_step_state(s.handle, which, pkg._lib.ptr(buf), 4, ctypes.byref(count)) == pkg._lib.ERR_INVALID
    out = (ctypes.c_int * 11)(*([77] * 11))
    assert lib.cgamd_solver_step_plan(s.handle, out, 11) == -pkg._lib.ERR_INVALID and list(out) == [77] * 11
    short = (ctypes.c_int * 20)(*([77] * 20))
    assert lib.cgamd_solver_rowmajor_plan(s.handle, short, 20) == 17 and list(short)[17:] == [77] * 3
    assert lib.cgamd_solver_rowmajor_plan(s.handle, short, 0) == -pkg._lib.ERR_INVALID


def run_loop(pkg, ctx, name, dt, nrhs, kind, knobs, iters, label, captured=True):
    """set_rhs and `iters` single iterations, the state compared after each; then (captured) the same from the same start in one call"""
    dtype = M.DT[dt]
    ip, ix, da, B, X0 = M.loop_inputs(name, dt, nrhs, kind)
    n = len(ip) - 1
    qcheck = M.check_q_exact if kind == "int" else M.check_q_bound
    s = make_handle(pkg, ctx, ip, ix, da, dtype, nrhs, knobs)
    try:
        bflat, xflat = B.reshape(-1), (None if X0 is None else X0.reshape(-1))
        s.set_rhs(bflat, xflat)
        plan = assert_plan(pkg, s, ip, dtype, nrhs, knobs, label)
        check_state_entries(pkg, s, plan, nrhs)
        st = M.RmSteps(dtype, nrhs, plan)
        got = device_state(pkg, ctx, s, n, nrhs, dtype, False)
        SEEN.add((dt, nrhs, plan["tq_plain"], False))
        if X0 is None:
            assert not R.bits(got["q"]).any(), f"{label}: A 0 is not +0"
        else:
            _note(dt, plan["tq_plain"], M.check_q_bound(got["q"], ip, ix, da, X0, dtype, f"{label} set_rhs"))
        st.set_rhs(B, X0, got["q"])
        compare(f"{label} after set_rhs", got, st.state())
        for k in range(iters):
            d_before = got["d"]
            s.iterate(1)
            got = device_state(pkg, ctx, s, n, nrhs, dtype, True)
            SEEN.add((dt, nrhs, plan["tq_fused"], True))
            ratio = qcheck(got["q"], ip, ix, da, d_before, dtype, f"{label} iteration {k + 1}")
            if kind == "rand":
                _note(dt, plan["tq_fused"], ratio)
            else:
                assert R.bit_equal(got["part_dq"], M.dq_integer(d_before, got["q"], dtype, plan["nwg_fused"])), \
                    f"{label}: the d.q partials differ from integer arithmetic"
            assert got["part_dq"].shape == (nrhs, plan["nwg_fused"])
            st.iterate(got["q"])
            compare(f"{label} after iteration {k + 1}", got, st.state())
        if captured and iters > 1:
            s.set_rhs(bflat, xflat)
            s.iterate(iters)
            again = device_state(pkg, ctx, s, n, nrhs, dtype, True)
            compare(f"{label} iterate({iters}) in one call against {iters} single calls", again, got)
    finally:
        s.close()


LOOP_VARIANTS = (("default", {}), ("vec_grid2", {"vec_grid": 2}), ("nt0", {"vec_nt": 0}), ("nt3", {"vec_nt": 3}))


@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
@pytest.mark.parametrize("name", ("grid5", "random"))
def test_loop_integer_values(pkg, gpu, name, dt, nrhs):
    """integer matrix and B, no first guess, one iteration: q and the d.q partials bit-equal to integer arithmetic, the rest restated"""
    ctx, queue, kernels = gpu
    label = f"loop int {name} {dt}x{nrhs}"
    t0 = time.time()
    with hip_guard(pkg, label):
        run_loop(pkg, ctx, name, dt, nrhs, "int", {}, 1, label)
    print(f"{label}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("dt,nrhs", M.WIDTHS, ids=IDS)
@pytest.mark.parametrize("variant,knobs", LOOP_VARIANTS, ids=[v for v, _ in LOOP_VARIANTS])
@pytest.mark.parametrize("name", ("grid5", "random"))
def test_loop_random_values(pkg, gpu, name, variant, knobs, dt, nrhs):
    """random matrix, B and X0: set_rhs and three iterations one by one, then iterate(3) in one call (the captured path)"""
    ctx, queue, kernels = gpu
    label = f"loop rand {name} {variant} {dt}x{nrhs}"
    t0 = time.time()
    with hip_guard(pkg, label):
        run_loop(pkg, ctx, name, dt, nrhs, "rand", knobs, 3, label)
    print(f"{label}: {time.time() - t0:.2f} s; q error / bound so far {_ratios()}")


@pytest.mark.parametrize("dt", list(M.DT))
@pytest.mark.parametrize("n", (1, 17))
def test_loop_fewer_packs_than_a_wave_has_threads(pkg, gpu, n, dt):
    """n = 1 and n = 17 with 16 right-hand sides: 4 to 136 packs in one work-group, one iteration"""
    ctx, queue, kernels = gpu
    label = f"loop small n={n} {dt}x16"
    with hip_guard(pkg, label):
        run_loop(pkg, ctx, str(n), dt, 16, "rand", {}, 1, label)


def test_rowmajor_plan_refuses_a_handle_that_is_not_row_major(pkg, gpu):
    ctx, queue, kernels = gpu
    lib = pkg._lib.load()
    ip, ix, da = C.chain_matrix(1000, np.float64)
    s = pkg.Solver(ctx, 1000, len(ix), da, ip, ix, 16)          # default knob: a small fp64 x 16 system keeps the RHS-major loops
    try:
        s.set_rhs(np.ones(16000), None)
        assert lib.cgamd_solver_layout(s.handle) == 0
        out = (ctypes.c_int * 17)(*([77] * 17))
        assert lib.cgamd_solver_rowmajor_plan(s.handle, out, 17) == -pkg._lib.ERR_INVALID and b"rowmajor_plan" in lib.cgamd_last_error()
        assert list(out) == [77] * 17
        assert s.step_plan()["n"] == 1000          # and step_plan / step_state describe it as before
    finally:
        s.close()


def test_every_instance_ran_with_and_without_the_fused_dot():
    """(type, width) x TQ 5 / 8 x (plain, fused): the 28 pairs, each asserted by the plan of the case that launched it"""
    print("q error / bound, largest per (type, TQ): " + _ratios())
    missing = _expected_instances() - SEEN
    assert not missing and len(SEEN) == 28, f"not launched in this session (the test needs the whole module): {sorted(missing)}"
