"""The vector and scalar steps of the launched CG / Jacobi-PCG loops (csrc/vector.hip, csrc/reduce_device.h) against the host
restatement tests/cg_step_ref.py, BIT FOR BIT: after set_rhs and after every iterate(1) the vectors x, r, d, q, the d.q / r.r / r.z
partial arrays, alpha, beta, delta, the rho parity buffer, the iteration counter and the history row.  The SpMV and its d.q partials
are spmv_ref's (test_gpu_spmv_forms.py checks them on their own); everything else of an iteration is restated in cg_step_ref.

Every case FIRST asserts Solver.step_plan() -- read from the fields the launch sites read -- and cgamd_solver_loop_launches against the
plan the case is written for (cg_step_ref.host_plan), so a threshold that moves cannot turn it into a test of another path.  Every
partial, every sum and (real types) alpha is also held to the bounds derived in cg_step_ref's docstring against np.longdouble; the
second bound of a partial -- against the T-rounded products -- is what shows that accumulation is in double.  No tolerance appears
here: comparisons with the restatement are spmv_ref.bit_equal, and the bounds come from the number formats.

tests/test_cg_step_ref.py proves on the CPU, on these very inputs (cg_step_ref.cases(): same generators, same seeds), that each
plausible mistake -- another order of the wave sums, of the lanes, of the prologue sums, of pack values and tail, accumulation in T,
an unrounded d.q, textbook complex division, a one-pass cg_alpha2, a contracted multiply-add in any element-wise expression --
changes a compared bit.

Groups (cg_step_ref.cases): edges (pack and tail edges, appended rows, pad_rows = 0, the scalar form), stride (grid-stride rounds),
loops (folded three-launch, four-launch, UNFUSED eight-launch, NO_GRAPH, two-launch), lag (a captured group of the deferred x update, compared
after iterate(8)), pcg (shared M; a batched handle with M per system), wide (member-blocked prologue sums, launched loop forced),
fold (2048 / 2049 d.q partials), unrolled (9221 partials: the 8-loads-in-flight branch of sum_partials_block), alpha2 (16384 /
16391 partials).

The two-launch loop is restated too (cg_step_ref.Steps._two_launch: beta and d = beta d + r at the head of the SpMV launch).

NOT covered here: the tridiagonal ZV form (its
partials come from the sweep kernels of precond.hip); the GUARD instantiations (tied to the unguarded bits by test_gpu_until.py); the
row-major rm_* kernels (test_gpu_rowmajor_steps.py restates them); the resident and distributed loops (tied to the launched loops form against form by their own modules)."""
import ctypes
import time

import numpy as np
import pytest

import cg_step_ref as C
import spmv_ref as R

pytestmark = pytest.mark.gpu

CASES = C.cases()
ONE_LANE = {"rowblock", "vc", "vcp", "spmm", "batched", "rowcode"}      # SpMV families spmv_ref.spmv_in_type restates exactly
RATIOS = {}      # (row, dt, what) -> largest error / bound seen on the device (DESIGN.md section 2 quotes them per row of its table)


def _row(case):
    """the row of the DESIGN table a case belongs to: its group, the loops by the launches they make"""
    if case["group"] != "loops":
        return case["group"]
    if case.get("two"):
        return "loops_two"
    if C.UNFUSED in case["flags"]:
        return "loops_unfused"
    if C.NO_GRAPH in case["flags"]:
        return "loops_nograph"
    return "loops_four" if case["knobs"].get("dev.no_fold_alpha") else "loops_three"


def _note(case, what, value):
    key = (_row(case), case["dt"], what)
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def _read(pkg, ctx, s, name, shape, dtype):
    out = np.empty(shape, dtype=dtype)
    pkg._lib.check(pkg._lib.load().cgamd_memcpy_d2h(ctx.handle, pkg._lib.ptr(out), ctypes.c_void_p(s.vector(name)), out.nbytes))
    return out


def device_state(pkg, ctx, s, plan, dtype, nrhs, pcg, after_iteration, unfused):
    """what cg_step_ref.Steps.state() names, read from the handle"""
    it = s.step_state("iter")                   # (drains the handle's stream)
    shape = (nrhs, plan["ld"])
    out = {k: _read(pkg, ctx, s, k, shape, dtype) for k in ("x", "r", "d", "q")}
    out.update(part_rr=s.step_state("part_rr"), delta=s.step_state("delta"), iter=np.array([it]), history=s.history())
    if pcg:
        out.update(part_rz=s.step_state("part_rz"), rho2=s.step_state("rho2"))
    if after_iteration:
        out.update(alpha=s.step_state("alpha"), beta=s.step_state("beta"))
        if not unfused:
            out["part_dq"] = s.dot_partials()
    return out


def compare(case, label, got, want):
    """bit equality of everything the restatement names (rho2: the slots written so far)"""
    bad = []
    for k, w in want.items():
        g, w = np.asarray(got[k]), np.asarray(w)
        if k == "rho2" and int(want["iter"][0]) == 0:
            g, w = g[:1], w[:1]
        if R.bit_equal(g, w):
            continue
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append(f"{k}: device {g.dtype}{g.shape}, host {w.dtype}{w.shape}")
            continue
        diff = np.argwhere((R.bits(g) != R.bits(w)).reshape(w.shape + (-1,)).any(axis=-1))
        first = tuple(diff[0])
        bad.append(f"{k}: {len(diff)} of {w.size} values differ, first at {list(first)}: device {g[first]!r}, host {w[first]!r}")
    assert not bad, f"{case['id']} {label}:\n  " + "\n  ".join(bad)


def bounds(case, plan, dtype, prev, got, pcg, unfused, m):
    """every partial, sum and (real types) alpha of the DEVICE inside the derived bounds"""
    E = C.pack_values(dtype)
    cid = case["id"]
    a, b = C.check_partials(got["part_rr"], got["r"], got["r"], dtype, plan["vgrid"], E, plan["vec"], cid + " r.r")
    _note(case, "partial/exact products", a)
    _note(case, "partial/rounded products", b)
    if pcg:
        with np.errstate(all="ignore"):
            z = R._join(*R.vmul_t(R._parts(m, dtype), R._parts(got["r"], dtype), dtype), dtype)
        a, b = C.check_partials(got["part_rz"], got["r"], z, dtype, plan["vgrid"], E, plan["vec"], cid + " r.z")
        _note(case, "partial/exact products", a)
        _note(case, "partial/rounded products", b)
        _note(case, "sum", C.check_sum(got["delta"], got["part_rz"], dtype, cid + " rho"))
    _note(case, "sum", C.check_sum(got["history"][-1], got["part_rr"], dtype, cid + " r.r sum"))
    if prev is not None and "part_dq" in got:
        d = got["d"] if case.get("two") else prev["d"]       # the direction q was formed from (two-launch loop: updated in that launch)
        a, b = C.check_partials(got["part_dq"], d, got["q"], dtype, plan["n_partials"], 1, False, cid + " d.q")
        _note(case, "partial/exact products", a)
        _note(case, "partial/rounded products", b)
        if not R.is_complex(dtype):
            _note(case, "alpha", C.check_alpha(got["alpha"], prev["delta"], got["part_dq"], dtype, cid + " alpha"))


def make_handle(pkg, ctx, case, inp):
    """the handle of a case, created under its knobs (a handle keeps the configuration it was created under); the knobs are restored"""
    lib = pkg._lib.load()
    dtype, nrhs = C.DT[case["dt"]], case["nrhs"]
    flags = 0
    for f in case["flags"]:
        flags |= getattr(pkg._lib, f)
    for k, v in case["knobs"].items():
        assert k in C.TUNE_DEFAULTS, k
        pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))
    try:
        batched = case.get("jacobi") == "systems"
        da = np.ascontiguousarray(inp["da"].reshape(-1))
        s = pkg.Solver(ctx, case["n"], len(inp["ix"]), da, inp["ip"], inp["ix"], nrhs, flags=flags, dtype=dtype, batched=batched)
        if inp["m"] is not None:
            s.set_preconditioner(inp["m"] if batched else inp["m"][0])
        return s
    finally:
        for k in case["knobs"]:
            pkg._lib.check(lib.cgamd_tune(k.encode(), C.TUNE_DEFAULTS[k]))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_steps_bit_for_bit(pkg, gpu, case):
    ctx, queue, kernels = gpu
    lib = pkg._lib.load()
    t0 = time.time()
    dtype, nrhs, n = C.DT[case["dt"]], case["nrhs"], case["n"]
    pcg, unfused = bool(case.get("jacobi")), C.UNFUSED in case["flags"]
    inp = C.case_inputs(n, dtype, nrhs, case["seed"], x0=case["x0"], jacobi=case.get("jacobi"))
    s = make_handle(pkg, ctx, case, inp)
    try:
        # ---- the plan record first: the case tests the path it is written for, or fails
        plan, want = s.step_plan(), C.host_plan(case)
        if case.get("wide"):       # rows per thread of the chip-wide loop are the plan's to choose (4 or 8): K = 2 rows-per-thread blocks
            assert plan["kdq"] in (8, 16), f"{case['id']}: the handle does not sum in the member-blocked order: {plan}"
            want.update(kdq=plan["kdq"], krr=plan["kdq"] // C.pack_values(dtype))
        assert {k: plan[k] for k in want} == want, f"{case['id']}: the handle launches {plan}, the case is written for {want}"
        assert 0 <= plan["vec_nt"] <= 7
        assert lib.cgamd_solver_loop_launches(s.handle) == C.host_launches(case)
        assert lib.cgamd_solver_x_lag(s.handle) == want["x_lag"]
        # ---- host side on the device's plan
        nt = plan["n"]
        m = None if inp["m"] is None else C.pad_vectors(inp["m"], inp["m"].shape[0], n, nt)
        st = C.Steps(C.pad_system(inp["ip"], nt), inp["ix"], inp["da"], dtype, nrhs, plan, m=m, unfused=unfused, two=bool(case.get("two")))
        mfull = None if m is None else np.broadcast_to(m, (nrhs, nt))
        # ---- set_rhs
        try:
            s.set_rhs(inp["B"].reshape(-1), None if inp["X0"] is None else inp["X0"].reshape(-1))
            form = s.last_spmv_form()
            assert form["family"] in ONE_LANE and form["fused"] == 0, form
            got = device_state(pkg, ctx, s, plan, dtype, nrhs, pcg, False, unfused)
            st.set_rhs(C.pad_vectors(inp["B"], nrhs, n, nt), None if inp["X0"] is None else C.pad_vectors(inp["X0"], nrhs, n, nt))
            compare(case, "after set_rhs", got, st.state())
            bounds(case, plan, dtype, None, got, pcg, unfused, mfull)
            # ---- iterations
            calls = [case["iters"]] if case.get("at_end") else [1] * case["iters"]
            for k, count in enumerate(calls):
                prev = got
                s.iterate(count)
                if not case.get("two"):        # (the SpMV of the two-launch loop is spmv_fused_kernel, one lane per row by construction)
                    form = s.last_spmv_form()
                    assert form["family"] in ONE_LANE and form["fused"] == (0 if unfused else 1), form
                    assert unfused or form["partials"] == plan["n_partials"], form
                got = device_state(pkg, ctx, s, plan, dtype, nrhs, pcg, True, unfused)
                st.iterate(count)
                compare(case, f"after iteration {st.it}", got, st.state())
                bounds(case, plan, dtype, prev if count == 1 else None, got, pcg, unfused, mfull)
        except pkg.CgAmdError as e:
            if e.status == pkg._lib.ERR_HIP:       # a kernel faulted: nothing more is started on that device in this session
                pytest.exit(f"HIP error in {case['id']}, the session ends here: {e}", returncode=3)
            raise
    finally:
        s.close()
    print(f"{case['id']}: {time.time() - t0:.2f} s; ratios so far " + ", ".join(f"{k[0]}/{k[1]}/{k[2]}={v:.3g}" for k, v in RATIOS.items()
                                                                                 if k[:2] == (_row(case), case["dt"])))


def test_entries_refuse_bad_arguments_on_a_live_handle(pkg, gpu):
    """the two record entries on a live handle: counts, capacities, an unknown `which`, and no r.z partials without a preconditioner"""
    ctx, queue, kernels = gpu
    lib = pkg._lib.load()
    ip, ix, da = C.chain_matrix(1000, np.float64)
    s = pkg.Solver(ctx, 1000, len(ix), da, ip, ix, 2)
    try:
        s.set_rhs(np.ones(2000), None)
        plan = (ctypes.c_int * 16)(*([77] * 16))
        assert lib.cgamd_solver_step_plan(s.handle, plan, 16) == 11 and list(plan)[11:] == [77] * 5 and plan[0] == 1000
        assert lib.cgamd_solver_step_plan(s.handle, plan, 0) == -1
        count = ctypes.c_longlong(0)
        buf = np.zeros(8)
        assert lib.cgamd_solver_step_state(s.handle, 4, pkg._lib.ptr(buf), 1, ctypes.byref(count)) == 1 and count.value == 2 and not buf.any()
        assert lib.cgamd_solver_step_state(s.handle, 7, pkg._lib.ptr(buf), 8, ctypes.byref(count)) == 1
        assert lib.cgamd_solver_step_state(s.handle, 1, pkg._lib.ptr(buf), 8, ctypes.byref(count)) == 1 and b"step_state" in lib.cgamd_last_error()
        assert s.step_state("iter") == 0 and s.step_state("delta").shape == (2,)
        assert R.bit_equal(s.step_state("delta"), s.history()[0])
    finally:
        s.close()


def test_entries_refuse_a_tridiagonal_handle(pkg, gpu):
    """a handle that runs the tridiagonal preconditioner launches its steps with grids of its own: neither entry describes it"""
    ctx, queue, kernels = gpu
    lib = pkg._lib.load()
    ip, ix, da = C.chain_matrix(1000, np.float64)
    s = pkg.Solver(ctx, 1000, len(ix), da, ip, ix, 1)
    try:
        s.set_preconditioner(("line", 1))
        s.set_rhs(np.ones(1000), None)
        plan = (ctypes.c_int * 11)(*([77] * 11))
        assert lib.cgamd_solver_step_plan(s.handle, plan, 11) == -1 and b"step_plan" in lib.cgamd_last_error() and list(plan) == [77] * 11
        count = ctypes.c_longlong(5)
        buf = np.zeros(8)
        assert lib.cgamd_solver_step_state(s.handle, 0, pkg._lib.ptr(buf), 8, ctypes.byref(count)) == 1
        assert b"step_state" in lib.cgamd_last_error() and count.value == 5 and not buf.any()
        s.set_preconditioner(None)          # plain CG again: recorded again
        s.set_rhs(np.ones(1000), None)
        assert s.step_plan()["n"] == 1000 and s.step_state("iter") == 0
    finally:
        s.close()
