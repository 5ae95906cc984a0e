"""The CGAMD_SPLIT_LONG_ROWS form (csrc/long_rows.hip) on the device, against tests/long_rows_ref.py.

Every case asserts Solver.last_spmv_form() -- recorded at the launch site -- before it compares a value.  y is prefilled with NaN
inside a canary buffer (tests/canary_buffers.py) that is compared in all its bytes; the d.q partials live inside the handle and are
read through dot_partials (one per 256-row block: what the handle allocates), so they carry no guard words of their own.
SpMV results are compared BIT FOR BIT with the restatement; the loops against the CPU oracle and against the true residual formed on
the host in long double.  The small shapes reach every edge through dev.long_row_bytes and dev.long_row_segment."""
import numpy as np
import pytest

import cg_oracle
import long_rows_ref as LR
import spmv_ref as R
from canary_buffers import Embedded

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
ALL = list(DT)
DEFAULTS = {"resident": 1, "index_codes_min_mb": 32, "spmv_nt": -1, "spmv_cycle": 64, "dev.generic_spmv": 0, "dev.spmv_slice_kb": 0,
            "dev.spmv_chunk_kb": 0, "dev.long_row_bytes": 0, "dev.long_row_segment": 0}
ZEROS = dict.fromkeys(LR_FIELDS := ("heavy_blocks", "segments", "segment", "body_kind", "body_lanes", "scratch_bytes"), 0)


@pytest.fixture
def tuned(pkg):
    lib = pkg._lib.load()

    def put(kv):
        for k, v in kv.items():
            assert k in DEFAULTS, k
            pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))

    def tune(**kv):
        put(DEFAULTS)
        put({k.replace("dev_", "dev."): v for k, v in kv.items()})
    yield tune
    put(DEFAULTS)


def fit_unroll(max_row, dtype):
    if np.dtype(dtype).itemsize > 8:
        return 4
    return 8 if max_row <= 0 else 4 if max_row <= 4 else 5 if max_row == 5 else 7 if max_row <= 7 else 8


def split_form(pl, n, dtype, fused, nt=0):
    width = pl["body_lanes"] if pl["body_kind"] == 7 else fit_unroll(pl["body_max_row"], dtype) if pl["body_kind"] == 5 else 0
    return {"family": "split", "vec": 1, "width": width, "index_bits": 0, "value_codes": 0, "nt": nt, "fused": int(fused), "wide": 0,
            "grid": len(pl["regular"]), "partials": (n + 255) // 256 if fused else 0}


def want_query(pl):
    return {"heavy_blocks": len(pl["heavy"]), "segments": len(pl["segments"]), "segment": pl["segment"], "body_kind": pl["body_kind"],
            "body_lanes": pl["body_lanes"], "scratch_bytes": pl["scratch_bytes"]}


def make_solver(pkg, ctx, mat, dtype, nrhs=1, long_rows=True, misalign=False, flags=0):
    import torch
    dev = torch.device("cuda", 0)
    ip, ix, da = mat
    n = len(ip) - 1
    if not misalign:
        return pkg.Solver(ctx, n, len(ix), np.asarray(da, dtype=dtype), ip, ix, nrhs, flags=flags, dtype=dtype, long_rows=long_rows)

    def off8(a):      # 8 bytes off a 16-byte boundary: no 16-byte loads
        raw = np.concatenate([np.zeros(8, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])
        t = torch.from_numpy(raw).to(dev)
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr() + 8
    tv, pv = off8(np.asarray(da, dtype=dtype))
    tc, pc = off8(np.asarray(ix, dtype=np.int32))
    tp = torch.from_numpy(np.asarray(ip, dtype=np.int32)).to(dev)
    torch.cuda.synchronize()
    s = pkg.Solver(ctx, n, len(ix), pv, tp, pc, nrhs, flags=flags | pkg._lib.MATRIX_ON_DEVICE, dtype=dtype, long_rows=long_rows)
    s._keep = (tv, tc, tp)
    return s


def nan_rows(nrhs, n, dtype):
    v = np.full((nrhs, n), np.nan, dtype=dtype)
    return v + 1j * v if np.dtype(dtype).kind == "c" else v


def run_spmv(pkg, ctx, s, x, dtype, fused, nrhs=1):
    """one SpMV on caller vectors -> (y, form, partials or None); the canary buffer around y is checked against what came back"""
    n = x.size // nrhs
    xe = Embedded(pkg, ctx, np.ascontiguousarray(x.reshape(nrhs, n)), n)
    ye = Embedded(pkg, ctx, nan_rows(nrhs, n, dtype), n)
    try:
        s.spmv(xe.ptr, ye.ptr, fused_dot=fused)
        form = s.last_spmv_form()
        ctx.synchronize()
    except pkg.CgAmdError as e:
        if e.status == pkg._lib.ERR_HIP:
            pytest.exit(f"HIP error in an SpMV launch, the session ends here: {e}", returncode=3)
        raise
    parts = s.dot_partials() if fused else None
    raw = ye.buf.get()
    y = raw[ye.start:ye.start + nrhs * n * np.dtype(dtype).itemsize].view(dtype).reshape(nrhs, n).copy()
    ye.check("y and its guard bytes", y)
    xe.check("x")
    return y, form, parts


def assert_bits(label, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{label}: {len(bad)} words differ from the restatement, first at {bad[0].tolist()}: got {got.reshape(-1)[bad[0][-1] // (2 if got.dtype.kind == 'c' else 1)]!r}"


_HOST = {}


def host_case(key, build, dtype, plan_kw):
    """matrix, adversarial x, plan and restatement, computed once per case"""
    if key not in _HOST:
        ip, ix, da = build()
        n = len(ip) - 1
        x = R.adversarial_d(np.random.default_rng(len(key) + n), n, dtype)
        pl = LR.plan(ip, dtype, **plan_kw)
        y = LR.spmv_split(ip, ix, da, x, dtype, pl)
        _HOST[key] = {"mat": (ip, ix, da), "n": n, "x": x, "plan": pl, "y": y, "parts": LR.block_partials(x, y, dtype, pl)}
    return _HOST[key]


def check_split(pkg, ctx, label, h, dtype, nt=0):
    s = make_solver(pkg, ctx, h["mat"], dtype)
    try:
        assert s.long_rows == want_query(h["plan"]), (label, s.long_rows)
        ys = []
        for fused in (False, True):
            y, form, parts = run_spmv(pkg, ctx, s, h["x"], dtype, fused)
            print(f"{label} fused={int(fused)}: ran {form}")
            assert form == split_form(h["plan"], h["n"], dtype, fused, nt), f"{label}: launched {form}"
            R.check_rows(y, *h["mat"], h["x"], dtype, label=label)
            assert_bits(f"{label} y", y[0], h["y"])
            if fused:
                assert_bits(f"{label} partials", parts[0], h["parts"])
            ys.append(y)
        assert R.bit_equal(ys[0], ys[1])
        V = np.dtype(dtype).itemsize
        ip = h["mat"][0]
        assert s._lib.cgamd_solver_spmv_moved_bytes(s.handle) == int(ip[-1]) * (V + 4) + (h["n"] + 1) * 4 + 2 * h["n"] * V + 2 * h["plan"]["scratch_bytes"]
        return ys[0]
    finally:
        s.close()


# ---- SpMV, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dt", ALL)
def test_small_hubs(pkg, gpu, tuned, dt, variant):
    """n = 737, blocks 1 and 2 heavy, segments of 256 entries: hubs of 255 ... 2500 entries at the first / last row of a block, at the
    last row of the matrix, adjacent, in adjacent blocks, between empty rows, on a segment start; slice starts of every residue"""
    dtype = DT[dt]
    t = LR.small_tune(dtype)
    h = host_case(("small", dt, variant), lambda: LR.small_case(variant, dtype), dtype,
                  dict(heavy_bytes=t["dev.long_row_bytes"], segment=t["dev.long_row_segment"]))
    assert h["plan"]["heavy"] == [1, 2] and h["plan"]["regular"] == [0]
    tuned(resident=0, **t)
    check_split(pkg, gpu[0], f"small {dt} v{variant}", h, dtype)


@pytest.mark.parametrize("dt", ALL)
def test_default_threshold_and_segment(pkg, gpu, tuned, dt):
    """n = 10 000 with a hub of 9000 entries at the defaults: one heavy block of 40, pieces of 2048 entries summed by waves"""
    dtype = DT[dt]
    h = host_case(("default", dt), lambda: LR.default_case(dtype), dtype, {})
    assert h["plan"]["heavy"] == [19] and h["plan"]["segment"] == 2048
    tuned(resident=0)
    check_split(pkg, gpu[0], f"default {dt}", h, dtype)
    # the unflagged handle of the same matrix still runs the stream kernel
    s = make_solver(pkg, gpu[0], h["mat"], dtype, long_rows=False)
    try:
        _, form, _ = run_spmv(pkg, gpu[0], s, h["x"], dtype, False)
        assert form["family"] == "stream" and s.long_rows == ZEROS
    finally:
        s.close()


@pytest.mark.parametrize("dt", ["f64", "c64"])
def test_chunked_body_and_non_temporal_loads(pkg, gpu, tuned, dt):
    """rows of about 40 entries: the regular blocks land in the chunked kernel (4 lanes per row); spmv_nt 0 and 1 give the same bits"""
    dtype = DT[dt]
    ip, _, _ = LR.dense_body_case(dtype)
    t = LR.dense_body_tune(ip, dtype)
    h = host_case(("dense", dt), lambda: LR.dense_body_case(dtype), dtype,
                  dict(heavy_bytes=t["dev.long_row_bytes"], segment=t["dev.long_row_segment"], slice_kb=t["dev.spmv_slice_kb"], chunk_kb=t["dev.spmv_chunk_kb"]))
    assert (h["plan"]["body_kind"], h["plan"]["body_lanes"]) == (7, 4) and h["plan"]["heavy"] == [1]
    ys = []
    for nt in (0, 1):
        tuned(resident=0, spmv_nt=nt, **t)
        ys.append(check_split(pkg, gpu[0], f"dense {dt} nt{nt}", h, dtype, nt=nt))
    assert R.bit_equal(ys[0], ys[1])


@pytest.mark.parametrize("dt", ["f32", "c128"])
def test_rowblock_body_and_non_temporal_loads(pkg, gpu, tuned, dt):
    dtype = DT[dt]
    t = LR.small_tune(dtype)
    h = host_case(("small", dt, 0), lambda: LR.small_case(0, dtype), dtype, dict(heavy_bytes=t["dev.long_row_bytes"], segment=t["dev.long_row_segment"]))
    if dt == "f32":
        assert h["plan"]["body_kind"] == 5
    tuned(resident=0, spmv_nt=1, **t)
    check_split(pkg, gpu[0], f"small {dt} nt1", h, dtype, nt=1)


# ---- no effect where the split does not apply -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["laplacian", "nrhs3", "misaligned", "generic"])
def test_flag_without_effect(pkg, gpu, tuned, what):
    dtype = np.float64
    nrhs = 3 if what == "nrhs3" else 1
    if what == "laplacian":
        mat = R.toeplitz_matrix(np.random.default_rng(5), 1287, (-300, -20, -1, 0, 1, 20, 300), dtype)
    else:
        mat = LR.default_case(dtype)
    n = len(mat[0]) - 1
    x = np.concatenate([R.adversarial_d(np.random.default_rng(40 + r), n, dtype) for r in range(nrhs)])
    tuned(resident=0, dev_generic_spmv=1 if what == "generic" else 0)
    out = []
    for flagged in (False, True):
        s = make_solver(pkg, gpu[0], mat, dtype, nrhs=nrhs, long_rows=flagged, misalign=what == "misaligned")
        try:
            assert s.long_rows == ZEROS
            moved = s._lib.cgamd_solver_spmv_moved_bytes(s.handle)
            out.append([run_spmv(pkg, gpu[0], s, x, dtype, fused, nrhs) for fused in (False, True)] + [moved])
        finally:
            s.close()
    for a, b in zip(out[0][:2], out[1][:2]):
        assert a[1] == b[1] and a[1]["family"] != "split", (a[1], b[1])
        assert R.bit_equal(a[0], b[0])
        if a[2] is not None:
            assert R.bit_equal(a[2], b[2])
    assert out[0][2] == out[1][2]


# ---- loops ----------------------------------------------------------------------------------------------------------------------------
_LOOP = {}


def loop_case(dt):
    if dt not in _LOOP:
        dtype = DT[dt]
        ip, ix, da = LR.loop_system(dtype)
        n = len(ip) - 1
        b = np.random.default_rng(5).standard_normal(n).astype(dtype)
        W = np.clongdouble if np.dtype(dtype).kind == "c" else np.longdouble
        _LOOP[dt] = {"mat": (ip, ix, da), "n": n, "b": b, "rows": np.repeat(np.arange(n), np.diff(ip)), "aw": da.astype(W), "bw": b.astype(W), "W": W}
    return _LOOP[dt]


def true_residual(c, x):
    ax = np.zeros(c["n"], c["W"])
    np.add.at(ax, c["rows"], c["aw"] * x.astype(c["W"])[c["mat"][1]])
    r = c["bw"] - ax
    return float(np.sqrt(np.sum(np.abs(r) ** 2))), float(np.sqrt(np.sum(np.abs(c["bw"]) ** 2)))


def assert_split_handle(s):
    q = s.long_rows
    assert q["heavy_blocks"] >= 1 and q["segments"] >= 3 and q["segment"] == 2048 and q["body_kind"] in (5, 7), q


@pytest.mark.parametrize("dt", ["f64", "c128"])
def test_history_against_the_oracle(pkg, gpu, tuned, dt):
    c = loop_case(dt)
    tuned()
    s = make_solver(pkg, gpu[0], c["mat"], DT[dt])
    try:
        assert_split_handle(s)
        s.set_rhs(c["b"])
        s.iterate(8)
        assert s.last_spmv_form()["family"] == "split"
        h = s.history()[:, 0]
    finally:
        s.close()
    _, ho = cg_oracle.cg(*c["mat"], c["b"], n_iterations=8, mode=cg_oracle.MODE_SEQUENTIAL)
    rel = np.abs(h - ho[:, 0]) / np.abs(ho[:, 0])
    print(f"history {dt}: largest relative difference to the oracle {rel.max():.3g}")
    assert rel.max() < 1e-10


@pytest.mark.parametrize("pre", [None, "jacobi"])
@pytest.mark.parametrize("dt", ALL)
def test_solve_to_tolerance(pkg, gpu, tuned, dt, pre):
    c = loop_case(dt)
    single = dt in ("f32", "c64")
    rel = 1e-4 if single else 1e-8
    nb = float(np.linalg.norm(c["b"].astype(np.complex128 if np.dtype(DT[dt]).kind == "c" else np.float64)))
    tuned()
    s = make_solver(pkg, gpu[0], c["mat"], DT[dt])
    try:
        assert_split_handle(s)
        if pre:
            s.set_preconditioner(pre)
        x, its, _ = s.solve_until(c["b"], tol=rel * nb, maxit=400)
        assert s.last_spmv_form()["family"] == "split"
    finally:
        s.close()
    res, bn = true_residual(c, x)
    print(f"solve {dt} pre={pre}: {int(its[0])} iterations, true residual {res / bn:.3g} ||b||")
    assert 0 < its[0] < 400
    assert res < 2 * rel * bn


def _run(pkg, ctx, c, cuts, flags=0):
    s = make_solver(pkg, ctx, c["mat"], np.float64, flags=flags)
    try:
        assert_split_handle(s)
        s.set_rhs(c["b"])
        for k in cuts:
            s.iterate(k)
        assert s.last_spmv_form()["family"] == "split"
        return s.x(), s.history()
    finally:
        s.close()


def test_same_bits_however_the_solve_is_run(pkg, gpu, tuned):
    c = loop_case("f64")
    tuned()
    x8, h8 = _run(pkg, gpu[0], c, [8])
    for label, (x, h) in {"2 x iterate(4)": _run(pkg, gpu[0], c, [4, 4]), "NO_GRAPH": _run(pkg, gpu[0], c, [8], flags=pkg._lib.NO_GRAPH),
                          "a second run": _run(pkg, gpu[0], c, [8])}.items():
        assert R.bit_equal(x, x8) and R.bit_equal(h, h8), label
    s = make_solver(pkg, gpu[0], c["mat"], np.float64)
    try:
        s.set_rhs(c["b"]); s.iterate(8); xa, ha = s.x(), s.history()
        s.set_rhs(c["b"]); s.iterate(8); xb, hb = s.x(), s.history()
        assert R.bit_equal(xa, x8) and R.bit_equal(xb, x8) and R.bit_equal(ha, h8) and R.bit_equal(hb, h8)
    finally:
        s.close()


def test_refresh_values_keeps_the_lists(pkg, gpu, tuned):
    dtype = np.float64
    t = LR.small_tune(dtype)
    h = host_case(("small", "f64", 0), lambda: LR.small_case(0, dtype), dtype, dict(heavy_bytes=t["dev.long_row_bytes"], segment=t["dev.long_row_segment"]))
    ip, ix, da = h["mat"]
    tuned(resident=0, **t)
    s = make_solver(pkg, gpu[0], h["mat"], dtype)
    try:
        before = s.long_rows
        s.refresh_values(np.asarray(da * 2, dtype=dtype))
        assert s.long_rows == before == want_query(h["plan"])
        y, form, parts = run_spmv(pkg, gpu[0], s, h["x"], dtype, True)
        assert form == split_form(h["plan"], h["n"], dtype, True)
        want = LR.spmv_split(ip, ix, da * 2, h["x"], dtype, h["plan"])
        assert_bits("refreshed y", y[0], want)
        assert_bits("refreshed partials", parts[0], LR.block_partials(h["x"], want, dtype, h["plan"]))
    finally:
        s.close()


def test_amg_on_a_flagged_handle(pkg, gpu, tuned):
    c = loop_case("f64")
    nb = float(np.linalg.norm(c["b"]))
    tuned()
    its = []
    for flagged in (False, True):
        s = make_solver(pkg, gpu[0], c["mat"], np.float64, long_rows=flagged)
        try:
            s.set_preconditioner("amg")
            x, k, _ = s.solve_until(c["b"], tol=1e-8 * nb, maxit=400)
            res, bn = true_residual(c, x)
            assert res < 2e-8 * bn
            its.append(int(k[0]))
        finally:
            s.close()
    print(f"amg: {its[0]} iterations unflagged, {its[1]} flagged")
    assert its[0] == its[1] and 0 < its[0] < 400
