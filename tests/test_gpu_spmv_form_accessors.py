"""The accessors and byte models of a handle follow the SpMV its loop LAUNCHES (csrc/solver.cpp loop_form: the launcher's own decision,
csrc/spmv_form.cpp).  Each case creates a CGAMD_NO_GRAPH handle under one set of tuning keys, runs set_rhs and one iteration, and
compares what the launch site recorded (cgamd_last_spmv_form) with Solver.spmv_form(), joint_codes, row_codes, row_pairs, row_pipe,
spmv_schedule and spmv_moved_bytes -- the byte count restated here from the RECORDED form alone.  The sets leave the defaults one key
at a time, the states in which a second copy of the launch condition used to answer for a form that does not run (DESIGN.md
section 1): dev.vc_pipe = 0 on joint codes, dev.spmv_unroll below the longest row, value codes built but not launched."""
import numpy as np
import pytest

import spmv_ref as R

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
# struct Tuning's defaults of every key this module sets
DEFAULTS = {"index_codes": 1, "index_codes_min_mb": 32, "resident": 1, "resident_wide": 1, "two_launch": 1, "dev.value_codes": 1, "dev.vc_pipe": 1,
            "dev.joint_codes": 1, "dev.row_codes": 1, "dev.row_codes_min_mb": 32, "dev.row_pairs": -1, "dev.row_pairs_min_mb": 256,
            "dev.spmv_plane": -1, "dev.spmv_unroll": 0}
# codes at any size; the launched loop through launch_spmv (no resident loop, no two-launch loop: their SpMV records no form)
BASE = {"index_codes_min_mb": 0, "dev.row_codes_min_mb": 0, "dev.row_pairs_min_mb": 0, "resident": 0, "resident_wide": 0, "two_launch": 0}
N = 2301                             # 9 row blocks, 3 super blocks: a ragged last group
# (matrix, keys) -> the (family, value encoding) the set is written for, None: whatever the default rules choose for the type.
# "palette": the 7-point pattern with values from a palette of 5 of test_value_coded_forms_and_pipeline_tails -- more than 256 row
# patterns, so the per-non-zero forms; "const": the same pattern with constant coefficients, 27 row patterns -- the row-coded forms, and
# the states in which row codes are PRESENT and do not run; "nine": every row 9 entries long, a 256-row slice of 2300 entries, more
# than the 8 x 256 the code staging holds (the matrix of _rows_up_to(9, ...) with no entry dropped), palette of 5 values
SETS = {
    ("palette", "default"): ({}, ("vcp", 2)), ("palette", "vc_pipe=0"): ({"dev.vc_pipe": 0}, ("vc", 1)),
    ("palette", "joint_codes=0"): ({"dev.joint_codes": 0}, ("vcp", 1)), ("palette", "spmv_unroll=4"): ({"dev.spmv_unroll": 4}, ("vc", 1)),
    ("palette", "value_codes=0"): ({"dev.value_codes": 0}, ("rowblock", 0)), ("palette", "index_codes=0"): ({"index_codes": 0}, ("rowblock", 0)),
    ("palette", "row codes"): ({"dev.row_pairs": 0}, ("vcp", 2)), ("palette", "row pairs"): ({"dev.row_pairs": 1}, ("vcp", 2)),
    ("palette", "spmv_plane=1"): ({"dev.spmv_plane": 1}, ("vcp", 2)),
    ("const", "default"): ({}, None), ("const", "row codes"): ({"dev.row_pairs": 0}, ("rowcode", 3)),
    ("const", "row pairs"): ({"dev.row_pairs": 1}, ("rowpair", 3)), ("const", "spmv_plane=1"): ({"dev.spmv_plane": 1}, None),
    ("const", "row_codes=0"): ({"dev.row_codes": 0}, ("vcp", 2)), ("const", "vc_pipe=0"): ({"dev.vc_pipe": 0}, ("vc", 1)),
    ("const", "spmv_unroll=4"): ({"dev.spmv_unroll": 4}, ("vc", 1)), ("const", "joint_codes=0"): ({"dev.joint_codes": 0}, ("vcp", 1)),
    ("nine", "default"): ({}, ("rowblock", 0)),
}
P7, P9 = (-64, -8, -1, 0, 1, 8, 64), (-64, -8, -2, -1, 0, 1, 2, 8, 64)
_MAT = {}


def matrix(kind, dt):
    if (kind, dt) not in _MAT:
        if kind == "const":
            ip = np.zeros(N + 1, dtype=np.int32)
            ix, da = [], []
            for r in range(N):
                for o, v in zip(P7, (-1.25, -0.75, -1.5, 6.5, -1.125, -0.875, -1.375)):
                    if 0 <= r + o < N:
                        ix.append(r + o)
                        da.append(v)
                ip[r + 1] = len(ix)
            _MAT[(kind, dt)] = ip, np.asarray(ix, np.int32), np.asarray(da).astype(DT[dt])
        else:
            n, offs, seed = (509, P9, 6) if kind == "nine" else (N, P7, 5)
            _MAT[(kind, dt)] = R.toeplitz_matrix(np.random.default_rng(n), n, offs, DT[dt], R.palette_values(np.random.default_rng(seed), 5, DT[dt]))
    return _MAT[(kind, dt)]


@pytest.fixture
def tuned(pkg):
    lib = pkg._lib.load()

    def put(kv):
        for k, v in kv.items():
            assert k in DEFAULTS, k
            pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))

    def tune(kv):
        put(DEFAULTS)
        put(BASE)
        put(kv)
    yield tune
    put(DEFAULTS)


def moved_bytes(form, n, nnz, V):
    """bytes one SpMV of the recorded form moves: the matrix as that form reads it, x read, y written"""
    if form["family"] in ("rowcode", "rowpair"):
        return n + 2 * n * V                                         # one code byte per row
    value = {0: V, 1: 1, 2: 0, 3: 0}[form["value_codes"]]
    index = {0: 4, 8: 1, 16: 2}[form["index_bits"]]
    return nnz * (value + index) + (n + 1) * 4 + 2 * n * V


@pytest.mark.parametrize("kind,name", list(SETS), ids=[f"{k}-{n}" for k, n in SETS])
@pytest.mark.parametrize("dt", list(DT))
def test_accessors_follow_the_launch(pkg, gpu, tuned, dt, kind, name):
    ctx = gpu[0]
    dtype = DT[dt]
    ip, ix, da = matrix(kind, dt)
    n, nnz, V = len(ip) - 1, len(ix), np.dtype(dtype).itemsize
    if kind == "nine":
        assert R.plan_spans(ip)[0][0] > 2048 and R.plan_spans(ip)[1] == 9 and R.distinct_values(da) == 5
    keys, want = SETS[(kind, name)]
    tuned(keys)
    s = pkg.Solver(ctx, n, nnz, da, ip, ix, 1, flags=pkg._lib.NO_GRAPH, dtype=dtype)
    try:
        s.set_rhs(np.linspace(1.0, 2.0, n).astype(dtype))
        s.iterate(1)
        ctx.synchronize()
        ran = s.last_spmv_form()
        print(f"{kind} {name} {dt}: ran {ran}; spmv_form {s.spmv_form()}; joint {s.joint_codes} rows {s.row_codes} pairs {s.row_pairs} "
              f"pipe {s.row_pipe} schedule {s.spmv_schedule} moved {s.spmv_moved_bytes}")
        assert ran["family"] is not None and ran["fused"] == 1
        assert s.spmv_form() == ran
        assert (s.joint_codes > 0) == (ran["value_codes"] in (2, 3))
        assert (s.row_codes > 0) == (ran["family"] in ("rowcode", "rowpair"))
        assert (s.row_pairs > 0) == (ran["family"] == "rowpair")
        # the launched depth: dev.row_pipe's default rule by the size of a value (4-byte values all four row blocks, 8-byte values one),
        # of which the pair form keeps at most its two passes
        depth = {"rowcode": 4 if V == 4 else 1, "rowpair": min(2, 4 if V == 4 else 1)}.get(ran["family"], 0)
        assert s.row_pipe == depth
        sched = s.spmv_schedule
        assert sched["grid"] == (ran["grid"] if ran["family"] in ("rowcode", "rowpair") else 0)
        assert s.spmv_moved_bytes == moved_bytes(ran, n, nnz, V)
        # and the set lands where it is written for
        if want:
            assert (ran["family"], ran["value_codes"]) == want
        if kind == "const" and name in ("default", "spmv_plane=1"):      # the default rule: 8-byte values in pairs, 4-byte values by rows
            assert ran["family"] == ("rowpair" if V == 8 else "rowcode")
            assert sched["kind"] == ("plane" if name == "spmv_plane=1" else "cycle")
    finally:
        s.close()
