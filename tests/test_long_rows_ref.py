"""tests/long_rows_ref.py against the extended-precision product and against the one-lane restatement (CPU only)."""
import numpy as np
import pytest

import long_rows_ref as LR
import spmv_ref as R

DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}


def _x(n, dtype, seed=3):
    return R.adversarial_d(np.random.default_rng(seed), n, dtype)


def _check(ip, ix, da, dtype, pl, label):
    n = len(ip) - 1
    x = _x(n, dtype)
    y = LR.spmv_split(ip, ix, da, x, dtype, pl)
    R.check_rows(y, ip, ix, da, x, dtype, label=label)                 # every row within row_bound of spmv_ext
    lane = R.spmv_in_type(ip, ix, da, x, dtype)[0]
    _, plain = LR.heavy_rows(ip, ix, da, x, dtype, pl)
    rows = np.array(sorted(r for r, p in plain.items() if p), dtype=np.int64)
    assert rows.size > 0
    assert np.array_equal(R.bits(y[rows]), R.bits(lane[rows])), f"{label}: a short row inside one segment differs from spmv_in_type"
    return y, lane, plain


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dt", list(DT))
def test_small_case(dt, variant):
    dtype = DT[dt]
    ip, ix, da = LR.small_case(variant, dtype)
    t = LR.small_tune(dtype)
    pl = LR.plan(ip, dtype, t["dev.long_row_bytes"], t["dev.long_row_segment"])
    assert pl["heavy"] == [1, 2] and pl["regular"] == [0] and pl["segment"] == 256
    assert pl["body_kind"] in (5, 7)
    assert [e0 for _, e0 in pl["segments"][:2]] == [int(ip[256]) // 4 * 4, int(ip[256]) // 4 * 4 + 256]
    y, lane, plain = _check(ip, ix, da, dtype, pl, f"small {dt} v{variant}")
    # the hubs are not plain rows: split, or longer than a one-lane piece
    assert not any(plain[r] for r in (256, 511, 300, 301, 400, 600, 736))
    # pieces of more than 64 entries are summed by a wave: on adversarial x that differs from the one-lane sum somewhere
    assert not np.array_equal(R.bits(y[[256, 511, 300, 301, 400, 600, 736]]), R.bits(lane[[256, 511, 300, 301, 400, 600, 736]]))


def test_slice_starts_cover_every_residue():
    starts = set()
    for v in (0, 1):
        ip, _, _ = LR.small_case(v, np.float64)
        starts |= {int(ip[256]) % 4, int(ip[512]) % 4}
    assert starts == {0, 1, 2, 3}


@pytest.mark.parametrize("dt", list(DT))
def test_default_case_is_kind_0_today_and_block_form_for_the_body(dt):
    """the launcher's thresholds restated (LR.choose_kind): the whole matrix ends at the stream kernel, its regular blocks do not"""
    dtype = DT[dt]
    ip, ix, da = LR.default_case(dtype)
    spans, _ = R.plan_spans(ip)
    assert LR.choose_kind(spans, dtype) == (0, 1)
    pl = LR.plan(ip, dtype)
    assert pl["heavy"] == [5000 // 256] and pl["segment"] == 2048 and len(pl["regular"]) == (10000 + 255) // 256 - 1
    assert sorted(pl["regular"]) == [rb for rb in range(40) if rb != 19]
    # cycle 64: work-group b runs on XCD b % 8, XCD j takes blocks 8 j .. 8 j + 7 of a cycle; block 19 = rowblock_of(26) is left out
    assert pl["regular"][:3] == [0, 8, 16] and pl["regular"][3:6] == [24, 32, 1] and pl["regular"] == [LR.rowblock_of(b, 40, 64) for b in range(64) if LR.rowblock_of(b, 40, 64) not in (-1, 19)]
    assert pl["body_kind"] == (7 if dt == "c128" else 5)      # (256 rows of ~8 entries at 20 bytes: above the 40 KB slice)
    if dt == "f64":
        _check(ip, ix, da, dtype, pl, "default f64")


@pytest.mark.parametrize("dt", list(DT))
def test_loop_system_plan(dt):
    dtype = DT[dt]
    ip, ix, da = LR.loop_system(dtype)
    assert int(np.diff(ip).max()) == 5999
    spans, _ = R.plan_spans(ip)
    assert LR.choose_kind(spans, dtype) == (0, 1)
    pl = LR.plan(ip, dtype)
    assert 3000 // 256 in pl["heavy"] and pl["body_kind"] in (5, 7)


def test_dense_body_is_chunked():
    dtype = np.float64
    ip, ix, da = LR.dense_body_case(dtype)
    t = LR.dense_body_tune(ip, dtype)
    pl = LR.plan(ip, dtype, t["dev.long_row_bytes"], t["dev.long_row_segment"], slice_kb=t["dev.spmv_slice_kb"], chunk_kb=t["dev.spmv_chunk_kb"])
    assert pl["heavy"] == [1] and (pl["body_kind"], pl["body_lanes"]) == (7, 4)
    _check(ip, ix, da, dtype, pl, "dense body f64")


def test_no_heavy_block_is_an_empty_plan():
    ip, ix, da = R.toeplitz_matrix(np.random.default_rng(1), 1287, (-37, -1, 0, 1, 37), np.float64)
    pl = LR.plan(ip, np.float64)
    assert pl["heavy"] == [] and pl["regular"] == [] and pl["segments"] == [] and pl["scratch_bytes"] == 0 and pl["body_kind"] == 0


def test_loop_system_is_symmetric_positive_definite():
    ip, ix, da = LR.loop_system(np.float64)
    n = len(ip) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(ip)), ix] = da
    assert np.array_equal(A, A.T)
    assert np.linalg.eigvalsh(A).min() > 0
