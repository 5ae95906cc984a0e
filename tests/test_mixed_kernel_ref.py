"""The host restatement of the mixed-precision kernels (tests/mixed_kernel_ref.py) on the inputs of tests/test_gpu_mixed_kernels.py,
without a GPU: the restated order of the norm is a sum (within the derived bound of an exact one), it is not numpy's order nor the
other form's (or a comparison of bits would prove nothing), the host's float64 -> float32 conversion is the IEEE one the planted
values are written for, and the case table reaches every kernel form."""
import numpy as np
import pytest

import mixed_kernel_ref as K

CASES = K.cases()
_INPUTS = {}


def inputs(c):
    if c["id"] not in _INPUTS:
        _INPUTS[c["id"]] = K.inputs(c)
    return _INPUTS[c["id"]]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_restated_norm_is_within_the_bound_of_the_exact_sum(c):
    for name in ("x_hi", "v"):
        v = inputs(c)[name]
        exact = K.norm2_exact(v)
        for vec in (True, False):
            partials, out = K.norm2(v, vec)
            assert partials.shape == (c["nrhs"], K.grid(c["m"]))
            err = np.abs(out - exact)
            bound = K.norm2_bound(c["m"], exact)
            assert np.all(err <= bound), (c["id"], name, vec, err, bound)


def test_grid_rule():
    assert [K.grid(m) for m in (1, 4096, 4097, 8192, 8193, 1024 * 4096, K.BIG, 10 ** 9)] == [1, 1, 2, 2, 3, 1024, 1024, 1024]
    # the cap case: more quads than one pass of the capped grid takes, so some threads make a fifth pass and some do not
    nq, stride = K.BIG // 4, 1024 * 256
    assert 4 * stride < nq < 5 * stride and K.BIG % 4 == 3


def test_restated_order_shows_in_the_bits():
    """from 513 lanes on, in every case (on the narrow vector): the 16-byte order and the scalar order give different results, and the
    order the case's pointers select differs from numpy's pairwise sum.  Below that a thread holds one quad or one lane and the
    orders can coincide; there at least one case must tell the forms apart."""
    small = 0
    for c in CASES:
        v = inputs(c)["v"]
        pv, ov = K.norm2(v, True)
        ps, os_ = K.norm2(v, False)
        with np.errstate(all="ignore"):
            plain = np.sum(v * v, axis=1)
        if c["m"] >= 513:
            assert np.any(bits(ov) != bits(os_)) and np.any(bits(pv) != bits(ps)), c["id"]
            assert np.any(bits(ov if c["vec_norm"] else os_) != bits(plain)), c["id"]
        else:
            small += int(np.any(bits(ov) != bits(os_)))
    assert small >= 1


def test_planted_values_round_as_ieee_says():
    """numpy's cast is the reference of round_down and round_values: nearest-even, gradual underflow, overflow to inf"""
    f = np.float32
    want = [f(1.0), f(1.0 + 2.0 ** -22), f(-1.0), f(np.inf), f(-np.inf), np.finfo(f).max, f(-0.0), f(np.nan), f(20227 * 2.0 ** -149),
            f(2.0 ** -148), f(-0.0), f(2.0 ** -149), f(2.0 ** -126)]
    got = K.round_values(np.array([p[0] for p in K.PLANTS]))
    assert bits(got).tolist() == bits(np.array(want, dtype=f)).tolist(), [p[1] for p, a, b in zip(K.PLANTS, got, want) if not (a == b or (a != a and b != b))]
    assert np.signbit(got[6]) and np.signbit(got[10]) and got[8] != 0 and abs(got[8]) < np.finfo(f).tiny
    # the planted values survive the exact scaling of round_down in every case
    for c in CASES:
        if c["m"] > 4096:
            continue
        inp = inputs(c)
        out = K.round_down(inp["r_hi"], inp["inv_scale"], c["ld_lo"] * c["R"])
        assert out.shape == (c["nrhs"], c["ld_lo"] * c["R"]) and not out[:, c["m"]:].any() and not np.signbit(out[:, c["m"]:]).any()
        shift = c["seed"] % len(K.PLANTS)
        for r in range(c["nrhs"]):
            for j in range(min(c["m"], len(K.PLANTS))):
                assert bits(out[r, j:j + 1])[0] == bits(np.array([want[(j + shift + r) % len(want)]], dtype=f))[0], (c["id"], r, j)
    # all thirteen are met over the tiny cases too, whose columns are shorter than the list
    seen = {(j + c["seed"] % len(K.PLANTS)) % len(K.PLANTS) for c in CASES for j in range(min(c["m"], len(K.PLANTS)))}
    assert seen == set(range(len(K.PLANTS)))


def test_accumulate_restated():
    c = next(c for c in CASES if c["group"] == "rhs3" and c["dt"] == "f64")
    inp = inputs(c)
    for mask in c["masks"]:
        out = K.accumulate(inp["x_hi"], inp["x_lo"], inp["scale"], mask)
        for r in range(3):
            same = bits(out[r]).tolist() == bits(inp["x_hi"][r]).tolist()
            assert same == (not mask[r]), (mask, r)
    # one rounding: against the longdouble sum of the exact product (s * l is exact there too).  The sum in longdouble is within
    # 2^-64 of the exact one, the restated one within 2^-53: 1.01 * 2^-53 covers both.  Where the host's longdouble is no wider than
    # double the comparison is of the thing with itself and still holds
    out = K.accumulate(inp["x_hi"], inp["x_lo"], inp["scale"], [1, 1, 1])
    LD = np.longdouble
    wide = inp["x_hi"].astype(LD) + inp["scale"][:, None].astype(LD) * inp["x_lo"].astype(LD)
    assert np.all(np.abs(out.astype(LD) - wide) <= np.abs(wide) * LD(1.01) * LD(2.0) ** -53)
    assert sorted(np.log2(inp["scale"]).tolist()) == [-60, 7, 60]


def test_the_form_rule_and_the_cases_that_reach_every_form():
    assert K.takes_vec(256, 8, 512, 4, 1) and not K.takes_vec(264, 16, 512, 16, 1) and not K.takes_vec(256, 16, 516, 16, 1)
    assert K.takes_vec(256, 958 * 8, 512, 960 * 4, 3) and not K.takes_vec(256, 957 * 8, 512, 960 * 4, 3)
    assert not K.takes_vec(256, 958 * 8, 512, 957 * 4, 3) and K.takes_vec(256, 957 * 16, None, 0, 3)
    seen = set()
    for c in CASES:
        R = c["R"]
        hi, lo = 4096 + c["off_hi"], 8192 + c["off_lo"]
        vec = K.takes_vec(hi, c["ld_hi"] * 8 * R, lo, c["ld_lo"] * 4 * R, c["nrhs"])
        assert vec == c["vec"], c["id"]
        vn = K.takes_vec(hi, c["ld_hi"] * 8 * R, None, 0, c["nrhs"])
        assert vn == c["vec_norm"], c["id"]
        seen |= {("accumulate", c["dt"], vec), ("round_down", c["dt"], vec), ("norm2", c["dt"], vn),
                 ("round_values", c["dt"], K.round_values_takes_vec(hi, lo))}
    assert seen == {(k, dt, v) for k in ("accumulate", "round_down", "norm2", "round_values") for dt in ("f64", "c128") for v in (True, False)}
