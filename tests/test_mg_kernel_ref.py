"""The host restatement of the multigrid cycle kernels (tests/mg_kernel_ref.py) on its own, without a GPU: that it is the algorithm of
mg_ref / amg_ref, that the orders it fixes show in the bits on the very inputs the device tests use (so a device kernel with another
order would fail there), and that the case lists reach every path."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref
import mg_kernel_ref as K
import mg_ref
import spmv_ref as R

ALL = [np.float32, np.float64, np.complex64, np.complex128]
DIMS = (13, 11, 9)


def system(dtype):
    A = mg_ref.variable7(*DIMS)
    return sp.csr_matrix(A * (1.0 + 0.05j)) if np.dtype(dtype).kind == "c" else A


def rhs(dtype, nrhs=1, seed=11):
    rng = np.random.default_rng(seed)
    n = int(np.prod(DIMS))
    B = rng.standard_normal((nrhs, n))
    if np.dtype(dtype).kind == "c":
        B = B + 1j * rng.standard_normal((nrhs, n))
    return B.astype(dtype)


def cycle_error(z, z_ref):
    z_ref = np.asarray(z_ref)
    return float(np.max(np.abs(np.asarray(z).astype(z_ref.dtype) - z_ref)) / np.max(np.abs(z_ref)))


def assert_same_algorithm(H, dtype, label):
    """the bound of check_cycle (tests/test_gpu_multigrid.py) with the restated chain in the device's place: error against the
    extended-precision cycle <= 4 max(error of the cycle in the value type, 4 eps)"""
    B = rhs(dtype)
    z = K.cycle_bits(K.levels_of(H, dtype), B, H.omega, dtype)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    z_ref = H.vcycle(B[0], mg_ref.wide(dtype, True))
    e_bits, e_type = cycle_error(z[0], z_ref), cycle_error(H.vcycle(B[0], dtype), z_ref)
    print(f"  {label} {np.dtype(dtype).name}: e(chain) {e_bits:.3e}, e(cycle in type) {e_type:.3e}, bound {4.0 * max(e_type, 4.0 * eps):.3e}")
    assert e_bits <= 4.0 * max(e_type, 4.0 * eps), (label, e_bits, e_type)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("opts", [{"min_rows": 32}, {"min_rows": 32, "smooth_steps": 2, "over_correction": 1.0},
                                  {"min_rows": 32, "smooth_steps": 3}, {"min_rows": 5000}], ids=str)
def test_chain_is_the_cycle_of_mg_ref(dtype, opts):
    H = mg_ref.Hierarchy(system(dtype), DIMS, dtype, **opts)
    assert len(H.levels) == (1 if opts["min_rows"] == 5000 else 4)
    assert_same_algorithm(H, dtype, f"grid {opts}")


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("opts", [{"min_rows": 32}, {"min_rows": 32, "smooth_steps": 3, "over_correction": 1.0}, {"min_rows": 5000}], ids=str)
def test_chain_is_the_cycle_of_amg_ref(dtype, opts):
    H = amg_ref.Hierarchy(system(dtype), dtype, **opts)
    assert len(H.levels) == (1 if opts["min_rows"] == 5000 else len(H.levels)) and (opts["min_rows"] == 5000 or len(H.levels) >= 3)
    assert_same_algorithm(H, dtype, f"algebraic {opts}")


def test_real_chain_has_the_bits_of_the_cycle_in_the_value_type():
    """for the real types the two restatements are the same operations in the same order (scipy adds a row up in stored order)"""
    for dtype in (np.float32, np.float64):
        H = mg_ref.Hierarchy(system(dtype), DIMS, dtype, min_rows=32, smooth_steps=2)
        B = rhs(dtype)
        assert R.bit_equal(K.cycle_bits(K.levels_of(H, dtype), B, H.omega, dtype)[0], H.vcycle(B[0], dtype))


def test_padding_rows_and_leading_dimension_do_not_change_the_chain():
    """level 0 over n > nu rows with dinv = 0 behind nu: the rows of the grid keep their bits, the padding rows give +0"""
    dtype = np.float64
    H = mg_ref.Hierarchy(system(dtype), DIMS, dtype, min_rows=32)
    lv = K.levels_of(H, dtype)
    B = rhs(dtype, 2)
    z = K.cycle_bits(lv, B, H.omega, dtype)
    L0, nu = lv[0], lv[0]["nu"]
    lv[0] = K.level(L0["ip"], L0["ix"], L0["da"], np.concatenate([L0["dinv"], np.zeros(3)]), L0["c0"], L0["c1"], n=nu + 3, nu=nu,
                    members=L0["members"], agg=L0["agg"])
    zp = K.cycle_bits(lv, np.concatenate([B, np.zeros((2, 3))], axis=1), H.omega, dtype)
    assert R.bit_equal(zp[:, :nu], z) and not zp[:, nu:].view(np.uint64).any()


# ---- the orders show in the bits ----------------------------------------------------------------------------------------------------------
TRANSFER = K.transfer_cases()


@pytest.mark.parametrize("c", TRANSFER, ids=[c["id"] for c in TRANSFER])
def test_member_order_shows_in_the_bits(c):
    """descending members change the bits of at least one aggregate in every column of every case that has an aggregate of three rows
    or more; an aggregate of one or two rows has one order only (IEEE addition commutes)"""
    inp, dtype = K.transfer_inputs(c), K.DTYPES[c["dt"]]
    sizes = (inp["members"] >= 0).sum(axis=1)
    assert np.array_equal(np.sort(inp["members"][inp["members"] >= 0]), np.arange(inp["nf"]))        # a partition of the fine rows
    up = K.restrict(dtype, inp["members"], inp["b"], inp["w"], inp["dinv_c"], inp["c1"])[0]
    down = K.restrict(dtype, inp["members"], inp["b"], inp["w"], inp["dinv_c"], inp["c1"], K.Rules(members="descending"))[0]
    differ = R.bits(up).reshape(up.shape[0], up.shape[1], -1) != R.bits(down).reshape(up.shape[0], up.shape[1], -1)
    differ = differ.any(axis=2)
    assert not differ[:, sizes <= 2].any()
    if sizes.max() >= 3:
        assert differ.any(axis=1).all(), c["id"]
        print(f"  {c['id']}: {int(differ.sum())} of {differ.shape[0] * int((sizes >= 3).sum())} sums of 3 or more rows change with the order")
    if c["kind"] == "stored":
        assert sizes.max() == 8                                                   # a list without a -1
        if c["nagg"] >= 8:
            assert set(sizes.tolist()) == set(range(1, 9))
        assert (np.diff(inp["members"], axis=1)[inp["members"][:, 1:] >= 0] > 0).all()        # ascending, and scattered:
        assert c["nagg"] == 1 or (np.diff(inp["members"], axis=1)[inp["members"][:, 1:] >= 0] > 1).mean() > 0.9
    # the restatement through member lists is the sum np.add.at forms through the map
    res = K.join(K._sub(K.parts(inp["b"], dtype), K.parts(inp["w"], dtype)), dtype)
    for r in range(res.shape[0]):
        via_map = np.zeros(inp["nc"], dtype)
        np.add.at(via_map, inp["agg"], res[r])
        assert R.bit_equal(via_map, up[r])


SMOOTH = K.smooth_cases()


def test_later_step_operand_order_and_contraction():
    """c0 d + t and t + c0 d are one IEEE addition with its operands exchanged: never another bit.  A contracted multiply-add rounds
    once where the kernel rounds twice: it changes bits in every mode-2 case of more than one lane"""
    seen = 0
    for c in SMOOTH:
        if c["mode"] != 2:
            continue
        inp, dtype = K.smooth_inputs(c), K.DTYPES[c["dt"]]
        args = (dtype, 2, inp["dinv"], inp["b"], inp["w"], inp["d"], inp["x"], inp["c0"], inp["c1"], 1)
        x, d = K.smooth_step(*args)
        xs, ds = K.smooth_step(*args, K.Rules(later="t+c0d"))
        ok = ~np.isnan(R.bits(x).view(R.real_type(dtype)))                       # (which NaN comes back is the one thing left open)
        assert np.array_equal(R.bits(x)[ok], R.bits(xs)[ok]) and np.array_equal(np.isnan(d), np.isnan(ds))
        if c["size"] > 1 and c["size"] <= 257:                                   # (exact rational arithmetic lane by lane: the small sizes)
            xf, df = K.smooth_step(*args, K.Rules(contract=True))
            assert not R.bit_equal(df, d), c["id"]
            seen += 1
    assert seen >= 8


def test_orders_show_in_the_bits_of_the_whole_cycle():
    """on the hierarchies of the device test the chain with descending members, and with a contracted later step, gives another z:
    comparing mg_apply with cycle_bits holds the device to both"""
    for dtype in (np.float32, np.float64, np.complex64):
        H = mg_ref.Hierarchy(system(dtype), DIMS, dtype, min_rows=32, smooth_steps=2)
        lv, B = K.levels_of(H, dtype), rhs(dtype)
        z = K.cycle_bits(lv, B, H.omega, dtype)
        assert not R.bit_equal(K.cycle_bits(lv, B, H.omega, dtype, K.Rules(members="descending")), z)
        assert not R.bit_equal(K.cycle_bits(lv, B, H.omega, dtype, K.Rules(contract=True)), z)
        assert R.bit_equal(K.cycle_bits(lv, B, H.omega, dtype, K.Rules(later="t+c0d")), z)


def test_fused_multiply_add_restatement():
    """_fma against cases worked by hand: 1 + 2^-12 squared is 1 + 2^-11 + 2^-24, which float32 rounds to 1 + 2^-11 before 2^-24 is
    taken off again; the single rounding keeps it"""
    a = np.array([1 + 2.0 ** -12], np.float32)
    two = a * a + np.float32(-(1 + 2.0 ** -11))
    one = K._fma(np.float32(a[0]), a, np.array([-(1 + 2.0 ** -11)], np.float32))
    assert two[0] == 0.0 and one[0] == np.float32(2.0 ** -24)
    a = np.array([1 + 2.0 ** -27])
    assert (a * a - (1 + 2.0 ** -26))[0] == 0.0 and K._fma(a[0], a, np.array([-(1 + 2.0 ** -26)]))[0] == 2.0 ** -54


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_path():
    assert {(c["dt"], c["mode"], c["store_d"]) for c in SMOOTH} == {(dt, m, s) for dt in K.DTYPES for m in (0, 1, 2) for s in (0, 1)}
    for dt in K.DTYPES:
        for mode in (0, 1, 2):
            mine = [c for c in SMOOTH if c["dt"] == dt and c["mode"] == mode]
            assert {c["size"] for c in mine} == {1, 255, 256, 257, 1287}
            assert {c["nrhs"] for c in mine} == {1, 3} and {c["off"] for c in mine} == {0, 8}
            assert all(c["ld"] > c["size"] for c in mine)
    assert {(c["dt"], c["kind"]) for c in TRANSFER} == {(dt, k) for dt in K.DTYPES for k in ("box", "stored")}
    assert {c["dims"] for c in TRANSFER if c["kind"] == "box"} == {(1, 1, 1), (2, 1, 1), (13, 1, 1), (9, 7, 1), (7, 6, 5), (13, 11, 9), (16, 16, 16)}
    assert {c["nagg"] for c in TRANSFER if c["kind"] == "stored"} == {1, 255, 257, 700}
    assert {len(a) for name, a in K.scan_cases() if name.startswith("random")} == {1, 2, 1023, 1024, 1025, 2047, 2049, 5000}


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_special_lanes(dt):
    """the planted lanes hold what they are named for, and a step over them gives -0, infinities, NaNs, subnormals and exact ties"""
    dtype = K.DTYPES[dt]
    sp_ = K.specials(dtype)
    re = np.ascontiguousarray(sp_.real if R.is_complex(dtype) else sp_)
    Rt = R.real_type(dtype)
    tiny = np.finfo(Rt).tiny
    assert np.signbit(re[re == 0]).any() and np.isinf(re).any() and np.isnan(re).any() and ((re != 0) & (np.abs(re) < tiny)).any()
    p = 24 if Rt is np.float32 else 53
    a, b = Rt(re[0, 0]), Rt(re[0, 1])
    assert a * b == Rt(1 + 2.0 ** -(p // 2) + 2.0 ** -(p - p // 2))              # the half step 2^-p went down to even
    big = [c for c in SMOOTH if c["dt"] == dt and c["size"] == 257 and c["mode"] == 2 and c["store_d"]][0]
    inp = K.smooth_inputs(big)
    x, d = K.smooth_step(dtype, 2, inp["dinv"], inp["b"], inp["w"], inp["d"], inp["x"], inp["c0"], inp["c1"], 1)
    out = R.bits(x).view(Rt)
    assert np.isnan(out).any() and np.isinf(out).any() and ((out != 0) & (np.abs(out) < tiny)).any()


# ---- the scan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,counts", K.scan_cases(), ids=[n for n, _ in K.scan_cases()])
def test_scan_is_cumsum_where_nothing_overflows(name, counts):
    out, overflow = K.scan(counts)
    total = int(counts.astype(np.int64).sum())
    assert overflow == (total > K.INT_MAX) and out.dtype == np.int32 and out.size == counts.size + 1
    exact = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    assert np.array_equal(out, np.minimum(exact, K.INT_MAX))
    if not overflow:
        assert np.array_equal(out[1:], np.cumsum(counts)) and out[0] == 0
    else:
        assert out[-1] == K.INT_MAX and out.max() == K.INT_MAX


# ---- per-level data -----------------------------------------------------------------------------------------------------------------------
def test_smith_reciprocal_and_dinv():
    rng = np.random.default_rng(5)
    b = rng.standard_normal(400) + 1j * rng.standard_normal(400)
    got = K.smith_reciprocal(b)
    assert (np.abs(b.real) >= np.abs(b.imag)).any() and (np.abs(b.real) < np.abs(b.imag)).any()
    assert np.max(np.abs(got * b - 1)) < 8 * np.finfo(np.float64).eps
    want = np.empty(3, np.complex128)             # by hand, signs of the zeros included: (0 - -0) / -8 = -0
    want.real, want.imag = [0.5, 0.0, -0.125], [0.0, -0.25, -0.0]
    assert R.bit_equal(K.smith_reciprocal(np.array([2.0 + 0j, 0 + 4j, -8.0 + 0j])), want)
    # a diagonal stored twice is added in stored order before the division, and the result is rounded once
    ip, ix = np.array([0, 3, 4]), np.array([0, 1, 0, 1])
    da = np.array([0.1, 5.0, 0.2, 3.0], np.float32)
    want = np.array([1.0 / (np.float64(da[0]) + np.float64(da[2])), 1.0 / 3.0]).astype(np.float32)
    assert R.bit_equal(K.dinv_bits(ip, ix, da, np.float32), want)
    assert K.lmax_real(ip, da, want) == float(np.float64(want[0]) * ((np.float64(da[0]) + np.float64(da[1])) + np.float64(da[2])))
