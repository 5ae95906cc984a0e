"""CPU tests of tests/slab_ref.py, the host restatement of the slab loop (csrc/slab.hip) that tests/test_gpu_slab_bits.py holds the
device to bit for bit: it computes CG (against the fp64 oracle and, where every sum is exact, against a plain numpy CG), every
mutation of its rules changes a compared bit on an input of the device module, and its copy of the plan has the properties the kernel
relies on."""
import numpy as np
import pytest

import cg_oracle
import slab_ref as S
import spmv_ref as R

CASES = {c["id"]: c for c in S.cases()}

# mutation -> the case of the device module whose bits (x or history) it changes
COVER = {"members-sequential": "ragged-f64-2049-st-cus8-3",
         "waves-pairwise": "ragged-f64-1025-st-cus8-3",
         "acc-in-T": "ragged-f32-3000-vc-cus8-3",
         "widen-first": "ragged-c64-2049-vc-cus8-3",
         "dq-unrounded": "ragged-f32-2048-st-cus8-3",
         "uniform-members": "ragged-f64-3000-vc-cus8-3",
         "no-closing-d": "calls-chain-f64-8000-st-cus8-3+1+2x6",
         "d-before-r": "unroll-seven-f64-8000-st-cus8-3"}


def _run(c, rules=S.EXACT, dtype=None):
    sysd = S.case_system(c)
    plan = S.case_plan(c, sysd)
    dtype = dtype or sysd["dtype"]
    out = []
    for j, chain in enumerate(c["chains"]):
        b, x0 = sysd["rhs"][c["rhs_of"][j]]
        out.append(S.run_chain(sysd["ip"], sysd["ix"], sysd["da"].astype(dtype), b.astype(dtype), x0.astype(dtype), plan["member_start"], chain,
                               dtype, rules=rules))
    return sysd, plan, out


def test_case_ids_are_unique_and_every_input_is_valid():
    cs = S.cases()
    assert len({c["id"] for c in cs}) == len(cs)
    for c in cs:
        if not c["in_use"]:
            continue
        sysd = S.case_system(c)
        plan = S.case_plan(c, sysd)
        assert R.distinct_offsets(sysd["ip"], sysd["ix_local"]) <= 256
        if c["vc"]:
            assert R.distinct_values(sysd["da"]) <= 256
        for j, chain in enumerate(c["chains"]):
            b, x0 = sysd["rhs"][c["rhs_of"][j]]
            S.valid_inputs(sysd["ip"], sysd["ix"], sysd["da"], b, x0, plan["member_start"], chain, sysd["dtype"])


@pytest.mark.parametrize("cid,wide", [("unroll-seven-f64-8000-st-cus8-3", np.float64), ("calls-chain-c64-8000-st-cus8-1+1+1x3", np.complex128)])
def test_restatement_is_cg(cid, wide):
    """in fp64 / complex128 arithmetic the restatement agrees with the oracle at the standard tolerance (delta_k 1e-10, x 1e-9)"""
    c = CASES[cid]
    sysd, plan, out = _run(c, dtype=wide)
    b, x0 = sysd["rhs"][0]
    for chain, (x, hist) in zip(c["chains"], out):
        K = sum(chain)
        xo, ho = cg_oracle.cg(sysd["ip"], sysd["ix"], sysd["da"].astype(wide), b.astype(wide), x0=x0.astype(wide), n_iterations=K,
                              mode=cg_oracle.MODE_FAST)
        assert len(hist) == K + 1
        assert np.max(np.abs(hist - ho[:, 0]) / np.abs(ho[:, 0])) < 1e-10
        assert np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-9


def _exact_system(n, seed):
    """integers throughout and alpha a power of two: every product and every sum of the first iteration is exact in double, in any order"""
    rng = np.random.default_rng(seed)
    ip, ix, _ = S.build_matrix(n, (1, 40, 1300), np.float64, True, seed, periodic=True)
    rows = np.repeat(np.arange(n), np.diff(ip))
    da = np.where(ix == rows, 9.0, -rng.integers(1, 3, ix.size).astype(np.float64))
    da = np.where(ix > rows, da, 0.0)                     # keep the upper triangle, mirror it: symmetric with integer entries
    low = {(int(i), int(j)): v for i, j, v in zip(rows[ix > rows], ix[ix > rows], da[ix > rows])}
    da = np.array([9.0 if i == j else low[(min(i, j), max(i, j))] for i, j in zip(rows.tolist(), ix.tolist())])
    # r0 = b (x0 = 0 would make x trivial: x0 integer, b = r + A x0): entries +-1, some 0 and +-2 so that r.r = 4096
    r = rng.choice([-1.0, 1.0], n)
    m = (4096 - n) % 3
    z = {0: 0, 1: 2, 2: 1}[m]                             # n - z + 3 k = 4096
    k = (4096 - n + z) // 3
    assert n - z + 3 * k == 4096 and k >= 0
    r[1:1 + z] = 0.0
    r[1 + z:1 + z + k] *= 2.0

    def mul(v):
        q = np.zeros(n)
        np.add.at(q, rows, da * v[ix])
        return q
    dq = float(r @ mul(r))
    diag0 = np.nonzero((rows == 0) & (ix == 0))[0][0]
    da[diag0] += 65536.0 - dq                             # r[0] = +-1: d.q = 2^16, alpha = 2^-4
    assert r @ mul(r) == 65536.0 and da[diag0] > 9.0
    x0 = rng.integers(-3, 4, n).astype(np.float64)
    return ip, ix, da, r + mul(x0), x0, mul


@pytest.mark.parametrize("starts", [[0, 1024, 2048, 3000], [0, 2048, 3000], [0, 1024, 3000]])
def test_first_iteration_equals_plain_cg_where_sums_are_exact(starts):
    n = 3000
    ip, ix, da, b, x0, mul = _exact_system(n, 7)
    x, r, d = S.start_state(ip, ix, da, b, x0, np.float64)
    delta0 = np.float64(r @ r)
    assert delta0 == 4096.0
    xs, rs, ds, dlt, hist = S.iterate(ip, ix, da, x, r, d, delta0, starts, 1, np.float64)
    # the textbook iteration in numpy
    q = mul(r)
    alpha = delta0 / (r @ q)
    x1 = x0 + alpha * r
    r1 = r - alpha * q
    delta1 = r1 @ r1
    assert alpha == 2.0 ** -4
    assert R.bit_equal(xs, x1) and R.bit_equal(rs, r1)
    assert hist[0] == delta1 and dlt == delta1
    assert R.bit_equal(ds, r1 + (delta1 / delta0) * r)


@pytest.mark.parametrize("name", sorted(S.MUTATIONS))
def test_every_mutation_changes_a_compared_bit(name):
    c = CASES[COVER[name]]
    assert c["in_use"]
    _, _, exact = _run(c)
    _, _, mutant = _run(c, S.MUTATIONS[name])
    same = all(R.bit_equal(a[0], m[0]) and R.bit_equal(a[1], m[1]) for a, m in zip(exact, mutant))
    print(f"mutation {name}: case {c['id']}: bits {'unchanged' if same else 'changed'}")
    assert not same, f"mutation {name} changes no compared bit of case {c['id']}"


def test_mutation_table_is_complete():
    assert set(COVER) == set(S.MUTATIONS) and len(S.MUTATIONS) >= 8


def test_uniform_plans():
    for c in S.cases():
        if c["halo"]:
            continue
        sysd = S.case_system(c)
        plan = S.case_plan(c, sysd)
        assert plan["in_use"] == int(c["in_use"]), c["id"]
        if not plan["in_use"]:
            assert plan["member_start"] == []
            continue
        assert plan["uniform"] == 1 and plan["rows_m"] % 1024 == 0 and plan["steps"] == plan["rows_m"] // 512
        assert plan["budget"] == (10 if plan["steps"] <= 10 else 12) and plan["steps"] <= 12
        assert 2 <= plan["members"] <= min(256, c["cus"])
        assert len(plan["member_start"]) == plan["members"] + 1 and plan["member_start"][-1] == c["n"]
        S.check_partition(plan["member_start"], c["n"], plan["rows_m"])


def test_plan_thresholds():
    # unroll by the longest row; the span limit max_span * 2 + 8 <= 4096; more rows than 12 steps of 8 members; fewer than 8 CUs
    assert [S.slab_plan(np.float64, 5000, 8, r, 1000)["unroll"] for r in range(1, 9)] == [5, 5, 5, 5, 5, 7, 7, 8]
    assert S.slab_plan(np.float64, 5000, 8, 9, 1000) is None and S.slab_plan(np.float64, 5000, 8, 0, 1000) is None
    assert S.slab_plan(np.float32, 9000, 16, 8, 2044) is not None and S.slab_plan(np.float32, 9000, 16, 8, 2045) is None
    assert S.slab_plan(np.float64, 8 * 6144, 8, 5, 1283)["steps"] == 12 and S.slab_plan(np.float64, 8 * 6144 + 1, 8, 5, 1283) is None
    assert S.slab_plan(np.float64, 5000, 7, 5, 1283) is None and S.slab_plan(np.complex128, 5000, 8, 5, 1283) is None
    assert S.slab_plan(np.float64, 1024, 8, 5, 1283) is None           # one member would do
    # LDS: 12 steps of 7-entry rows fit in single precision, not in double
    assert S.slab_plan(np.float32, 45000, 8, 7, 1795)["budget"] == 12 and S.slab_plan(np.float64, 45000, 8, 7, 1795) is None


def test_trimmed_partition():
    c = CASES["unequal-f64-25000-st-cus8-5x3+2"]
    sysd = S.case_system(c)
    plan = S.case_plan(c, sysd)
    b = sysd["boundary"]
    assert b.tolist() == [g in (0, 1, 2, 23, 24) for g in range(25)]
    assert plan["in_use"] == 1 and plan["uniform"] == 0 and plan["rows_m"] == 4096
    assert plan["member_start"] == [0, 2048, 4096, 8192, 12288, 16384, 20480, 23552, 25600]
    S.check_partition(plan["member_start"], c["n"], plan["rows_m"], b, 2)
    # every boundary granule sits in a member of at most rows_m / 1024 - trim granules; interior members stop short of a boundary
    # granule; too few CUs for the trimmed members: equal members
    assert S.slab_partition(4096, 25000, b, 2, 7) is None
    assert S.host_plan(np.float64, 25000, 8, sysd["ip"], False, b, 0)["uniform"] == 1
    one = S.slab_partition(4096, 25000, b, 1, 256)
    S.check_partition(one, 25000, 4096, b, 1)
    assert one[:3] == [0, 3072, 7168]


def test_cases_reach_every_kernel_form():
    """type x register budget x row unroll x {value-coded, streamed}: all 36.  The unroll follows the longest row and LDS the largest
    256-row span, so the 12-step forms of the 8-byte types take unroll 7 from 6-entry rows and unroll 8 from 5-entry rows of which a
    few carry 8; with 7 entries in EVERY row they do not fit (slab_plan refuses)."""
    forms = set()
    for c in S.cases():
        if c["in_use"]:
            forms.add(S.form(c, S.case_plan(c, S.case_system(c))))
    assert forms == S.ALL_FORMS and len(S.ALL_FORMS) == 36
    for dt in (np.float64, np.complex64):
        assert S.slab_plan(dt, 45000, 8, 6, 1539)["unroll"] == 7 and S.slab_plan(dt, 45000, 8, 7, 1795) is None
