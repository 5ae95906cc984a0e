"""The slab loop (csrc/slab.hip, CGAMD_DIST_RESIDENT) against its host restatement (tests/slab_ref.py), BIT FOR BIT, at small shapes:
x and every history entry of every call, np.array_equal on the raw bits, no tolerance.  Every case first compares
DistSolver.slab_plan() with the host copy of slab_plan / slab_partition, so the kernel instantiation a case launches is the one it
is written for, and asserts loop_launches() == 0 before and after its calls (no launch fell back).

One rank, flags = CGAMD_DIST_RESIDENT, index_codes_min_mb = 0, dev.slab_cus set by the case (the partition does not depend on the
card), resident_wide_min = 1 (calls shorter than 16 iterations take the slab loop), a non-zero first guess; every tuning key is restored
in `finally`.  delta_0 is no sum of the slab loop: cgamd_dist_set_rhs forms it with the launched loops' dot kernels, in an order this
module does not restate.  It is held to the host r0 . r0 within the bound of any double sum of the T-rounded products
(slab_ref.check_delta0) and then handed to the restatement, together with x0, r0 = b - A x0 and d0 = r0 restated on the host.

Cases (tests/slab_ref.py cases()): two and three members with a last member of one row, n at a multiple of 1024 and one past it,
periodic couplings between member 0 and the ragged last member; rows of 5, 6, 7 and 8 entries, far columns one and two members away,
the largest span slab_plan accepts (2044) and one entry more (not in use), rows of a lone diagonal and a row without entries
(cgamd_dist_create accepts such a matrix); 2, 4, 10 and 12 steps; 32, 33, 64, 65, 129 and the card's largest member count, with a
member below 32 that gathers from one above; calls of 1, 2, 3 and 17 iterations, chains of odd calls, two right-hand sides on one
handle; the trimmed members of a rank that is its own peer over the peer-to-peer mailboxes.

Kernel instantiations launched -- type x register budget x row unroll x {value-coded, streamed}: all 36 (slab_ref.ALL_FORMS).  Every
case records the form its slab_plan() reports; the last test of the module asserts that the recorded set is the whole set.  The row
unroll follows the longest row and LDS the largest 256-row span, so double and float2 reach the 12-step budget with unroll 7 on
6-entry rows and with unroll 8 on 5-entry rows of which a sparse set carries 8; 7 entries in every row do not fit there."""
import ctypes
import importlib

import numpy as np
import pytest

import slab_ref as S
import spmv_ref as R
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
RESIDENT = 512
DEFAULTS = {"index_codes_min_mb": 32, "resident_wide_min": 16, "dev.slab_cus": 0, "dev.slab_trim": -1, "dev.value_codes": 1}
CASES = S.cases()
LAUNCHED = {}           # case id -> (type, budget, unroll, value-coded) as slab_plan() reported it


def _tune(pkg, **kv):
    lib = pkg._lib.load()
    for k, v in kv.items():
        pkg._lib.check(lib.cgamd_tune(k.encode(), int(v)))


def _handle(pkg, ctx, c, sysd, cus):
    """the handle of a case, created under the case's tuning keys (a handle keeps the configuration it was created under)"""
    import torch
    dmod = importlib.import_module(PKG_NAME + ".dist")
    dev = torch.device("cuda", 0)
    n, dtype = c["n"], sysd["dtype"]
    vals = torch.from_numpy(sysd["da"]).to(dev)
    indptr = torch.from_numpy(sysd["ip"]).to(dev)
    try:
        _tune(pkg, **{"index_codes_min_mb": 0, "resident_wide_min": 1, "dev.slab_cus": cus, "dev.slab_trim": c["trim"],
                      "dev.value_codes": int(c["vc"])})
        if c["halo"]:
            h = c["halo"]
            plan = dmod.HaloPlan(0, 1, 0, n, n, h, torch.from_numpy(sysd["ix_local"]).to(dev), torch.arange(h), [0], [h], [h],
                                 torch.arange(h, dtype=torch.int32, device=dev))
            s = dmod.DistSolver(ctx, plan, indptr, vals, dtype, flags=RESIDENT, comm="p2p")
        else:
            plan = dmod.build_halo_plan(torch.from_numpy(sysd["ix"].astype(np.int64)).to(dev), [(0, n)], 0)
            s = dmod.DistSolver(ctx, plan, indptr, vals, dtype, flags=RESIDENT)
    finally:
        _tune(pkg, **DEFAULTS)
    s._test_keep = (vals, indptr, plan)
    return s


def _mismatch(got, ref):
    g, r = R.bits(got).reshape(len(got), -1), R.bits(ref).reshape(len(ref), -1)
    bad = np.nonzero(np.any(g != r, axis=1))[0]
    return f"{bad.size} of {len(got)} differ" + (f", first at {int(bad[0])}: {got[bad[0]]!r} != {ref[bad[0]]!r}" if bad.size else "")


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_slab_loop_bit_for_bit(pkg, gpu, cid):
    import torch
    ctx, queue, kernels = gpu
    dev = torch.device("cuda", 0)
    card = int(torch.cuda.get_device_properties(0).multi_processor_count)
    c = next(v for v in CASES if v["id"] == cid)
    if c["tag"] == "Gmax" and card < c["cus"]:
        c = S.members_cases(min(256, card), tag="Gmax")[0]
    if c["cus"] > card:
        pytest.skip(f"{c['cus']} members of 1024 rows need {c['cus']} CUs, the card has {card}")
    sysd = S.case_system(c)
    want = S.case_plan(c, sysd, card)
    assert want["in_use"] == int(c["in_use"])
    n, dtype = c["n"], sysd["dtype"]
    tdt = pkg.generators.torch_dtype(dtype)
    s = _handle(pkg, ctx, c, sysd, c["cus"])
    try:
        got = s.slab_plan()
        print(f"{c['id']}: plan {got}")
        assert got == want
        if not c["in_use"]:
            assert s.loop_launches() > 0
            return
        assert s.loop_launches() == 0
        LAUNCHED[cid] = (c["dt"], got["budget"], got["unroll"], got["value_coded"])
        # the cap convention of cgamd_dist_slab_plan: a buffer that is too small is left alone and the count needed comes back
        info, few = (ctypes.c_int * 8)(), (ctypes.c_int * (want["members"] + 1))(*([-7] * (want["members"] + 1)))
        assert pkg._lib.load().cgamd_dist_slab_plan(s.handle, info, few, want["members"]) == want["members"] + 1
        assert list(few) == [-7] * (want["members"] + 1) and list(info)[:2] == [1, want["members"]]
        outs = []
        for j, chain in enumerate(c["chains"]):
            b, x0 = sysd["rhs"][c["rhs_of"][j]]
            s.set_rhs(torch.from_numpy(b).to(dev), torch.from_numpy(x0).to(dev))
            for K in chain:
                s.iterate(K)
            x = s.x(torch.empty(n, dtype=tdt, device=dev)).cpu().numpy()
            hist = s.history().copy()
            assert s.loop_launches() == 0          # no launch fell back
            if c["halo"]:
                assert s.p2p_error() == 0
            assert len(hist) == sum(chain) + 1
            r0 = S.start_state(sysd["ip"], sysd["ix"], sysd["da"], b, x0, dtype)[1]
            print(f"{c['id']} calls {chain}: delta_0 error / bound = {S.check_delta0(hist[0], r0, dtype):.3g}")
            ref_x, ref_h = S.run_chain(sysd["ip"], sysd["ix"], sysd["da"], b, x0, want["member_start"], chain, dtype, delta0=hist[0])
            print(f"{c['id']} calls {chain}: history {_mismatch(hist, ref_h)}; x {_mismatch(x, ref_x)}")
            assert np.array_equal(R.bits(hist), R.bits(ref_h))
            assert np.array_equal(R.bits(x), R.bits(ref_x))
            outs.append((x, hist))
        # chains of one right-hand side and one total length: the state handed from launch to launch is the whole state
        for j in range(1, len(outs)):
            if c["rhs_of"][j] == c["rhs_of"][0] and sum(c["chains"][j]) == sum(c["chains"][0]):
                assert np.array_equal(R.bits(outs[j][0]), R.bits(outs[0][0])) and np.array_equal(R.bits(outs[j][1]), R.bits(outs[0][1]))
    finally:
        s.close()


def test_every_kernel_form_was_launched():
    """after the cases above: the forms their slab_plan() reported are all 36 instantiations of cg_slab_kernel"""
    forms = set(LAUNCHED.values())
    print(f"{len(LAUNCHED)} cases launched {len(forms)} kernel forms: {sorted(forms)}")
    assert set(LAUNCHED) == {c["id"] for c in CASES if c["in_use"]}, "this test follows a run of every case of test_slab_loop_bit_for_bit"
    assert forms == S.ALL_FORMS
