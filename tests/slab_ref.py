"""Host restatement of K iterations of the slab loop (csrc/slab.hip, CGAMD_DIST_RESIDENT) and of its plan -- pure numpy, no GPU --
built on the helpers of spmv_ref.py and cg_step_ref.py.

Why it can be exact
-------------------
As for every other loop (cg_step_ref.py): -ffp-contract=off, one rounding per multiply and per add in the value type T, sums in the
accumulator type (double, two doubles for complex64) in an order that timing cannot change.  The order of the slab loop is fixed by n,
the member starts and the CSR order alone: member m owns the rows [start[m], start[m + 1]) whatever CU it runs on, and with more than
32 members every XCD poller forms the same sum of the same G partials (resident_device.h xcd_scalars :190-229 hands the RESULT on).

Rules restated (file:line of the rule; slab.hip unless another file is named)
-----------------------------------------------------------------------------
row product     q_i = left-to-right sum in T from +0 of vfma(a, d, sum) = vadd(sum, vmul(a, d)) over the row's entries in CSR order
                (slab_row :183-187, slab_row_vc :207-211); a row without entries gives +0 (every select keeps `sum`).  Columns of the
                member's own rows come from its LDS copy of d, the others from the buffer of the iteration's parity, halo columns from
                its tail (:160-162, :176-184): the values are those of the same d, so the restatement reads one vector.
d.q             thread t of member m starts from +0 in the accumulator type and adds to_acc(vmul(d, q)) of its rows R0 + h 512 + t,
                h = 0 .. nsteps - 1 (:544-547): the product is rounded in T, then widened.  Rows past the member's end hold d = 0 and
                q = 0 (:393-396, rowinfo 0) and contribute to_acc(0 * 0).  wg_sum (resident_device.h :233-244): the wave tree per wave,
                then the eight wave sums added to wave 0's in order.
r.r             the same with to_acc(vmul(r, r)) (:561-569); rows past the end hold r = 0.
members         group_scalars (resident_device.h :116-152): lane t < G holds 0 + p[t] (:135), the wave tree over each 64 members, then
                ((w0 + w1) + w2) + w3 (:141-143).
rank            slab_rank_sum :220-256: one rank without peers returns `local`; a rank that is its own peer returns 0 + local.
scalars         dqT = T(sum), alpha = T(acc_div(double(delta), double(dqT))) (:554-555); dn = T(sum r.r),
                beta = T(acc_div(double(dn), double(delta_old))) (:426-427, :578-579); acc_div of complex values is Smith's algorithm
                (device_types.h), every product unconjugated.
element steps   in T: x = vadd(x, vmul(al, d)) (:565); r = vsub(r, vmul(al, q)) (:566); d = vaypx(bt, d, r) at the top of the iterations
                k > 0 (:442) and once more after the last one (:587) -- that value is what the launch writes back as the caller's d.
history         entry it0 + k is dn (:433, :594); delta = dn.

-0: the restatement pads the members to whole steps and the partials to 256 lanes with +0.  acc + (+0) == acc in every bit unless acc is
-0, and `0 + p` changes only p = -0; an accumulator that starts from +0 never becomes -0 under round-to-nearest.  `valid_inputs` asserts
that no accumulator, partial or sum of the chosen inputs is -0 and that no value formed in T is subnormal, infinite or NaN.

The plan (slab_plan :622-646, slab_partition :657-680, dist.cpp cgamd_dist_enable_resident) is restated by `host_plan`; the device
module compares DistSolver.slab_plan() with it before anything else.

Mutations (`Rules`): each switch replaces one rule by a plausible wrong one; tests/test_slab_ref.py proves on the CPU that every one of
them changes a compared bit (x or history) on an input the device module uses.
"""
import zlib

import numpy as np

import cg_step_ref as CS
import spmv_ref as R

STEP = 512            # rows per step (kSlabStep)
MAX_STEPS = 12        # kSlabRpt
DT = {"f32": np.float32, "f64": np.float64, "c64": np.complex64}


class Rules:
    """the rules of the module docstring; a mutation is a Rules with one switch changed"""
    def __init__(self, **kw):
        self.members = "tree"           # "sequential": member partials added 0, 1, 2, ... instead of through group_scalars' tree
        self.waves = "inorder"          # "pairwise": the eight wave sums of wg_sum added pairwise
        self.acc_in_T = False           # d.q and r.r of a member accumulated in T
        self.widen_first = False        # the product widened before it is rounded: to_acc(d) * to_acc(q)
        self.dq_unrounded = False       # d.q not rounded to T before the division
        self.uniform_members = False    # members of ceil(n / G) rows instead of the reported starts
        self.no_closing_d = False       # the d update after the last iteration left out
        self.d_before_r = False         # the d update takes r before, instead of after, the r update
        for k, v in kw.items():
            assert k in self.__dict__, k
            setattr(self, k, v)


EXACT = Rules()
MUTATIONS = {"members-sequential": Rules(members="sequential"), "waves-pairwise": Rules(waves="pairwise"), "acc-in-T": Rules(acc_in_T=True),
             "widen-first": Rules(widen_first=True), "dq-unrounded": Rules(dq_unrounded=True), "uniform-members": Rules(uniform_members=True),
             "no-closing-d": Rules(no_closing_d=True), "d-before-r": Rules(d_before_r=True)}


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def slab_plan(dtype, n, n_cus, max_row, max_span, coded=True):
    """slab.hip slab_plan :622-646 for a matrix the row-block SpMV takes (plan.kind == 5): None when the loop does not apply"""
    dtype = np.dtype(dtype)
    if n_cus < 8 or dtype == np.complex128 or not coded or max_row < 1 or max_row > 8:
        return None
    vs = dtype.itemsize
    rows_m = -(-n // n_cus)
    rows_m = -(-rows_m // (2 * STEP)) * (2 * STEP)
    if rows_m > MAX_STEPS * STEP:
        return None
    G = -(-n // rows_m)
    if G < 2 or G > 256:
        return None
    if max_span * 2 + 8 > 8 * 512:
        return None
    vcap = 8 * 512
    ccap = ((max_span * (rows_m // 256) + 8 + 15) & ~15) + 16
    lds = rows_m * vs + max(2 * vcap * vs + ccap, 2 * ccap) + 64
    if lds > 150 * 1024:
        return None
    steps = rows_m // STEP
    return {"in_use": 1, "members": G, "rows_m": rows_m, "steps": steps, "unroll": 5 if max_row <= 5 else 7 if max_row <= 7 else 8,
            "budget": 10 if steps <= 10 else 12}


def slab_partition(rows_m, n, boundary, trim, max_members):
    """slab.hip slab_partition :657-680: member starts [G + 1] (the last one granules * 1024), or None when more than max_members"""
    granules, cap_i = -(-n // 1024), rows_m // 1024
    cap_b = max(1, cap_i - trim)
    starts, g, members = [], 0, 0
    while g < granules:
        take = min(cap_i, granules - g)
        if any(boundary[g:g + take]):
            first_b = 0
            while not boundary[g + first_b]:
                first_b += 1
            take = first_b if first_b > 0 else min(cap_b, granules - g)
        starts.append(g * 1024)
        g += take
        members += 1
        if members > max_members:
            return None
    starts.append(granules * 1024)
    return starts


def boundary_granules(ip, ix, n, send_rows):
    """dist.cpp cgamd_dist_enable_resident :1267-1274: the 1024-row granules with a row that is sent to a peer, or with a 256-row block
    that reads a halo column (column >= n)"""
    out = np.zeros(-(-n // 1024), dtype=bool)
    out[np.asarray(send_rows, dtype=np.int64) >> 10] = True
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    out[rows[np.asarray(ix) >= n] >> 10] = True
    return out


def host_plan(dtype, n, n_cus, ip, value_coded, boundary=None, slab_trim=-1):
    """what DistSolver.slab_plan() must report.  boundary: the granule flags of a rank with peers (boundary_granules), None without"""
    spans, max_row = R.plan_spans(ip)
    p = slab_plan(dtype, n, n_cus, max_row, spans[0])
    if p is None:
        return {"in_use": 0, "members": 0, "rows_m": 0, "steps": 0, "unroll": 0, "budget": 0, "value_coded": 0, "uniform": 0, "member_start": []}
    p["value_coded"] = int(bool(value_coded))
    starts = None
    if boundary is not None and slab_trim != 0:
        want = slab_trim if slab_trim > 0 else 2
        for trim in range(min(want, p["rows_m"] // 1024 - 1), 0, -1):
            got = slab_partition(p["rows_m"], n, boundary, trim, min(n_cus, 256))
            if got is not None and len(got) - 1 >= 2:
                starts = got
                break
    p["uniform"] = int(starts is None)
    if starts is None:
        starts = [min(m * p["rows_m"], n) for m in range(p["members"] + 1)]
    p["members"] = len(starts) - 1
    p["member_start"] = [int(v) for v in starts]
    return p


def check_partition(starts, n, rows_m, boundary=None, trim=0):
    """the properties of a set of member starts, uniform (boundary None) or not"""
    s = np.asarray(starts, dtype=np.int64)
    assert s[0] == 0 and np.all(np.diff(s) > 0)
    assert np.all(s[:-1] % 1024 == 0)
    assert s[-2] < n <= s[-1] or s[-1] == n
    assert np.all(np.diff(s) <= rows_m)
    if boundary is not None:
        assert s[-1] % 1024 == 0
        cap_b = max(1, rows_m // 1024 - trim)
        for m in range(len(s) - 1):
            g0, g1 = s[m] // 1024, s[m + 1] // 1024
            if np.any(boundary[g0:g1]):
                assert g1 - g0 <= cap_b, (m, g0, g1)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def _member_sum(t, starts, n, rules, watch):
    """the G member partials of the terms t (n,): thread accumulators over the steps, then wg_sum"""
    s = np.asarray(starts, dtype=np.int64)
    G = len(s) - 1
    if rules.uniform_members:
        per = -(-n // G)
        s = np.minimum(np.arange(G + 1, dtype=np.int64) * per, n)
    r1 = np.minimum(s[1:], n)
    steps = max(1, int(-(-(r1 - s[:-1]).max() // STEP)))
    j = np.arange(steps * STEP, dtype=np.int64)[None, :]
    idx = s[:-1, None] + j
    ok = idx < r1[:, None]
    v = np.where(ok, t[np.where(ok, idx, 0)], np.zeros(1, t.dtype)).reshape(G, steps, STEP)
    acc = np.zeros((G, STEP), t.dtype)
    with np.errstate(all="ignore"):
        for h in range(steps):
            acc = acc + v[:, h]
    if watch is not None:
        watch.note_acc(acc)
    p = CS.block_sum(acc, CS.Rules(waves=rules.waves))
    return p.astype(np.complex128 if p.dtype.kind == "c" else np.float64)


def _group_sum(p, rules, watch):
    """group_scalars on the G partials, then the rank sum of one rank: a 0-d accumulator"""
    G = len(p)
    assert G <= 256
    with np.errstate(all="ignore"):
        if rules.members == "sequential":
            s = np.zeros((), p.dtype)
            for m in range(G):
                s = s + p[m]
        else:
            v = np.zeros(256, p.dtype)
            v[:G] = np.zeros((), p.dtype) + p
            s = CS.block_sum(v.reshape(1, 256))[0]
        s = np.zeros((), p.dtype) + s
    if watch is not None:
        watch.note_acc(p)
        watch.note_acc(np.asarray(s).reshape(1))
    return np.asarray(s).reshape(1)


def _terms(ops, a, b, rules):
    if rules.widen_first:
        with np.errstate(all="ignore"):
            return (CS.to_acc(a) * CS.to_acc(b))[0]
    return ops.terms(a, b)[0]


def iterate(ip, ix, da, x, r, d, delta, starts, K, dtype, rules=EXACT, watch=None):
    """K iterations of one launch from the state (x, r, d, delta) -- d is the caller's d, already beta d + r -- over the matrix
    (ip, ix, da) of n rows; a halo column is named by its owner row.  Returns (x, r, d, delta, [the K history entries])."""
    dtype = np.dtype(dtype)
    n = len(ip) - 1
    ops = CS.Ops(dtype, CS.Rules(acc_in_T=rules.acc_in_T), watch)
    x, r, d = (np.array(v, dtype=dtype).reshape(1, n) for v in (x, r, d))
    dlt = np.array(delta, dtype=dtype).reshape(1)
    hist, r_prev = [], r

    def scalar(t):
        return _group_sum(_member_sum(t, starts, n, rules, watch), rules, watch)

    def beta_step(rr):
        dn = CS.from_acc(rr, dtype)
        bt = CS.quotient(dn, dlt, dtype)
        if watch is not None:
            watch.note_T(dn)
            watch.note_T(bt)
        hist.append(dn[0])
        return dn, bt

    rr = None
    for k in range(K):
        if k > 0:
            dlt_new, bt = beta_step(rr)
            d = ops.aypx(bt, d, r_prev if rules.d_before_r else r)
            dlt = dlt_new
        q = R.spmv_in_type(ip, ix, da, d, dtype, 1)
        if watch is not None:
            watch.note_T(q)
        dq = scalar(_terms(ops, d, q, rules))
        dqT = dq if rules.dq_unrounded else CS.from_acc(dq, dtype)
        al = CS.from_acc(CS.acc_div(CS.to_acc(dlt), CS.to_acc(dqT)), dtype)
        if watch is not None:
            watch.note_T(al)
        x = ops.axpy(x, al, d)
        r_prev = r
        r = ops.axmy(r, al, q)
        rr = scalar(_terms(ops, r, r, rules))
    dlt_new, bt = beta_step(rr)
    if not rules.no_closing_d:
        d = ops.aypx(bt, d, r_prev if rules.d_before_r else r)
    return x[0], r[0], d[0], dlt_new[0], hist


def start_state(ip, ix, da, b, x0, dtype):
    """x, r, d of cgamd_dist_set_rhs (dist.cpp): r = vsub(b, A x0) with the row sums of every one-lane-per-row SpMV, d = r.  delta_0 is
    formed by the launched loops' dot kernels (cg_step_ref.py holds those); the device module reads it from history[0]."""
    dtype = np.dtype(dtype)
    n = len(ip) - 1
    x = np.array(x0, dtype=dtype).reshape(1, n)
    q = R.spmv_in_type(ip, ix, da, x, dtype, 1)
    r = CS.Ops(dtype).sub(np.asarray(b, dtype=dtype).reshape(1, n), q)
    return x[0], r[0], r[0].copy()


def delta0_host(r, dtype):
    """r.r for the host tests (any order: they compare mutations with the exact rules from the same start)"""
    t = CS.Ops(dtype).terms(r.reshape(1, -1), r.reshape(1, -1))[0]
    return CS.from_acc(np.asarray(t.sum()).reshape(1), dtype)[0]


def run_chain(ip, ix, da, b, x0, starts, chain, dtype, delta0=None, rules=EXACT, watch=None):
    """set_rhs, then one launch per entry of `chain`: (x, history with entry 0 = delta0)"""
    x, r, d = start_state(ip, ix, da, b, x0, dtype)
    dlt = delta0_host(r, dtype) if delta0 is None else np.dtype(dtype).type(delta0)
    hist = [dlt]
    for K in chain:
        x, r, d, dlt, h = iterate(ip, ix, da, x, r, d, dlt, starts, K, dtype, rules, watch)
        hist += h
    return x, np.array(hist, dtype=dtype)


def check_delta0(got, r, dtype):
    """delta_0 of cgamd_dist_set_rhs is no slab-loop sum: the launched loops' dot kernels form it, in an order this module does not
    restate.  Whatever the order, it is T(a double sum of the n terms to_acc(vmul(r_i, r_i))): cg_step_ref.check_sum's bound,
    (gamma_n(u_D) + gamma_n(u_ext)) sum |t_i| + u_T |sum| per component, against their longdouble sum.  Returns error / bound."""
    r = np.asarray(r, dtype=dtype).reshape(1, -1)
    return CS.check_sum(np.asarray(got, dtype=dtype).reshape(1), CS.Ops(dtype).terms(r, r), dtype, "delta_0")


def valid_inputs(ip, ix, da, b, x0, starts, chain, dtype, delta0=None):
    w = CS.Watch()
    run_chain(ip, ix, da, b, x0, starts, chain, dtype, delta0, EXACT, w)
    assert w.seen > 0 and w.neg_zero == 0 and w.bad_T == 0, (w.seen, w.neg_zero, w.bad_T)


# ---- matrices: symmetric, diagonally dominant, from a list of offsets ---------------------------------------------------------------------
def build_matrix(n, offs, dtype, vc, seed, periodic=False, extra=(), lone=(), empty=()):
    """row i couples with i + o for every o of `offs` (positive; band: where i + o < n; periodic: (i + o) mod n) and carries a diagonal
    that dominates; both entries of a symmetric pair hold the same value (complex types: complex symmetric).  extra: (rows, o) pairs,
    further couplings of the given rows only.  lone: rows that keep their diagonal alone; empty: rows without a stored entry.
    Entries of a row in the order of their offsets (-o ... 0 ... +o, a wrapped column where its offset puts it).  vc: every value from a
    palette (off-diagonal -k / 8, k = 3 .. 8; diagonal: the row's sum of moduli of the real parts + 1, a multiple of 1 / 8): fewer than
    256 distinct values; else values random per symmetric pair."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    cplx = dtype.kind == "c"
    rows, cols, keys, vals = [], [], [], []
    drop = np.zeros(n, dtype=bool)
    drop[list(lone) + list(empty)] = True
    for which, (rsel, o) in enumerate([(None, o) for o in offs] + list(extra)):
        i = np.arange(n, dtype=np.int64) if rsel is None else np.asarray(rsel, dtype=np.int64)
        if periodic:
            j = (i + o) % n
        else:
            i = i[i + o < n]
            j = i + o
        keep = ~(drop[i] | drop[j])
        i, j = i[keep], j[keep]
        if vc:
            v = -rng.integers(3, 9, i.size) / 8.0
            v = v * (1 + 0.25j) if cplx else v
        else:
            v = -rng.uniform(0.25, 1.0, i.size)
            v = v * (1 + 1j * rng.uniform(-0.3, 0.3, i.size)) if cplx else v
        key = o if which < len(offs) else o + 0.5       # an extra coupling sorts behind the regular offset next to it
        rows += [i, j]
        cols += [j, i]
        keys += [np.full(i.size, key), np.full(i.size, -key)]
        vals += [v, v]
    rows, cols, keys, vals = (np.concatenate(v) for v in (rows, cols, keys, vals))
    weight = np.zeros(n)
    np.add.at(weight, rows, np.abs(vals.real) if vc else np.abs(vals))
    di = np.nonzero(~np.isin(np.arange(n), list(empty)))[0]
    if vc:
        dv = (weight[di] + 1.0) + (0.5j if cplx else 0.0)
    else:
        dv = weight[di] + rng.uniform(0.5, 1.5, di.size) + (0.2j * rng.uniform(-1, 1, di.size) if cplx else 0.0)
    rows, cols, keys, vals = (np.concatenate(v) for v in ((rows, di), (cols, di), (keys, np.zeros(di.size)), (vals, dv)))
    order = np.lexsort((keys, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    ip = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=ip[1:])
    return ip, cols.astype(np.int32), vals.astype(dtype)


def vectors(n, dtype, seed):
    """right-hand side and first guess with spread magnitudes (cg_step_ref.spread; every 256 rows scaled by a power of two of their
    own), so that the order of every sum shows in its bits"""
    rng = np.random.default_rng(seed ^ 0x5EED)
    block = np.repeat(np.exp2(rng.integers(-8, 9, -(-n // 256))), 256)[:n].astype(R.real_type(dtype))
    return CS.spread(rng, n, dtype) * block, CS.spread(rng, n, dtype, half=8)


# ---- the cases of tests/test_gpu_slab_bits.py ----------------------------------------------------------------------------------------------
BAND = (1, 40)
SEVEN = (1, 1300, 2500)


def _span_extra(count):
    """`count` rows of the first 256-row block of a periodic 7-per-row matrix take an eighth entry (their partners, 4096 rows on, too):
    the block's span is 1792 + count"""
    return [(np.arange(count), 4096)]


def _case(group, dt, n, offs, vc, cus, chains=((3,),), **kw):
    c = {"group": group, "dt": dt, "n": n, "offs": tuple(offs), "vc": bool(vc), "cus": cus, "chains": tuple(tuple(v) for v in chains),
         "periodic": False, "extra": (), "lone": (), "empty": (), "halo": 0, "trim": -1, "in_use": True, "tag": "", "rhs_of": None}
    c.update(kw)
    c["rhs_of"] = tuple(c["rhs_of"] or (0,) * len(c["chains"]))
    c["id"] = "-".join(str(v) for v in (group, c["tag"], dt, n if c["tag"] != "Gmax" else "", "vc" if vc else "st", f"cus{cus}", "x".join("+".join(map(str, ch)) for ch in c["chains"]))
                       if v != "")
    c["seed"] = zlib.crc32(c["id"].encode())
    return c


def members_cases(G, tag=None):
    """n = 1024 G - 300 rows in G members of 1024 rows"""
    n = 1024 * G - 300
    far = {33: 32 * 1024 + 100, 65: 40 * 1024 + 17}.get(G)
    offs = (1, 1100) + ((far,) if far else ())
    out = [_case("members", "f64", n, offs, False, G, tag=tag or f"G{G}")]
    if far:
        out.append(_case("members", "c64", n, offs, True, G, tag=tag or f"G{G}"))
    return out


def cases(card_cus=256):
    """card_cus: the CU count of the card (the largest member count is made for it)"""
    out = []
    gmax = min(256, card_cus)
    # minimal and ragged: two members, the last owns one row; exact multiples of 1024 and one past; periodic: member 0 gathers from the
    # ragged last member and the last member from member 0
    for dt in ("f64", "f32", "c64"):
        for vc in (True, False):
            for n in (1025, 2048, 2049, 3000):
                out.append(_case("ragged", dt, n, BAND, vc, 8))
            out.append(_case("ragged", dt, 2049, BAND, vc, 8, periodic=True, tag="periodic"))
    # row unroll
    sparse8 = [(np.arange(100, 9000, 97), 777)]
    for dt, vc in ((dt, vc) for dt in ("f64", "f32", "c64") for vc in (False, True)):
        out.append(_case("unroll", dt, 5000, (1, 64), vc, 8, tag="five"))                               # unroll 5
        out.append(_case("unroll", dt, 8000, SEVEN, vc, 8, tag="seven"))                                # unroll 7, far columns 1 and 2 members away
        out.append(_case("unroll", dt, 5000, (1, 64), vc, 8, extra=[(np.arange(2500), 2500)], tag="six"))  # row i couples with i +- 2500: 6 per row
        out.append(_case("unroll", dt, 9100, SEVEN, vc, 16, periodic=True, extra=sparse8, tag="eight"))  # max_row 8
    for dt, vc in (("f64", False), ("f32", True)):
        out.append(_case("unroll", dt, 9000, SEVEN, vc, 16, periodic=True, extra=_span_extra(252), tag="span2044"))
        out.append(_case("unroll", dt, 9000, SEVEN, vc, 16, periodic=True, extra=_span_extra(253), tag="span2045", in_use=False))
        out.append(_case("unroll", dt, 5000, SEVEN[:2] + (2100,), vc, 8, lone=(0, 511, 512, 1023, 1024, 3000, 4999), tag="lone"))
        out.append(_case("unroll", dt, 5000, SEVEN[:2] + (2100,), vc, 8, lone=(1024, 4999), empty=(2047,), tag="empty"))
    # register budget and steps (dev.slab_cus = 8)
    sparse = np.arange(100, 40000, 97)
    for n in (7681, 16000):
        out.append(_case("steps", "f64", n, (1, 64), False, 8, chains=((2,),)))
    for n in (40001, 45000):
        out.append(_case("steps", "f64", n, (1, 64), False, 8, chains=((2,),)))
        out.append(_case("steps", "f32", n, (1, 64), True, 8, chains=((2,),)))
    # the other forms of the 12-step budget that fit LDS (8-byte values: rows of at most 6 entries, which take unroll 7)
    for dt in ("f64", "c64"):
        for vc in (False, True):
            out.append(_case("steps", dt, 45000, (1, 64), vc, 8, chains=((2,),), extra=[(np.arange(22500), 22500)], tag="six"))
            # unroll follows the LONGEST row, LDS the largest span: 5-entry rows of which a sparse set takes three more couplings
            out.append(_case("steps", dt, 45000, (1, 64), vc, 8, chains=((2,),), extra=[(sparse, o) for o in (777, 1500, 3100)], tag="eight"))
    for dt, vc in (("f64", True), ("f32", False), ("c64", True), ("c64", False)):
        out.append(_case("steps", dt, 45000, (1, 64), vc, 8, chains=((2,),)))
    for vc in (False, True):
        out.append(_case("steps", "f32", 45000, SEVEN, vc, 8, chains=((2,),), tag="seven"))
        out.append(_case("steps", "f32", 45000, SEVEN, vc, 8, chains=((2,),), periodic=True, extra=[(np.arange(100, 40000, 97), 777)], tag="eight"))
    # member counts: 1024-row members; at 33 and 65 member 0 gathers from a member >= 32 (the second depmask word); the last one is the
    # largest count the card hosts
    for G in (32, 33, 64, 65, 129):
        out += members_cases(G)
    if gmax not in (32, 33, 64, 65, 129):
        out += members_cases(gmax, tag="Gmax")
    # call structure
    for K in (1, 2, 3, 17):
        out.append(_case("calls", "f64", 8000, SEVEN, False, 8, chains=((K,),)))
    out.append(_case("calls", "f64", 8000, SEVEN, False, 8, chains=((3, 1, 2), (6,)), tag="chain"))
    out.append(_case("calls", "f32", 8000, SEVEN, True, 8, chains=((3, 1, 2), (6,)), tag="chain"))
    out.append(_case("calls", "c64", 8000, SEVEN, False, 8, chains=((1, 1, 1), (3,)), tag="chain"))
    out.append(_case("calls", "f64", 8000, SEVEN, False, 8, chains=((3,), (2,)), rhs_of=(0, 1), tag="tworhs"))
    # members of unequal size: the rank as its own peer
    for dt in ("f64", "c64"):
        out.append(_case("unequal", dt, 25000, (1, 40, 1300), False, 8, chains=((5,), (3, 2)), periodic=True, halo=1500, trim=2))
    return out


MAX_CUS = 256
# every instantiation of cg_slab_kernel: (type, register budget, row unroll, value-coded); the cases launch all of them
ALL_FORMS = {(dt, b, u, v) for dt in DT for b in (10, 12) for u in (5, 7, 8) for v in (0, 1)}


def form(c, plan):
    return (c["dt"], plan["budget"], plan["unroll"], plan["value_coded"])


def case_cus(c, card_cus):
    """the CU count the plan of a case is made for on a card of card_cus CUs"""
    return min(card_cus, c["cus"])


def case_system(c):
    """matrix, vectors and (halo cases) the boundary flags of a case.  A halo case routes the entries of rows >= h at columns < h
    through the halo: local column n + c; `ix` keeps the owner row, `ix_local` is what the device gets."""
    dtype = DT[c["dt"]]
    ip, ix, da = build_matrix(c["n"], c["offs"], dtype, c["vc"], c["seed"], c["periodic"], c["extra"], c["lone"], c["empty"])
    sysd = {"ip": ip, "ix": ix, "da": da, "ix_local": ix, "boundary": None, "dtype": dtype}
    if c["halo"]:
        n, h = c["n"], c["halo"]
        rows = np.repeat(np.arange(n), np.diff(ip))
        route = (ix < h) & (rows >= h)
        sysd["ix_local"] = np.where(route, n + ix, ix).astype(np.int32)
        sysd["boundary"] = boundary_granules(ip, sysd["ix_local"], n, np.arange(h))
    # (chain j of a case runs on right-hand side rhs_of[j], on the one handle)
    sysd["rhs"] = [vectors(c["n"], dtype, c["seed"] + k) for k in range(max(c["rhs_of"]) + 1)]
    return sysd


def case_plan(c, sysd, card_cus=MAX_CUS):
    return host_plan(sysd["dtype"], c["n"], case_cus(c, card_cus), sysd["ip"], c["vc"], sysd["boundary"], c["trim"])
