"""Host restatement of the kernels of the multigrid V-cycle and of the setup's scan (csrc/multigrid.hip, csrc/amg.hip) and of the
launch chain of one cycle (mg_walk in csrc/multigrid_setup.cpp) -- pure numpy, no GPU.  include/cgamd.h "Multigrid: the kernels"
states the contract; this file is that contract as code.

Why it can be exact: the library is compiled without contraction, so every operation of the three cycle kernels is ONE IEEE operation
in the value type T.  Complex values are (re, im) pairs in the real type of T: the product by components as spmv_ref.vmul_t forms it
(never numpy's complex product), sums and differences by components, a scale by c0, c1 or omega multiplies both components by the
coefficient ROUNDED TO THE REAL TYPE FIRST.  numpy's float32 / float64 array operations are such IEEE operations, so the results can
be compared with the device's bit for bit.  The one thing IEEE leaves open is which NaN an operation returns (sign and payload); the
device tests therefore require a NaN wherever this file has one and compare every other lane in all its bits.

Besides the kernels as they are, every function takes `rules`: the same kernel with ONE thing done differently (members summed in
descending order, t + c0 d for c0 d + t, a contracted multiply-add).  tests/test_mg_kernel_ref.py shows on the inputs of the device
tests which of these change bits -- so that a device kernel that did them would fail -- and which cannot."""
import fractions
import zlib

import numpy as np

import mg_ref
import spmv_ref as R

WIDTH = 8                       # kAmgWidth: ints per member list
SCAN_BLOCK = 1024               # threads of mg_scan_kernel
INT_MAX = 2 ** 31 - 1
DTYPES = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
CODE = {"f32": 0, "f64": 1, "c64": 2, "c128": 3}


class Rules:
    def __init__(self, members="ascending", later="c0d+t", contract=False):
        self.members, self.later, self.contract = members, later, contract


EXACT = Rules()


# ---- arithmetic on (re, im) pairs ---------------------------------------------------------------------------------------------------------
def parts(v, dtype):
    return R._parts(v, dtype)


def join(p, dtype):
    return R._join(p[0], p[1], dtype)


def _add(a, b):
    return a[0] + b[0], None if a[1] is None else a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], None if a[1] is None else a[1] - b[1]


def coefficient(c, dtype):
    """a double coefficient as the launches round it: to the real type of T"""
    return R.real_type(dtype)(c)


def _scale(c, a):
    return c * a[0], None if a[1] is None else c * a[1]


def _round_fraction(q, Rt):
    """the exact rational q rounded once to the real type Rt, nearest-even (finite values)"""
    f = Rt(float(q))                                    # within one step of the answer: float() is correctly rounded to double
    best, err = None, None
    for c in (np.nextafter(f, Rt(-np.inf)), f, np.nextafter(f, Rt(np.inf))):
        if not np.isfinite(c):
            continue
        e = abs(fractions.Fraction(float(c)) - q)
        even = int(np.array([c]).view({4: np.uint32, 8: np.uint64}[Rt(0).itemsize])[0]) % 2 == 0
        if best is None or e < err or (e == err and even):
            best, err = c, e
    return best


def _fma(c, a, b):
    """round(c * a + b) with ONE rounding, lane by lane (finite lanes; others as the two-rounding form): what a contracted
    multiply-add returns"""
    Rt = a.dtype.type
    out = c * a + b
    flat_a, flat_b, flat_o = a.reshape(-1), b.reshape(-1), out.reshape(-1)
    for i in range(flat_a.size):
        if np.isfinite(flat_a[i]) and np.isfinite(flat_b[i]) and np.isfinite(flat_o[i]):
            q = fractions.Fraction(float(c)) * fractions.Fraction(float(flat_a[i])) + fractions.Fraction(float(flat_b[i]))
            r = _round_fraction(q, Rt)
            if r is not None and (r != 0 or q != 0):        # (an exact zero keeps the sign the two-rounding form gave it)
                flat_o[i] = r
    return out


# ---- the three cycle kernels --------------------------------------------------------------------------------------------------------------
def smooth_step(dtype, mode, dinv, b, w, d, x, c0, c1, store_d, rules=EXACT):
    """mg_cheb_kernel on (nrhs, size) arrays (dinv: (size,)): returns (x_new, d_new); d_new is None when store_d is 0 (d is not
    written).  w is not looked at in mode 0, d not unless the mode is 2, x not in mode 0"""
    with np.errstate(all="ignore"):
        res = parts(b, dtype)
        if mode != 0:
            res = _sub(res, parts(w, dtype))
        di = parts(dinv, dtype)
        t = R.vmul_t((di[0][None, :], None if di[1] is None else di[1][None, :]), res, dtype)
        t = _scale(coefficient(c1, dtype), t)
        if mode == 2:
            k0, dp = coefficient(c0, dtype), parts(d, dtype)
            if rules.contract:
                t = (_fma(k0, dp[0], t[0]), None if t[1] is None else _fma(k0, dp[1], t[1]))
            elif rules.later == "t+c0d":
                t = _add(t, _scale(k0, dp))
            else:
                t = _add(_scale(k0, dp), t)
        xn = t if mode == 0 else _add(parts(x, dtype), t)
    return join(xn, dtype), (join(t, dtype) if store_d else None)


def box_members(dims):
    """the member lists of the box map of a grid: (n_coarse, 8), fine rows ascending (x fastest, then y, then z), -1 behind the last"""
    return members_of(mg_ref.agg_map(dims), int(np.prod(mg_ref.coarse_dims(dims))))


def members_of(agg, nc):
    """the ascending preimages of a map as member lists: (nc, 8) ints, -1 behind the last"""
    agg = np.asarray(agg, np.int64)
    order = np.argsort(agg, kind="stable")
    counts = np.bincount(agg, minlength=nc)
    assert counts.max(initial=0) <= WIDTH
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    mem = np.full((nc, WIDTH), -1, np.int32)
    mem[agg[order], np.arange(agg.size) - first[agg[order]]] = order
    return mem


def restrict(dtype, members, b, w, dinv_c, c1, rules=EXACT):
    """mg_restrict_kernel / amg_restrict_kernel through member lists (nc, 8): s = +0, then s = s + (b[i] - w[i]) over the members in
    list order; returns (bc, t) with t = c1 * vmul(dinv_c, bc), what xc takes and, with store_d, dc.  b, w: (nrhs, >= fine rows)"""
    members = np.asarray(members)
    nc, nrhs = members.shape[0], np.asarray(b).shape[0]
    Rt = R.real_type(dtype)
    cplx = R.is_complex(dtype)
    bp, wp = parts(b, dtype), parts(w, dtype)
    s = (np.zeros((nrhs, nc), Rt), np.zeros((nrhs, nc), Rt) if cplx else None)
    slots = range(WIDTH) if rules.members == "ascending" else range(WIDTH - 1, -1, -1)
    with np.errstate(all="ignore"):
        for k in slots:
            live = np.flatnonzero(members[:, k] >= 0)
            i = members[live, k]
            s[0][:, live] = s[0][:, live] + (bp[0][:, i] - wp[0][:, i])
            if cplx:
                s[1][:, live] = s[1][:, live] + (bp[1][:, i] - wp[1][:, i])
        di = parts(dinv_c, dtype)
        t = R.vmul_t((di[0][None, :], None if di[1] is None else di[1][None, :]), s, dtype)
        t = _scale(coefficient(c1, dtype), t)
    return join(s, dtype), join(t, dtype)


def prolong(dtype, agg, e, x, omega):
    """mg_prolong_kernel / amg_prolong_kernel: x[i] + omega * e[agg[i]] for the len(agg) fine rows; e: (nrhs, >= coarse rows), x: (nrhs,
    len(agg)).  Returns the new rows"""
    agg = np.asarray(agg, np.int64)
    ep, xp = parts(e, dtype), parts(x, dtype)
    with np.errstate(all="ignore"):
        g = (ep[0][:, agg], None if ep[1] is None else ep[1][:, agg])
        out = _add((xp[0][:, :agg.size], None if xp[1] is None else xp[1][:, :agg.size]), _scale(coefficient(omega, dtype), g))
    return join(out, dtype)


# ---- the scan -----------------------------------------------------------------------------------------------------------------------------
def scan(counts):
    """mg_scan_kernel as it runs: thread t of 1024 sums the chunk [t c, (t + 1) c) cut at n, c = ceil(n / 1024), in 64 bits; thread 0
    scans the chunk sums and clamps the total; every thread writes its chunk's prefixes, clamped.  Returns (the n + 1 ints, overflow)"""
    a = np.asarray(counts, np.int64)
    n = a.size
    chunk = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    lo = np.minimum(n, np.arange(SCAN_BLOCK, dtype=np.int64) * chunk)
    hi = np.minimum(n, lo + chunk)
    sums = np.array([int(a[l:h].sum()) for l, h in zip(lo, hi)], np.int64)
    base = np.concatenate([[0], np.cumsum(sums)[:-1]])
    total = int(sums.sum())
    out = np.empty(n + 1, np.int64)
    for t in range(SCAN_BLOCK):
        run = int(base[t])
        for i in range(int(lo[t]), int(hi[t])):
            out[i] = min(run, INT_MAX)
            run += int(a[i])
    out[n] = min(total, INT_MAX)
    return out.astype(np.int32), int(total > INT_MAX)


# ---- the launch chain of one cycle --------------------------------------------------------------------------------------------------------
def level(ip, ix, da, dinv, c0, c1, n=None, nu=None, ld=None, members=None, agg=None, spmv=("lane",)):
    """one level as data.  ip, ix, da: the CSR arrays of its nu rows; n >= nu: the rows its kernels work on (the rows from nu on are
    empty); dinv: n values; c0, c1: the doubles of its steps (len = steps); members / agg: the lists and the map to the next level
    (None on the coarsest); spmv: ("lane",) for every one-lane-per-row form, ("chunked", lanes per row) for the chunked kernel"""
    nu = len(ip) - 1 if nu is None else nu
    n = nu if n is None else n
    ip = np.concatenate([np.asarray(ip, np.int64), np.full(n - nu, ip[-1], np.int64)])
    return {"ip": ip, "ix": np.asarray(ix), "da": np.asarray(da), "dinv": np.asarray(dinv), "c0": list(c0), "c1": list(c1), "n": n,
            "nu": nu, "ld": n if ld is None else ld, "steps": len(c1), "members": members, "agg": agg, "spmv": spmv}


def product(L, x, dtype):
    """w = A x on the n rows of a level, as its SpMV form adds a row up; x, w: (nrhs, n)"""
    if L["spmv"][0] == "chunked":
        return np.concatenate([R.spmv_chunked_in_type(L["ip"], L["ix"], L["da"], x[r], dtype, L["spmv"][1]) for r in range(x.shape[0])])
    return R.spmv_in_type(L["ip"], L["ix"], L["da"], x, dtype, x.shape[0])


def cycle_bits(levels, r, omega, dtype, rules=EXACT):
    """z of one V-cycle launch for launch (include/cgamd.h, the chain of one cycle): r, z: (nrhs, n of level 0), the padding rows of r
    zero.  Every vector of a coarse level starts as zeros, as the hierarchy allocates them"""
    dtype = np.dtype(dtype)
    r = np.asarray(r, dtype)
    nrhs, nl = r.shape[0], len(levels)
    x = [np.zeros((nrhs, L["n"]), dtype) for L in levels]
    b = [np.zeros((nrhs, L["n"]), dtype) for L in levels]
    d = [np.zeros((nrhs, L["n"]), dtype) for L in levels]
    b[0] = r
    assert r.shape[1] == levels[0]["n"]

    def step(l, mode, k):
        L = levels[l]
        w = product(L, x[l], dtype) if mode else None
        keep = mode == 2 or L["steps"] > 1
        xn, dn = smooth_step(dtype, mode, L["dinv"], b[l], w, d[l], x[l], L["c0"][k] if mode == 2 else 0.0, L["c1"][k], keep, rules)
        x[l] = xn
        if dn is not None:
            d[l] = dn

    def later(l):
        for k in range(1, levels[l]["steps"]):
            step(l, 2, k)

    for l in range(nl):
        L = levels[l]
        if l == 0:
            step(0, 0, 0)
        later(l)
        if l == nl - 1:
            break
        C = levels[l + 1]
        w = product(L, x[l], dtype)
        bc, t = restrict(dtype, L["members"], b[l], w, C["dinv"], C["c1"][0], rules)
        b[l + 1][:, :C["nu"]] = bc
        x[l + 1][:, :C["nu"]] = t
        if C["steps"] > 1:
            d[l + 1][:, :C["nu"]] = t
    for l in range(nl - 2, -1, -1):
        L = levels[l]
        x[l][:, :L["nu"]] = prolong(dtype, L["agg"], x[l + 1], x[l][:, :L["nu"]], omega)
        step(l, 1, 0)
        later(l)
    return x[0]


def levels_of(H, dtype):
    """the levels of an mg_ref.Hierarchy (grid or algebraic) as cycle_bits takes them"""
    out = []
    for l, L in enumerate(H.levels):
        last = l == len(H.levels) - 1
        A = L.A
        nc = None if last else H.levels[l + 1].n
        out.append(level(A.indptr, A.indices, A.data.astype(dtype), L.dinv.astype(dtype), L.c0, L.c1,
                         members=None if last else members_of(L.agg, nc), agg=None if last else np.asarray(L.agg)))
    return out


# ---- per-level setup data -----------------------------------------------------------------------------------------------------------------
def diag_sums(ip, ix, da, dtype):
    """the diagonal of every row: its entries with column == row added in stored order in double / complex double, from +0"""
    W = mg_ref.wide(dtype)
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(ip, np.int64)))
    on = np.asarray(ix, np.int64) == rows
    acc = np.zeros(n, W)
    np.add.at(acc, rows[on], np.asarray(da)[on].astype(W))
    return acc


def smith_reciprocal(b):
    """(1 + 0i) / b by Smith's algorithm as csrc/device_types.h acc_div writes it, every operation one IEEE double operation"""
    br, bi = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(all="ignore"):
        r1 = bi / br
        d1 = br + bi * r1
        re1, im1 = (one + zero * r1) / d1, (zero - one * r1) / d1
        r2 = br / bi
        d2 = br * r2 + bi
        re2, im2 = (one * r2 + zero) / d2, (zero * r2 - one) / d2
    first = np.abs(br) >= np.abs(bi)
    out = np.empty(b.shape, np.complex128)
    out.real, out.imag = np.where(first, re1, re2), np.where(first, im1, im2)
    return out


def dinv_bits(ip, ix, da, dtype):
    """T(1 / the diagonal sum in double): one correctly rounded division for the real types, Smith's for the complex ones"""
    acc = diag_sums(ip, ix, da, dtype)
    with np.errstate(all="ignore"):
        return (smith_reciprocal(acc) if R.is_complex(dtype) else np.float64(1.0) / acc).astype(dtype)


def lmax_real(ip, da, dinv):
    """max_i |dinv_i| * (sum_j |a_ij| in stored order, in double, from +0) for a real value type: the bits of the device's lmax"""
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(ip, np.int64)))
    s = np.zeros(n, np.float64)
    np.add.at(s, rows, np.abs(np.asarray(da).astype(np.float64)))
    return float(np.max(np.abs(np.asarray(dinv)[:n].astype(np.float64)) * s))


# ---- the inputs of the device tests (and of the CPU test, which shows what they can tell apart) -------------------------------------------
def spread(rng, shape, dtype, half):
    """magnitudes over 2^-half .. 2^half, random signs and mantissas"""
    Rt = R.real_type(dtype)

    def one():
        return (rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-half, half + 1, shape)) * rng.choice([-1.0, 1.0], shape)).astype(Rt)
    return R._join(one(), one(), dtype) if R.is_complex(dtype) else one().astype(dtype)


def specials(dtype):
    """lanes (dinv, b, w, d, x) that hold -0, +-inf, NaN, subnormals and ties of the products and sums of a step.  p = the significand
    bits of the real type: (1 + 2^-j)(1 + 2^-k), j + k = p, ends in a half step (tie to even), as do 1 + 2^-p and 1 + 3 * 2^-p"""
    Rt = R.real_type(dtype)
    p = 24 if Rt is np.float32 else 53
    j = p // 2
    tiny = float(np.finfo(Rt).tiny)
    sub = float(np.finfo(Rt).smallest_subnormal)
    lanes = [
        (1.0 + 2.0 ** -j, 1.0 + 2.0 ** -(p - j), 0.0, 0.0, 0.0),              # dinv * b: a tie, down to even
        (1.0 + 2.0 ** -j, 3.0 + 3 * 2.0 ** -(p - j), 1.0, 2.0 ** -p, 1.0),     # b - w exact, the product rounds up; d and x half a step
        (1.0, 2.0 ** -p, 0.0, 1.0, 1.0 + 2.0 ** -(p - 1)),                      # x + t: a tie, up to even
        (-0.0, 1.0, 0.0, -0.0, -0.0),                                          # -0 from the product, kept by the sums of zeros
        (1.0, -0.0, 0.0, -0.0, -0.0),
        (1.0, np.inf, 1.0, 1.0, 1.0),
        (1.0, np.inf, np.inf, 1.0, 1.0),                                       # inf - inf
        (0.0, -np.inf, 1.0, 1.0, 1.0),                                         # 0 * inf
        (2.0, np.nan, 1.0, 1.0, 1.0),
        (1.0, 1.0, 1.0, np.inf, -np.inf),
        (0.75, 3 * sub, sub, 5 * sub, 7 * sub),                                # subnormals, the product rounded at the least one
        (0.5, tiny, sub, tiny / 2, -tiny),                                     # across the edge of the normal range
        (float(np.finfo(Rt).max), 2.0, 0.0, 1.0, 1.0),                         # overflow of the product
    ]
    arr = np.array(lanes, dtype=np.float64).astype(Rt)
    if R.is_complex(dtype):
        im = np.roll(arr, 3, axis=0)                                           # the imaginary parts: the same lanes, rotated,
        im[10:12] = 0                                                          # but +0 beside the subnormals, which stay subnormal
        return R._join(arr, im, dtype)
    return arr.astype(dtype)


SMOOTH_SIZES = (1, 255, 256, 257, 1287)


def smooth_cases():
    """mode x store_d x type x size; nrhs, the spare lanes of the leading dimension and the pointer offset vary with the size"""
    out = []
    for dt in DTYPES:
        for mode in (0, 1, 2):
            for store_d in (0, 1):
                for size in SMOOTH_SIZES:
                    nrhs = 3 if size in (1, 257) else 1
                    off = 8 if size in (255, 1287) else 0
                    c = {"dt": dt, "mode": mode, "store_d": store_d, "size": size, "nrhs": nrhs, "ld": size + (5 if size != 256 else 1),
                         "off": off}
                    c["id"] = f"{dt}-mode{mode}-d{store_d}-n{size}x{nrhs}-off{off}"
                    c["seed"] = zlib.crc32(c["id"].encode())
                    out.append(c)
    return out


def smooth_inputs(c):
    """dinv (size,), b, w, d, x (nrhs, size), c0, c1 (doubles that are not representable in float)"""
    dtype, rng = DTYPES[c["dt"]], np.random.default_rng(c["seed"])
    n, nrhs = c["size"], c["nrhs"]
    inp = {"dinv": spread(rng, n, dtype, 3)}
    for name in ("b", "w", "d", "x"):
        inp[name] = spread(rng, (nrhs, n), dtype, 4)
    sp = specials(dtype)
    K = len(sp)
    shift = c["seed"] % K
    lanes = [(j, (j + shift) % K) for j in range(min(n, K))]
    if n >= K + 3:
        lanes += [(n - 3 + j, (shift + 5 + j) % K) for j in range(3)]          # (the last lanes of the last work-group as well)
    for at, k in lanes:
        inp["dinv"][at] = sp[k][0]
        for pos, name in enumerate(("b", "w", "d", "x")):
            inp[name][:, at] = sp[k][pos + 1]
    inp["c0"], inp["c1"] = 0.3 + rng.uniform(0, 0.1), 1.0 / (3.0 + rng.uniform(0, 1))
    return inp


BOX_DIMS = ((1, 1, 1), (2, 1, 1), (13, 1, 1), (9, 7, 1), (7, 6, 5), (13, 11, 9), (16, 16, 16))
STORED_AGGREGATES = (1, 255, 257, 700)


def partition(rng, nagg):
    """a random partition into nagg aggregates of 1 .. 8 rows, every size present where nagg allows (one aggregate: 8 rows), members
    scattered over the fine rows; coarse ids in no particular order.  Returns (agg, members)"""
    sizes = rng.integers(1, WIDTH + 1, nagg)
    sizes[:min(nagg, WIDTH)] = (np.arange(WIDTH, 0, -1))[:min(nagg, WIDTH)]
    sizes = rng.permutation(sizes) if nagg > 1 else sizes
    agg = rng.permutation(np.repeat(np.arange(nagg), sizes)).astype(np.int32)
    return agg, members_of(agg, nagg)


def transfer_cases():
    out = []
    for dt in DTYPES:
        for dims in BOX_DIMS:
            out.append({"dt": dt, "kind": "box", "dims": dims, "id": f"{dt}-box-" + "x".join(map(str, dims))})
        for nagg in STORED_AGGREGATES:
            out.append({"dt": dt, "kind": "stored", "nagg": nagg, "id": f"{dt}-stored-{nagg}"})
    for c in out:
        c["seed"] = zlib.crc32(c["id"].encode())
    return out


def order_shows(dtype, members, b, w, dinv_c, c1):
    """per right-hand side: does summing the members in descending order change a bit of bc?"""
    up = restrict(dtype, members, b, w, dinv_c, c1)[0]
    down = restrict(dtype, members, b, w, dinv_c, c1, Rules(members="descending"))[0]
    return [not R.bit_equal(up[r], down[r]) for r in range(up.shape[0])]


def transfer_inputs(c, nrhs=3):
    """agg, members, nf, nc, and b, w, x (nrhs, nf), e (nrhs, nc), dinv_c (nc,), c1, omega.  b - w cancels to a few binades below the
    operands in most rows and the differences lie a few binades apart, so the order of an aggregate's sum shows; where a case has an
    aggregate of three rows or more the seed is advanced until it shows in every column (tests/test_mg_kernel_ref.py asserts it)"""
    dtype = DTYPES[c["dt"]]
    seed = c["seed"]
    while True:
        rng = np.random.default_rng(seed)
        if c["kind"] == "box":
            agg = mg_ref.agg_map(c["dims"]).astype(np.int32)
            nc = int(np.prod(mg_ref.coarse_dims(c["dims"])))
            members = members_of(agg, nc)
        else:
            agg, members = partition(rng, c["nagg"])
            nc = c["nagg"]
        nf = agg.size
        w = spread(rng, (nrhs, nf), dtype, 3)
        near = join(_add(parts(w, dtype), parts(spread(rng, (nrhs, nf), dtype, 3), dtype)), dtype)      # b = fl(w + delta): b - w cancels
        b = np.where(rng.random((nrhs, nf)) < 0.5, near, spread(rng, (nrhs, nf), dtype, 3))
        inp = {"agg": agg, "members": members, "nf": nf, "nc": nc, "b": b.astype(dtype), "w": w, "x": spread(rng, (nrhs, nf), dtype, 3),
               "e": spread(rng, (nrhs, nc), dtype, 3), "dinv_c": spread(rng, nc, dtype, 3), "c1": 1.0 / (3.0 + rng.uniform(0, 1)),
               "omega": 1.6, "seed": seed}
        if (members[:, 2] < 0).all() or all(order_shows(dtype, members, inp["b"], w, inp["dinv_c"], inp["c1"])):
            return inp
        seed += 1


SCAN_SIZES = (1, 2, 1023, 1024, 1025, 2047, 2049, 5000)


def scan_cases():
    """(id, counts): random counts 0 .. 64 at every size, all zeros, and three counts of 2^30 (a total above 2^31 - 1)"""
    out = []
    for n in SCAN_SIZES:
        out.append((f"random-{n}", np.random.default_rng(n).integers(0, 65, n).astype(np.int32)))
    out.append(("zeros-2049", np.zeros(2049, np.int32)))
    out.append(("overflow-3", np.full(3, 2 ** 30, np.int32)))
    big = np.random.default_rng(7).integers(0, 65, 2049).astype(np.int32)
    big[[5, 1030, 2040]] = 2 ** 30
    out.append(("overflow-2049", big))
    return out
