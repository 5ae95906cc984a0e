"""Host restatement of the four streaming kernels of the mixed-precision solve (csrc/mixed.hip; include/cgamd.h "Mixed precision: the
kernels") -- plain numpy, no GPU -- and the cases tests/test_gpu_mixed_kernels.py runs them on.

Why it can be exact
-------------------
The library is built with -ffp-contract=off, so every product and sum of a kernel is one IEEE double operation and every (float) one
rounding to nearest-even; numpy's float64 array operations and its float64 -> float32 cast are the same single operations.  All four
kernels are real and component-wise: a column of `size` values is m = size * R real lanes, R = 1 (float64) or 2 (complex128), and
everything here works on the lanes (the float64 / float32 view of the arrays).

Rules restated (mixed.hip)
--------------------------
accumulate    x_hi[i] = x_hi[i] + s_r * (double)x_lo[i], columns with mask[r] != 0; the others stay as they are
round_down    r_lo[i] = (float)(r_hi[i] * s_r) for i < m; lanes m <= i < ld_lo R of every column are written as +0
round_values  lo[j] = (float)hi[j]
norm2         G = min(1024, ceil(m / 4096)) work-groups of 256 threads per column, T = 256 g + t, S = 256 G, every thread from +0:
              16-byte form: the quads q = T, T + S, ... < m / 4, the four squares of a quad in lane order, then the tail lane
              4 (m / 4) + T for T < m % 4; scalar form: the lanes T, T + S, ... < m; then cg_step_ref.block_sum (wave tree, wave
              sums in order) gives partials[r, g]; one thread adds the G partials from +0 in index order.
the form      mixed_vec: 16-byte form when every array pointer is 16-byte aligned and, with nRHS > 1, every leading dimension is a
              whole number of 16 bytes; round_values: both pointers aligned.

Padding with zeros: a strided pass is padded to whole rounds with +0.  A square is never -0 and an accumulator that starts from +0
never becomes -0, so acc + (+0) is acc in every bit.

The bound of the norm against an exact sum (math.fsum of the rounded squares): (k + 1) eps sum, eps = 2^-52, k the additions on the
longest path -- ceil(m / (256 G)) per thread, 6 wave steps, 3 wave sums, G partials.  It covers the kernel: a thread of the 16-byte
form makes at most 4 ceil(m / (4 S)) + 1 <= m / S + 5 additions, each within the unit roundoff eps / 2 of a partial sum of non-negative
terms, so the whole error is at most (m / S + 5 + 9 + G) (eps / 2) sum (1 + O(eps)) < (k + 1) eps sum."""
import math
import zlib

import numpy as np

import cg_step_ref as S

EPS = float(np.finfo(np.float64).eps)
BLOCK, LANES_PER_GROUP, MAX_GRID = 256, 256 * 16, 1024
DT = {"f64": np.float64, "c128": np.complex128}
CODE = {"f64": 1, "c128": 3}                    # CGAMD_F64, CGAMD_C128


def lanes_per_value(dt):
    return 2 if np.dtype(DT.get(dt, dt)).kind == "c" else 1


def grid(m):
    """mixed_grid: work-groups per column for m real lanes"""
    return max(1, min(-(-m // LANES_PER_GROUP), MAX_GRID))


def takes_vec(hi_addr, ld_hi_bytes, lo_addr, ld_lo_bytes, nrhs):
    """mixed.hip mixed_vec; lo_addr None: a kernel with one array (norm2, whose ld_lo_bytes is 0)"""
    if hi_addr % 16 or (lo_addr is not None and lo_addr % 16):
        return False
    return nrhs <= 1 or ((ld_hi_bytes | ld_lo_bytes) & 15) == 0


def round_values_takes_vec(hi_addr, lo_addr):
    return hi_addr % 16 == 0 and lo_addr % 16 == 0


# ---- the element-wise kernels, on lanes: hi (nrhs, m) float64, lo (nrhs, m) float32 ------------------------------------------------------
def accumulate(x_hi, x_lo, scale, mask):
    out = x_hi.copy()
    with np.errstate(all="ignore"):
        for r in range(x_hi.shape[0]):
            if mask[r]:
                out[r] = x_hi[r] + np.float64(scale[r]) * x_lo[r].astype(np.float64)
    return out


def round_down(r_hi, inv_scale, ld_lo_lanes):
    """(nrhs, ld_lo_lanes) float32: the rounded lanes, then the padding zeros"""
    nrhs, m = r_hi.shape
    out = np.zeros((nrhs, ld_lo_lanes), np.float32)
    with np.errstate(all="ignore"):
        for r in range(nrhs):
            out[r, :m] = (r_hi[r] * np.float64(inv_scale[r])).astype(np.float32)
    return out


def round_values(hi):
    with np.errstate(all="ignore"):
        return hi.astype(np.float32)


# ---- the norm ----------------------------------------------------------------------------------------------------------------------------
def _thread_sums_vec(t, G):
    """16-byte form: t (nrhs, m) squares -> (nrhs, 256 G) per-thread sums"""
    nrhs, m = t.shape
    St, nq = G * BLOCK, m // 4
    J = -(-nq // St)
    body = np.zeros((nrhs, J * St * 4), np.float64)
    body[:, :nq * 4] = t[:, :nq * 4]
    body = body.reshape(nrhs, J, St, 4)
    acc = np.zeros((nrhs, St), np.float64)
    with np.errstate(all="ignore"):
        for j in range(J):
            for k in range(4):
                acc = acc + body[:, j, :, k]
        tail = np.zeros((nrhs, St), np.float64)
        tail[:, :m - nq * 4] = t[:, nq * 4:]
        acc = acc + tail
    return acc


def _thread_sums_scalar(t, G):
    """scalar form: lane T, T + S, ... per thread"""
    nrhs, m = t.shape
    St = G * BLOCK
    J = -(-m // St)
    body = np.zeros((nrhs, J * St), np.float64)
    body[:, :m] = t
    body = body.reshape(nrhs, J, St)
    acc = np.zeros((nrhs, St), np.float64)
    with np.errstate(all="ignore"):
        for j in range(J):
            acc = acc + body[:, j]
    return acc


def norm2(v, vec):
    """v (nrhs, m) float64 lanes -> (partials (nrhs, G), out (nrhs,)) in the device's order"""
    nrhs, m = v.shape
    G = grid(m)
    with np.errstate(all="ignore"):
        t = v * v
        acc = _thread_sums_vec(t, G) if vec else _thread_sums_scalar(t, G)
        partials = S.block_sum(acc.reshape(nrhs * G, BLOCK)).reshape(nrhs, G)
        out = np.zeros(nrhs, np.float64)
        for g in range(G):
            out = out + partials[:, g]
    return partials, out


def norm2_exact(v):
    """math.fsum of the rounded squares per column: exact sums of what the kernel adds up"""
    return np.array([math.fsum((row * row).tolist()) for row in v])


def norm2_bound(m, total):
    G = grid(m)
    k = -(-m // (G * BLOCK)) + 6 + 3 + G
    return (k + 1) * EPS * total


# ---- planted values of the two rounding kernels: (the double that is rounded, what it tests) ----------------------------------------------
PLANTS = [
    (1.0 + 2.0 ** -24, "tie, down to the even 1"),
    (1.0 + 3 * 2.0 ** -24, "tie, up to the even 1 + 2^-22"),
    (-(1.0 + 2.0 ** -24), "tie, negative"),
    (1e39, "overflow: inf"),
    (-(2.0 - 2.0 ** -24) * 2.0 ** 127, "the tie above FLT_MAX: -inf"),
    ((2.0 - 2.0 ** -24 - 2.0 ** -40) * 2.0 ** 127, "just below that tie: FLT_MAX"),
    (-0.0, "-0 stays -0"),
    (float("nan"), "NaN"),
    (1.2345678 * 2.0 ** -135, "float subnormal, rounded at 2^-149"),
    (3 * 2.0 ** -150, "tie of two subnormals: the even 2^-148"),
    (-(2.0 ** -150), "tie of 0 and the least subnormal: -0"),
    (2.0 ** -150 + 2.0 ** -190, "just above it: 2^-149"),
    (2.0 ** -126 - 2.0 ** -151, "rounds up into the normal range"),
]


def plant(h, scale, shift):
    """write PLANTS[...] / scale (exact: scale is a power of two) over the first lanes of every column and, rotated, over the last
    three, so that the body and the tail of the 16-byte form both convert them"""
    nrhs, m = h.shape
    K = len(PLANTS)
    for r in range(nrhs):
        for j in range(min(m, K)):
            h[r, j] = PLANTS[(j + shift + r) % K][0] / scale[r]
        for j in range(max(m - 3, min(m, K)), m):
            h[r, j] = PLANTS[(j + shift + r + 5) % K][0] / scale[r]
    return h


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
BIG = 1024 * 4096 + 4 * 256 * 3 + 3             # the grid cap (G = 1024 < ceil(m / 4096)) and a fifth, partial stride pass
MASKS3 = ([1, 0, 1], [0, 0, 0], [0, 1, 0])
# cases whose seed was advanced until the order of the norm's sum shows in the bits (tests/test_mixed_kernel_ref.py: the two forms
# differ, and the case's own form differs from numpy's sum): two orders of one sum agree in every bit in about half the draws
SALT = {'edges-f64-1023x1-ld1023.1023-off0.0': '+3', 'edges-f64-1025x1-ld1025.1025-off0.0': '+5', 'edges-f64-4096x1-ld4096.4096-off0.0': '+4',
        'edges-f64-4097x1-ld4097.4097-off0.0': '+4', 'edges-c128-2049x1-ld2049.2049-off0.0': '+2', 'rhs3-f64-957x3-ld958.960-off0.0': '+1',
        'rhs3-c128-957x3-ld957.957-off0.0': '+1', 'offset-f64-1029x1-ld1029.1029-off8.4': '+1', 'offset-c128-515x1-ld515.515-off8.4': '+2'}


def _case(group, dt, size, nrhs=1, ld_hi=None, ld_lo=None, off_hi=0, off_lo=0, vec=True, vec_norm=None):
    c = {"group": group, "dt": dt, "size": size, "nrhs": nrhs, "ld_hi": ld_hi or size, "ld_lo": ld_lo or size, "off_hi": off_hi,
         "off_lo": off_lo, "vec": vec, "vec_norm": vec if vec_norm is None else vec_norm}
    c["id"] = f"{group}-{dt}-{size}x{nrhs}-ld{c['ld_hi']}.{c['ld_lo']}-off{off_hi}.{off_lo}"
    c["seed"] = zlib.crc32((c["id"] + SALT.get(c["id"], "")).encode())
    c["R"] = lanes_per_value(dt)
    c["m"] = size * c["R"]
    c["masks"] = MASKS3 if nrhs == 3 else ([1] * nrhs,)
    return c


def cases():
    out = []
    for size in (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4096, 4097):
        out.append(_case("edges", "f64", size))
    for size in (1, 2, 3, 513, 2049):
        out.append(_case("edges", "c128", size))
    out.append(_case("cap", "f64", BIG))
    # three right-hand sides of 957 values: the leading dimensions of a handle (whole packs), then 957 on both sides.  complex128:
    # a value is 16 bytes, so 957 is whole packs on the hi side and the norm keeps its 16-byte form
    out.append(_case("rhs3", "f64", 957, 3, 958, 960))
    out.append(_case("rhs3", "f64", 957, 3, 957, 957, vec=False))
    out.append(_case("rhs3", "c128", 957, 3, 957, 958))
    out.append(_case("rhs3", "c128", 957, 3, 957, 957, vec=False, vec_norm=True))
    # pointers 8 bytes (hi) and 4 bytes (lo) off a 16-byte boundary
    out.append(_case("offset", "f64", 1029, 1, off_hi=8, off_lo=4, vec=False))
    out.append(_case("offset", "c128", 515, 1, off_hi=8, off_lo=4, vec=False))
    return out


def inputs(c):
    """the lanes of a case: x_hi, r_hi with the planted values, values (float64, magnitudes over 2^-30 .. 2^30), x_lo (float32), v
    (float64, narrow), scale, inv_scale (powers of two, 2^-60 .. 2^60)"""
    rng = np.random.default_rng(c["seed"])
    nrhs, m = c["nrhs"], c["m"]
    x_hi = np.stack([S.spread(rng, m, np.float64, half=30) for _ in range(nrhs)])
    x_lo = np.stack([S.spread(rng, m, np.float32, half=30) for _ in range(nrhs)])
    r_hi = np.stack([S.spread(rng, m, np.float64, half=30) for _ in range(nrhs)])
    scale = np.exp2(np.array([[-60, 60, 7][(r + c["seed"]) % 3] for r in range(nrhs)], dtype=np.float64))
    inv_scale = np.exp2(np.array([[60, -60, -9][(r + c["seed"]) % 3] for r in range(nrhs)], dtype=np.float64))
    r_hi = plant(r_hi, inv_scale, c["seed"] % len(PLANTS))
    vals = plant(np.stack([S.spread(rng, m, np.float64, half=30)]), np.ones(1), (c["seed"] // 7) % len(PLANTS))[0]
    # a second vector for the norm with magnitudes over 2^-4 .. 2^4 only: under the wide spread a few squares carry the sum and most
    # orders of adding the rest round to the same bits; here nearly every change of order shows
    v = np.stack([S.spread(rng, m, np.float64, half=4) for _ in range(nrhs)])
    return {"x_hi": x_hi, "x_lo": x_lo, "r_hi": r_hi, "scale": scale, "inv_scale": inv_scale, "values": vals, "v": v}
