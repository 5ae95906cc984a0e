// Mixed-precision CG (include/cgamd.h "Mixed precision"): the streaming kernels between the fp64 / complex128 side (x and the true
// residual, the OUTER handle) and the fp32 / complex64 side (the recurrence, the INNER handle).  Templated on the pair (HI, LO) =
// (double, float) or (double2, float2).  Every operation here is real and component-wise -- the scale is a real power of two and the
// norm is the conjugated one, re^2 + im^2 -- so a kernel walks the R = 1 or 2 real lanes of its values: 4 lanes per step, one 16-byte
// access on the lo side and two on the hi side, and a scalar tail.  The two sides have leading dimensions of their own (957 rows:
// 958 in fp64, 960 in fp32), both whole 16-byte packs; where a pointer or a leading dimension is not, the scalar form runs.
// grid = (G, nRHS).  Sums: per-thread in index order, block_sum, then ONE thread adds the G partials in order -- no atomics, the
// same bits on every run.  Bytes per right-hand side of n values: accumulate 20 n R (reads 4 + 8, writes 8), round_down 12 n R,
// norm2 8 n R.
#include <algorithm>

#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"

namespace cgamd {

template <typename HI, typename LO> struct MixedPair;
template <> struct MixedPair<double, float> { static constexpr int R = 1; };
template <> struct MixedPair<double2, float2> { static constexpr int R = 2; };

constexpr int kMixedLanesPerThread = 16;     // four 4-lane steps per thread at streaming sizes
constexpr int kMixedMaxGrid = 1024;

static int mixed_grid(long long lanes) {
    long long g = (lanes + (long long)kBlock * kMixedLanesPerThread - 1) / ((long long)kBlock * kMixedLanesPerThread);
    return (int)std::max(1LL, std::min<long long>(g, kMixedMaxGrid));
}

// x_hi += scale * HI(x_lo): the product is exact (a power of two times a float, in double), the add rounds once.  A right-hand side
// whose mask is clear leaves at once: its x_hi is neither read nor written
template <typename HI, typename LO, bool VEC>
__global__ __launch_bounds__(kBlock) void mixed_accumulate_kernel(long long n, HI *__restrict__ x_hi, long long ld_hi, const LO *__restrict__ x_lo,
                                                                  long long ld_lo, const double *__restrict__ scale, const int *__restrict__ mask) {
    const int r = blockIdx.y;
    if (mask[r] == 0) return;
    constexpr int R = MixedPair<HI, LO>::R;
    double *xh = reinterpret_cast<double *>(x_hi + (long long)r * ld_hi);
    const float *xl = reinterpret_cast<const float *>(x_lo + (long long)r * ld_lo);
    const long long m = n * R, stride = (long long)gridDim.x * kBlock;
    const double s = scale[r];
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long nq = m / 4;
        for (long long i = i0; i < nq; i += stride) {
            const float4 l = *reinterpret_cast<const float4 *>(xl + 4 * i);
            double2 h0 = *reinterpret_cast<const double2 *>(xh + 4 * i), h1 = *reinterpret_cast<const double2 *>(xh + 4 * i + 2);
            h0.x = h0.x + s * (double)l.x; h0.y = h0.y + s * (double)l.y;
            h1.x = h1.x + s * (double)l.z; h1.y = h1.y + s * (double)l.w;
            *reinterpret_cast<double2 *>(xh + 4 * i) = h0;
            *reinterpret_cast<double2 *>(xh + 4 * i + 2) = h1;
        }
        i0 += nq * 4;
    }
    for (long long i = i0; i < m; i += stride) xh[i] = xh[i] + s * (double)xl[i];
}

// r_lo = LO(r_hi * inv_scale): exact scaling, one rounding; the lo side's padding rows (n <= i < ld_lo) are written as zeros
template <typename HI, typename LO, bool VEC>
__global__ __launch_bounds__(kBlock) void mixed_round_down_kernel(long long n, const HI *__restrict__ r_hi, long long ld_hi, LO *__restrict__ r_lo,
                                                                  long long ld_lo, const double *__restrict__ inv_scale) {
    const int r = blockIdx.y;
    constexpr int R = MixedPair<HI, LO>::R;
    const double *rh = reinterpret_cast<const double *>(r_hi + (long long)r * ld_hi);
    float *rl = reinterpret_cast<float *>(r_lo + (long long)r * ld_lo);
    const long long m = n * R, stride = (long long)gridDim.x * kBlock;
    const double s = inv_scale[r];
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long nq = m / 4;
        for (long long i = i0; i < nq; i += stride) {
            const double2 h0 = *reinterpret_cast<const double2 *>(rh + 4 * i), h1 = *reinterpret_cast<const double2 *>(rh + 4 * i + 2);
            float4 l;
            l.x = (float)(h0.x * s); l.y = (float)(h0.y * s); l.z = (float)(h1.x * s); l.w = (float)(h1.y * s);
            *reinterpret_cast<float4 *>(rl + 4 * i) = l;
        }
        i0 += nq * 4;
    }
    for (long long i = i0; i < m; i += stride) rl[i] = (float)(rh[i] * s);
    if (blockIdx.x == 0)
        for (long long i = m + threadIdx.x; i < ld_lo * R; i += kBlock) rl[i] = 0.f;
}

// partials[r * G + b] = the work-group's part of sum |v_i|^2
template <typename HI, bool VEC>
__global__ __launch_bounds__(kBlock) void mixed_norm2_kernel(long long m, int R, const HI *__restrict__ v, long long ld, double *__restrict__ partials) {
    __shared__ double red[kBlock / kWave];
    const int r = blockIdx.y;
    const double *p = reinterpret_cast<const double *>(v + (long long)r * ld);
    const long long stride = (long long)gridDim.x * kBlock;
    double acc = 0.;
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long nq = m / 4;
        for (long long i = i0; i < nq; i += stride) {
            const double2 h0 = *reinterpret_cast<const double2 *>(p + 4 * i), h1 = *reinterpret_cast<const double2 *>(p + 4 * i + 2);
            acc = acc + h0.x * h0.x; acc = acc + h0.y * h0.y; acc = acc + h1.x * h1.x; acc = acc + h1.y * h1.y;
        }
        i0 += nq * 4;
    }
    for (long long i = i0; i < m; i += stride) acc = acc + p[i] * p[i];
    const double t = block_sum<kBlock>(acc, red);
    if (threadIdx.x == 0) partials[(long long)r * gridDim.x + blockIdx.x] = t;
}
// the one-thread finish: the G partials of right-hand side blockIdx.x in order
__global__ void mixed_norm2_finish_kernel(const double *__restrict__ partials, int G, double *__restrict__ out) {
    if (threadIdx.x != 0) return;
    const double *p = partials + (long long)blockIdx.x * G;
    double acc = 0.;
    for (int i = 0; i < G; ++i) acc = acc + p[i];
    out[blockIdx.x] = acc;
}

// lo[j] = LO(hi[j]) over `m` real lanes: the inner handle's copy of the matrix values, rounded once
template <bool VEC>
__global__ __launch_bounds__(kBlock) void mixed_round_values_kernel(long long m, const double *__restrict__ hi, float *__restrict__ lo) {
    const long long stride = (long long)gridDim.x * kBlock;
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long nq = m / 4;
        for (long long i = i0; i < nq; i += stride) {
            const double2 h0 = *reinterpret_cast<const double2 *>(hi + 4 * i), h1 = *reinterpret_cast<const double2 *>(hi + 4 * i + 2);
            float4 l;
            l.x = (float)h0.x; l.y = (float)h0.y; l.z = (float)h1.x; l.w = (float)h1.y;
            *reinterpret_cast<float4 *>(lo + 4 * i) = l;
        }
        i0 += nq * 4;
    }
    for (long long i = i0; i < m; i += stride) lo[i] = (float)hi[i];
}

// 16-byte form: both pointers aligned and, with several right-hand sides, both leading dimensions whole packs
static bool mixed_vec(const void *hi, long long ld_hi_bytes, const void *lo, long long ld_lo_bytes, int nrhs) {
    if (!aligned16(hi) || (lo && !aligned16(lo))) return false;
    return nrhs <= 1 || (((ld_hi_bytes | ld_lo_bytes) & 15) == 0);
}
static bool mixed_dtype(int dtype_hi) { return dtype_hi == CGAMD_F64 || dtype_hi == CGAMD_C128; }

int launch_mixed_accumulate(int dtype_hi, int n, void *x_hi, long long ld_hi, const void *x_lo, long long ld_lo, const double *scale,
                            const int *mask, int nrhs, hipStream_t st) {
    if (!mixed_dtype(dtype_hi)) return fail(CGAMD_ERR_INVALID, "mixed_accumulate: bad dtype");
    if (n <= 0 || nrhs <= 0) return CGAMD_OK;
    if (ld_hi < n || ld_lo < n) return fail(CGAMD_ERR_INVALID, "mixed_accumulate: leading dimension below n");
    const int R = dtype_hi == CGAMD_F64 ? 1 : 2;
    const bool vec = mixed_vec(x_hi, ld_hi * 8 * R, x_lo, ld_lo * 4 * R, nrhs);
    dim3 g(mixed_grid((long long)n * R), nrhs), blk(kBlock);
#define CG_MIXED_ACC(HI, LO) (long long)n, (HI *)x_hi, ld_hi, (const LO *)x_lo, ld_lo, scale, mask
    if (dtype_hi == CGAMD_F64) {
        if (vec) hipLaunchKernelGGL((mixed_accumulate_kernel<double, float, true>), g, blk, 0, st, CG_MIXED_ACC(double, float));
        else hipLaunchKernelGGL((mixed_accumulate_kernel<double, float, false>), g, blk, 0, st, CG_MIXED_ACC(double, float));
    } else {
        if (vec) hipLaunchKernelGGL((mixed_accumulate_kernel<double2, float2, true>), g, blk, 0, st, CG_MIXED_ACC(double2, float2));
        else hipLaunchKernelGGL((mixed_accumulate_kernel<double2, float2, false>), g, blk, 0, st, CG_MIXED_ACC(double2, float2));
    }
#undef CG_MIXED_ACC
    return check_launch("mixed_accumulate");
}

int launch_mixed_round_down(int dtype_hi, int n, const void *r_hi, long long ld_hi, void *r_lo, long long ld_lo, const double *inv_scale,
                            int nrhs, hipStream_t st) {
    if (!mixed_dtype(dtype_hi)) return fail(CGAMD_ERR_INVALID, "mixed_round_down: bad dtype");
    if (n <= 0 || nrhs <= 0) return CGAMD_OK;
    if (ld_hi < n || ld_lo < n) return fail(CGAMD_ERR_INVALID, "mixed_round_down: leading dimension below n");
    const int R = dtype_hi == CGAMD_F64 ? 1 : 2;
    const bool vec = mixed_vec(r_hi, ld_hi * 8 * R, r_lo, ld_lo * 4 * R, nrhs);
    dim3 g(mixed_grid((long long)n * R), nrhs), blk(kBlock);
#define CG_MIXED_RD(HI, LO) (long long)n, (const HI *)r_hi, ld_hi, (LO *)r_lo, ld_lo, inv_scale
    if (dtype_hi == CGAMD_F64) {
        if (vec) hipLaunchKernelGGL((mixed_round_down_kernel<double, float, true>), g, blk, 0, st, CG_MIXED_RD(double, float));
        else hipLaunchKernelGGL((mixed_round_down_kernel<double, float, false>), g, blk, 0, st, CG_MIXED_RD(double, float));
    } else {
        if (vec) hipLaunchKernelGGL((mixed_round_down_kernel<double2, float2, true>), g, blk, 0, st, CG_MIXED_RD(double2, float2));
        else hipLaunchKernelGGL((mixed_round_down_kernel<double2, float2, false>), g, blk, 0, st, CG_MIXED_RD(double2, float2));
    }
#undef CG_MIXED_RD
    return check_launch("mixed_round_down");
}

int mixed_norm2_grid(int dtype_hi, int n) { return mixed_grid((long long)n * (dtype_hi == CGAMD_F64 ? 1 : 2)); }

int launch_mixed_norm2(int dtype_hi, int n, const void *v, long long ld, int nrhs, double *partials, double *out, hipStream_t st) {
    if (!mixed_dtype(dtype_hi)) return fail(CGAMD_ERR_INVALID, "mixed_norm2: bad dtype");
    if (n <= 0 || nrhs <= 0) return CGAMD_OK;
    if (ld < n) return fail(CGAMD_ERR_INVALID, "mixed_norm2: leading dimension below n");
    const int R = dtype_hi == CGAMD_F64 ? 1 : 2, G = mixed_norm2_grid(dtype_hi, n);
    const bool vec = mixed_vec(v, ld * 8 * R, nullptr, 0, nrhs);
    dim3 g(G, nrhs), blk(kBlock);
    const long long m = (long long)n * R;
    if (dtype_hi == CGAMD_F64) {
        if (vec) hipLaunchKernelGGL((mixed_norm2_kernel<double, true>), g, blk, 0, st, m, R, (const double *)v, ld, partials);
        else hipLaunchKernelGGL((mixed_norm2_kernel<double, false>), g, blk, 0, st, m, R, (const double *)v, ld, partials);
    } else {
        if (vec) hipLaunchKernelGGL((mixed_norm2_kernel<double2, true>), g, blk, 0, st, m, R, (const double2 *)v, ld, partials);
        else hipLaunchKernelGGL((mixed_norm2_kernel<double2, false>), g, blk, 0, st, m, R, (const double2 *)v, ld, partials);
    }
    if (int rc = check_launch("mixed_norm2")) return rc;
    hipLaunchKernelGGL(mixed_norm2_finish_kernel, dim3(nrhs), dim3(kWave), 0, st, (const double *)partials, G, out);
    return check_launch("mixed_norm2_finish");
}

int launch_mixed_round_values(int dtype_hi, long long count, const void *hi, void *lo, hipStream_t st) {
    if (!mixed_dtype(dtype_hi)) return fail(CGAMD_ERR_INVALID, "mixed_round_values: bad dtype");
    if (count <= 0) return CGAMD_OK;
    const long long m = count * (dtype_hi == CGAMD_F64 ? 1 : 2);
    const bool vec = aligned16(hi) && aligned16(lo);
    dim3 g(mixed_grid(m)), blk(kBlock);
    if (vec) hipLaunchKernelGGL((mixed_round_values_kernel<true>), g, blk, 0, st, m, (const double *)hi, (float *)lo);
    else hipLaunchKernelGGL((mixed_round_values_kernel<false>), g, blk, 0, st, m, (const double *)hi, (float *)lo);
    return check_launch("mixed_round_values");
}

}  // namespace cgamd
