// Solution projection (Fischer 1998): the streaming kernels behind cgamd_solver_set_rhs_projected / cgamd_solver_projection_update
// (solver.cpp) and the two context-level entries the kernel tests call.  The basis W holds `slots` vectors per right-hand side,
// slot j of right-hand side r at W + j * slot_pitch + r * ld; a bit mask names the slots that take part (the retired slot of a
// full ring is masked off).  Three plain streaming kernels -- 16-byte packs, one pack per lane per step, right-hand sides on
// grid.y, no atomics, nothing that waits on another work-group -- and two scalar kernels:
//   proj_dots_kernel     partials of c_j = <w_j, v> for a group of up to 8 live slots per pass over v (accumulators in registers)
//   proj_dots_sum_kernel one 1024-thread work-group per (slot, right-hand side): sum_partials_block, rounded once to the value type
//   proj_combine_kernel  y = (v | v - u | 0) + sign * sum_j c_j w_j, slots ascending, one vmul and one vadd / vsub per slot
//   proj_decide_kernel   s, the acceptance of every column, t = 1 / sqrt(nu) or 0, the `added` flags
//   proj_store_kernel    w_slot = e' * t (zeros for a refused column)
// Order of the sums (include/cgamd.h states it): that of dot_partials_kernel (vector.hip) per slot.
#include "cgamd_internal.h"
#include "device_mem.h"
#include "device_types.h"
#include "launch_util.h"
#include "reduce_device.h"

namespace cgamd {

constexpr int kProjGroup = 8;       // slots whose accumulators one pass over v keeps in registers

// the live slots in ascending order (kernel argument: indexed by uniform values only)
struct ProjSlots {
    int count = 0;
    int idx[kProjMaxSlots];
};
static ProjSlots live_slots(int slots, unsigned live_mask) {
    ProjSlots sl;
    for (int j = 0; j < slots && j < kProjMaxSlots; ++j)
        if (live_mask & (1u << j)) sl.idx[sl.count++] = j;
    for (int j = sl.count; j < kProjMaxSlots; ++j) sl.idx[j] = 0;
    return sl;
}

// G live slots, sl.idx[first .. first + G - 1]: partials[(slot * nrhs + r) * gridDim.x + work-group]
template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kBlock) void proj_dots_kernel(int n, const T *__restrict__ W, long long slot_pitch, long long ld,
                                                           const T *__restrict__ v, ProjSlots sl, int first,
                                                           typename VT<T>::acc *__restrict__ partials) {
    using A = typename VT<T>::acc;
    __shared__ A red[kBlock / kWave];
    const int r = blockIdx.y, nrhs = gridDim.y;
    v += (long long)r * ld;
    const T *w[G];
    A acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        w[g] = W + (long long)sl.idx[first + g] * slot_pitch + (long long)r * ld;
        acc[g] = vzero<A>();
    }
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * kBlock;
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            const Pack<T> pv = ld_pack(v + i * E);
            Pack<T> pw[G];
#pragma unroll
            for (int g = 0; g < G; ++g) pw[g] = ld_pack(w[g] + i * E);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int k = 0; k < E; ++k) acc[g] = vadd(acc[g], to_acc(vmul(pw[g].v[k], pv.v[k])));
        }
        i0 += npack * E;  // scalar tail
    }
    for (long long i = i0; i < n; i += stride) {
        const T vi = v[i];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = vadd(acc[g], to_acc(vmul(w[g][i], vi)));
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const A tot = block_sum<kBlock>(acc[g], red);
        if (threadIdx.x == 0) partials[((long long)sl.idx[first + g] * nrhs + r) * gridDim.x + blockIdx.x] = tot;
    }
}

// grid = (live slots, nrhs): out[slot * nrhs + r] = T(sum of the P partials of that pair)
template <typename T>
__global__ __launch_bounds__(kScalarBlock) void proj_dots_sum_kernel(const typename VT<T>::acc *__restrict__ partials, int P, ProjSlots sl,
                                                                     T *__restrict__ out) {
    using A = typename VT<T>::acc;
    __shared__ A smem[kScalarBlock / kWave];
    const int slot = sl.idx[blockIdx.x], r = blockIdx.y, nrhs = gridDim.y;
    const A s = sum_partials_block(partials + ((long long)slot * nrhs + r) * P, P, smem);
    if (threadIdx.x == 0) out[(long long)slot * nrhs + r] = from_acc<T>(s);
}

// y may be v (every element is read and written by one thread)
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void proj_combine_kernel(int n, const T *__restrict__ W, long long slot_pitch, long long ld, ProjSlots sl,
                                                              const T *v, const T *__restrict__ u, const T *__restrict__ c, int plus,
                                                              T *y) {
    const int r = blockIdx.y, nrhs = gridDim.y;
    const long long off = (long long)r * ld;
    W += off;
    y += off;
    if (v) v += off;
    if (u) u += off;
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * kBlock;
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            Pack<T> a;
            if (v) {
                a = ld_pack(v + i * E);
                if (u) {
                    const Pack<T> pu = ld_pack(u + i * E);
#pragma unroll
                    for (int k = 0; k < E; ++k) a.v[k] = vsub(a.v[k], pu.v[k]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k) a.v[k] = vzero<T>();
            }
#pragma unroll 4
            for (int j = 0; j < sl.count; ++j) {
                const int slot = sl.idx[j];
                const Pack<T> pw = ld_pack(W + (long long)slot * slot_pitch + i * E);
                const T cj = c[(long long)slot * nrhs + r];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const T p = vmul(cj, pw.v[k]);
                    if (plus) a.v[k] = vadd(a.v[k], p);
                    else a.v[k] = vsub(a.v[k], p);
                }
            }
            st_pack(y + i * E, a);
        }
        i0 += npack * E;  // scalar tail
    }
    for (long long i = i0; i < n; i += stride) {
        T a = vzero<T>();
        if (v) a = v[i];
        if (v && u) a = vsub(a, u[i]);
        for (int j = 0; j < sl.count; ++j) {
            const int slot = sl.idx[j];
            const T p = vmul(c[(long long)slot * nrhs + r], W[(long long)slot * slot_pitch + i]);
            if (plus) a = vadd(a, p);
            else a = vsub(a, p);
        }
        y[i] = a;
    }
}

// ---- the scalar step of the update ------------------------------------------------------------------------------------------
CG_DEV bool acc_finite(double a) { return isfinite(a); }
CG_DEV bool acc_finite(double2 a) { return isfinite(a.x) && isfinite(a.y); }
CG_DEV double acc_abs(double a) { return fabs(a); }
CG_DEV double acc_abs(double2 a) { return hypot(a.x, a.y); }
CG_DEV bool acc_positive(double a) { return a > 0.; }
CG_DEV bool acc_positive(double2) { return true; }      // the complex types ask for a finite nu above the threshold only
// 1 / sqrt(nu); complex: the principal square root, then Smith's division
CG_DEV double acc_rsqrt(double a) { return 1. / sqrt(a); }
CG_DEV double2 acc_rsqrt(double2 a) {
    const double m = hypot(a.x, a.y);
    double2 q;
    if (m == 0.) {
        q = make_double2(0., 0.);
    } else if (a.x >= 0.) {
        q.x = sqrt(0.5 * (m + a.x));
        q.y = a.y / (2. * q.x);
    } else {
        q.y = copysign(sqrt(0.5 * (m - a.x)), a.y);
        q.x = a.y / (2. * q.y);
    }
    return acc_div(make_double2(1., 0.), q);
}

// one thread per right-hand side of ONE work-group.  alpha / c: value type, [slot * nrhs + r]; held: the slots of the guess, live: the
// slots of c.  out_nus: nu[nrhs], then s[nrhs]
template <typename T>
__global__ __launch_bounds__(kWave) void proj_decide_kernel(int nrhs, int slots, unsigned held, unsigned live, const T *__restrict__ alpha,
                                                            const T *__restrict__ c, const typename VT<T>::acc *__restrict__ eq,
                                                            const typename VT<T>::acc *__restrict__ nu, double drop_tol,
                                                            typename VT<T>::acc *__restrict__ out_nus, T *__restrict__ t,
                                                            int *__restrict__ added) {
    using A = typename VT<T>::acc;
    for (int r = threadIdx.x; r < nrhs; r += kWave) {
        A aa = vzero<A>(), ac = vzero<A>();
        for (int j = 0; j < slots; ++j) {
            if (!(held & (1u << j))) continue;
            const A aj = to_acc(alpha[(long long)j * nrhs + r]);
            aa = vadd(aa, vmul(aj, aj));
            if (live & (1u << j)) ac = vadd(ac, vmul(aj, to_acc(c[(long long)j * nrhs + r])));
        }
        const A s = vadd(vadd(aa, vadd(ac, ac)), eq[r]);
        const A v = nu[r];
        const bool ok = acc_finite(v) && acc_positive(v) && acc_abs(v) > drop_tol * drop_tol * acc_abs(s);
        out_nus[r] = v;
        out_nus[nrhs + r] = s;
        if (ok) t[r] = from_acc<T>(acc_rsqrt(v));
        else t[r] = vzero<T>();
        added[r] = ok ? 1 : 0;
    }
}

// w[i] = e[i] * t[r] for an accepted column, 0 for a refused one (whatever e holds there)
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void proj_store_kernel(int n, const T *__restrict__ e, long long ld, const T *__restrict__ t,
                                                            const int *__restrict__ added, T *__restrict__ w) {
    const int r = blockIdx.y;
    e += (long long)r * ld;
    w += (long long)r * ld;
    const bool on = added[r] != 0;
    const T tr = t[r];
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * kBlock;
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            Pack<T> a;
            if (on) {
                a = ld_pack(e + i * E);
#pragma unroll
                for (int k = 0; k < E; ++k) a.v[k] = vmul(a.v[k], tr);
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k) a.v[k] = vzero<T>();
            }
            st_pack(w + i * E, a);
        }
        i0 += npack * E;
    }
    for (long long i = i0; i < n; i += stride) {
        if (on) w[i] = vmul(e[i], tr);
        else w[i] = vzero<T>();
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
int proj_dots_grid(int dtype, long long n) {
    // sized like vec_grid: one pack per thread for small systems, then 2, then 4; at most four work-groups per CU -- every thread keeps
    // up to nine 16-byte loads in flight, and every work-group adds a partial per slot to what the second launch sums
    const long long E = 16 / (long long)dtype_size(dtype), ppt = n <= 65536 ? 1 : n <= 524288 ? 2 : 4;
    const long long per_block = (long long)kBlock * E * ppt;
    long long g = (n + per_block - 1) / per_block;
    if (g > 1024) g = 1024;
    return g < 1 ? 1 : (int)g;
}
static int stream_grid(int dtype, long long n) {       // combine / store: one pack per thread per step
    const long long per_block = (long long)kBlock * (16 / (long long)dtype_size(dtype));
    long long g = (n + per_block - 1) / per_block;
    if (g > kMaxGrid) g = kMaxGrid;
    return g < 1 ? 1 : (int)g;
}
static bool proj_vec_ok(int dtype, long long ld, long long slot_pitch, int nrhs, std::initializer_list<const void *> ptrs) {
    return vec_ok(dtype, ld, nrhs, ptrs) && ((slot_pitch * (long long)dtype_size(dtype)) & 15) == 0;
}

template <typename T, int G>
static void dots_group(int n, const void *W, long long slot_pitch, long long ld, const void *v, const ProjSlots &sl, int first, void *partials,
                       dim3 g, bool vec, hipStream_t st) {
    auto *pp = static_cast<typename VT<T>::acc *>(partials);
    if (vec) hipLaunchKernelGGL((proj_dots_kernel<T, G, true>), g, dim3(kBlock), 0, st, n, (const T *)W, slot_pitch, ld, (const T *)v, sl, first, pp);
    else hipLaunchKernelGGL((proj_dots_kernel<T, G, false>), g, dim3(kBlock), 0, st, n, (const T *)W, slot_pitch, ld, (const T *)v, sl, first, pp);
}
template <typename T>
static int dots_impl(int n, long long ld, const ProjSlots &sl, const void *W, long long slot_pitch, const void *v, int nrhs, void *partials,
                     int grid, void *out, bool vec, hipStream_t st) {
    const dim3 g(grid, nrhs);
    for (int first = 0; first < sl.count; first += kProjGroup) {
        switch (std::min(kProjGroup, sl.count - first)) {
        case 1: dots_group<T, 1>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        case 2: dots_group<T, 2>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        case 3: dots_group<T, 3>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        case 4: dots_group<T, 4>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        case 5: dots_group<T, 5>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        case 6: dots_group<T, 6>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        case 7: dots_group<T, 7>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        default: dots_group<T, 8>(n, W, slot_pitch, ld, v, sl, first, partials, g, vec, st); break;
        }
        if (int rc = check_launch("projection dots")) return rc;
    }
    hipLaunchKernelGGL((proj_dots_sum_kernel<T>), dim3(sl.count, nrhs), dim3(kScalarBlock), 0, st,
                       static_cast<const typename VT<T>::acc *>(partials), grid, sl, static_cast<T *>(out));
    return check_launch("projection dots sum");
}
int launch_proj_dots(int dtype, int n, long long ld, int slots, unsigned live_mask, const void *W, long long slot_pitch, const void *v, int nrhs,
                     void *partials, int grid, void *out, hipStream_t st) {
    const ProjSlots sl = live_slots(slots, live_mask);
    if (sl.count == 0) return CGAMD_OK;
    const bool vec = proj_vec_ok(dtype, ld, slot_pitch, nrhs, {W, v});
    CG_DISPATCH(dtype, dots_impl, n, ld, sl, W, slot_pitch, v, nrhs, partials, grid, out, vec, st);
}

template <typename T>
static int combine_impl(int n, long long ld, const ProjSlots &sl, const void *W, long long slot_pitch, const void *v, const void *u, const void *c,
                        int sign, void *y, int nrhs, bool vec, hipStream_t st) {
    const dim3 g(stream_grid(VT<T>::dtype, n), nrhs);
    const int plus = sign >= 0 ? 1 : 0;
    if (vec)
        hipLaunchKernelGGL((proj_combine_kernel<T, true>), g, dim3(kBlock), 0, st, n, (const T *)W, slot_pitch, ld, sl, (const T *)v, (const T *)u,
                           (const T *)c, plus, (T *)y);
    else
        hipLaunchKernelGGL((proj_combine_kernel<T, false>), g, dim3(kBlock), 0, st, n, (const T *)W, slot_pitch, ld, sl, (const T *)v, (const T *)u,
                           (const T *)c, plus, (T *)y);
    return check_launch("projection combine");
}
int launch_proj_combine(int dtype, int n, long long ld, int slots, unsigned live_mask, const void *W, long long slot_pitch, const void *v,
                        const void *u, const void *c, int sign, void *y, int nrhs, hipStream_t st) {
    const ProjSlots sl = live_slots(slots, live_mask);
    const bool vec = proj_vec_ok(dtype, ld, slot_pitch, nrhs, {W, v, u, y});
    CG_DISPATCH(dtype, combine_impl, n, ld, sl, W, slot_pitch, v, u, c, sign, y, nrhs, vec, st);
}

template <typename T>
static int decide_impl(int nrhs, int slots, unsigned held, unsigned live, const void *alpha, const void *c, const void *eq, const void *nu,
                       double drop_tol, void *out_nus, void *t, int *added, hipStream_t st) {
    using A = typename VT<T>::acc;
    hipLaunchKernelGGL((proj_decide_kernel<T>), dim3(1), dim3(kWave), 0, st, nrhs, slots, held, live, (const T *)alpha, (const T *)c, (const A *)eq,
                       (const A *)nu, drop_tol, (A *)out_nus, (T *)t, added);
    return check_launch("projection decide");
}
int launch_proj_decide(int dtype, int nrhs, int slots, unsigned held, unsigned live, const void *alpha, const void *c, const void *eq,
                       const void *nu, double drop_tol, void *out_nus, void *t, int *added, hipStream_t st) {
    CG_DISPATCH(dtype, decide_impl, nrhs, slots, held, live, alpha, c, eq, nu, drop_tol, out_nus, t, added, st);
}

template <typename T>
static int store_impl(int n, const void *e, long long ld, const void *t, const int *added, void *w, int nrhs, bool vec, hipStream_t st) {
    const dim3 g(stream_grid(VT<T>::dtype, n), nrhs);
    if (vec) hipLaunchKernelGGL((proj_store_kernel<T, true>), g, dim3(kBlock), 0, st, n, (const T *)e, ld, (const T *)t, added, (T *)w);
    else hipLaunchKernelGGL((proj_store_kernel<T, false>), g, dim3(kBlock), 0, st, n, (const T *)e, ld, (const T *)t, added, (T *)w);
    return check_launch("projection store");
}
int launch_proj_store(int dtype, int n, const void *e, long long ld, const void *t, const int *added, void *w, int nrhs, hipStream_t st) {
    const bool vec = vec_ok(dtype, ld, nrhs, {e, w});
    CG_DISPATCH(dtype, store_impl, n, e, ld, t, added, w, nrhs, vec, st);
}

}  // namespace cgamd

// ---- context-level entries (development: the kernel tests) ----------------------------------------------------------------------
using namespace cgamd;

static int proj_op_check(cgamd_ctx *c, int dtype, int size, long long ld, int slots, int nRHS, const char *who) {
    if (!c) return fail(CGAMD_ERR_INVALID, std::string(who) + ": context is NULL");
    if (dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, std::string(who) + ": bad dtype");
    if (size < 0 || nRHS < 1 || ld < size) return fail(CGAMD_ERR_INVALID, std::string(who) + ": size >= 0, nRHS >= 1 and ld >= size are required");
    if (slots < 0 || slots > kProjMaxSlots) return fail(CGAMD_ERR_INVALID, std::string(who) + ": slots runs 0 ... 32");
    thread_hip_setup();
    CG_HIP(hipSetDevice(c->device));
    return stream_not_capturing(c->stream, who);
}

extern "C" {

int cgamd_projection_dots_grid(int dtype, int size) {
    if (dtype < 0 || dtype > 3 || size < 0) return -fail(CGAMD_ERR_INVALID, "projection_dots_grid: bad dtype or size");
    return proj_dots_grid(dtype, size);
}

int cgamd_projection_dots(cgamd_ctx *ctx, int dtype, int size, long long ld, int slots, unsigned live_mask, const void *W, long long slot_pitch,
                          const void *v, int nRHS, void *out) {
    if (int rc = proj_op_check(ctx, dtype, size, ld, slots, nRHS, "projection_dots")) return rc;
    if (slots == 0) return CGAMD_OK;
    if (!W || !v || !out) return fail(CGAMD_ERR_INVALID, "projection_dots: null pointer");
    const int grid = proj_dots_grid(dtype, size);
    const size_t bytes = acc_size(dtype) * (size_t)slots * nRHS * grid;
    if (ctx->partials_bytes < bytes) {
        if (ctx->partials) {
            CG_HIP(hipStreamSynchronize(ctx->stream));
            CG_HIP(hipFree(ctx->partials));
            ctx->partials = nullptr;
            ctx->partials_bytes = 0;
        }
        const hipError_t e = hipMalloc(&ctx->partials, bytes);
        if (e != hipSuccess) return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(partials): ") + hipGetErrorString(e));
        ctx->partials_bytes = bytes;
    }
    return launch_proj_dots(dtype, size, ld, slots, live_mask, W, slot_pitch, v, nRHS, ctx->partials, grid, out, ctx->stream);
}

int cgamd_projection_combine(cgamd_ctx *ctx, int dtype, int size, long long ld, int slots, unsigned live_mask, const void *W, long long slot_pitch,
                             const void *v, const void *c, int sign, void *y, int nRHS) {
    if (int rc = proj_op_check(ctx, dtype, size, ld, slots, nRHS, "projection_combine")) return rc;
    if (sign != 1 && sign != -1) return fail(CGAMD_ERR_INVALID, "projection_combine: sign is +1 or -1");
    if (!y || (slots > 0 && (!W || !c))) return fail(CGAMD_ERR_INVALID, "projection_combine: null pointer");
    return launch_proj_combine(dtype, size, ld, slots, live_mask, W, slot_pitch, v, nullptr, c, sign, y, nRHS, ctx->stream);
}

}  // extern "C"
