// Multi-shift CG (Frommer; Jegerlehner): the systems (A + sigma_j I) x_j = b, j < S, ride on the seed recurrence of A x = b.  Their
// residuals are collinear with the seed's, r_k^j = zeta_k^j r_k, so the one SpMV of the seed's iteration serves all of them; a shift
// costs a few scalar operations and one pass over its own x_j and d_j.  Two launches behind the seed's d step (solver.cpp):
//   shift_scalars_kernel   one thread per (shift, right-hand side): from alpha_k, beta_k as the loop stored them
//                            theta' = alpha_{k-1} / (alpha_k beta_{k-1} (1 - theta) + alpha_{k-1} (1 + sigma_j alpha_k))
//                            zeta' = zeta theta',  alpha_j = alpha_k theta',  beta_j = beta_k theta' theta'
//                          in double / complex double (theta = zeta_k / zeta_{k-1}: the RATIO form -- zeta underflows to 0 for a
//                          well-shifted system, which here only switches the r term off, where the three-zeta form divides 0 / 0);
//                          alpha_j, beta_j, zeta' rounded once to the value type; zeta' appended to the shift history
//   shift_update_kernel    x_j = x_j + alpha_j d_j ; d_j = zeta' r + beta_j d_j  for ALL shifts in one launch: r is read once per
//                          element and kept in registers, every shift reads and writes its x_j and d_j once (4 S + 1 vector passes)
// Every thread of the scalar launch reads and writes the state of its own (j, r) only -- alpha_{k-1} and beta_{k-1} are kept per pair,
// not shared -- so no work-group reads a word another one writes; the vector launch only reads what the scalar launch left.
// Algebraic in alpha and beta, so the same code serves the unconjugated recurrence on complex-symmetric matrices with complex shifts.
// Grid and layout of vector.hip: 256 threads, right-hand sides on grid.y, 16-byte packs with a scalar tail, no atomics.
#include "cgamd_internal.h"
#include "device_mem.h"
#include "device_types.h"
#include "launch_util.h"
#include "stop_device.h"

#include <algorithm>

namespace cgamd {

constexpr int kShiftGroup = 4;      // shifts whose x_j and d_j packs one thread keeps in flight together: 8 loads of 16 bytes

template <typename A> CG_DEV A acc_one();
template <> CG_DEV double acc_one<double>() { return 1.; }
template <> CG_DEV double2 acc_one<double2>() { return make_double2(1., 0.); }

// set_rhs: theta = zeta = 1, alpha_{-1} = 1, beta_{-1} = 0, history row 0 all ones; one thread per (shift, right-hand side)
template <typename T>
__global__ __launch_bounds__(kWave) void shift_init_kernel(int count, typename VT<T>::acc *__restrict__ theta, typename VT<T>::acc *__restrict__ zeta,
                                                           typename VT<T>::acc *__restrict__ aprev, typename VT<T>::acc *__restrict__ bprev,
                                                           T *__restrict__ al_s, T *__restrict__ be_s, T *__restrict__ ze_s, T *__restrict__ hist) {
    using A = typename VT<T>::acc;
    const int t = blockIdx.x * kWave + threadIdx.x;
    if (t >= count) return;
    theta[t] = acc_one<A>();
    zeta[t] = acc_one<A>();
    aprev[t] = acc_one<A>();
    bprev[t] = vzero<A>();
    al_s[t] = vzero<T>();
    be_s[t] = vzero<T>();
    ze_s[t] = from_acc<T>(acc_one<A>());
    hist[t] = from_acc<T>(acc_one<A>());
}

// GUARD (cgamd_solver_iterate_until): the step follows the deciding launch and belongs to the stopping iteration, so it leaves on
// live[] like a beta-side launch (stop_device.h); a frozen pair repeats its zeta in the history rows the others go on to fill
template <typename T, bool GUARD>
__global__ __launch_bounds__(kWave) void shift_scalars_kernel(int nrhs, int S, const typename VT<T>::acc *__restrict__ sigma,
                                                              typename VT<T>::acc *__restrict__ theta, typename VT<T>::acc *__restrict__ zeta,
                                                              typename VT<T>::acc *__restrict__ aprev, typename VT<T>::acc *__restrict__ bprev,
                                                              const T *__restrict__ alpha, const T *__restrict__ beta, T *__restrict__ al_s,
                                                              T *__restrict__ be_s, T *__restrict__ ze_s, T *__restrict__ hist, int hist_cap,
                                                              const int *__restrict__ iter, CgStop g) {
    using A = typename VT<T>::acc;
    const int t = blockIdx.x * kWave + threadIdx.x;
    if (t >= S * nrhs) return;
    const int j = t / nrhs, r = t - j * nrhs;
    const int it = *iter;       // advanced by this iteration's alpha step
    const long long row = (long long)it * S * nrhs + t;
    if (GUARD && g.live[r] == 0) {
        if (it < hist_cap) hist[row] = from_acc<T>(zeta[t]);
        return;
    }
    const A one = acc_one<A>();
    const A al = to_acc(alpha[r]), be = to_acc(beta[r]), ap = aprev[t], bp = bprev[t], th = theta[t];
    const A den = vadd(vmul(vmul(al, bp), vsub(one, th)), vmul(ap, vadd(one, vmul(sigma[j], al))));
    const A tn = acc_div(ap, den);
    const A zn = vmul(zeta[t], tn);
    theta[t] = tn;
    zeta[t] = zn;
    aprev[t] = al;
    bprev[t] = be;
    al_s[t] = from_acc<T>(vmul(al, tn));
    be_s[t] = from_acc<T>(vmul(vmul(be, tn), tn));
    const T zT = from_acc<T>(zn);
    ze_s[t] = zT;
    if (it < hist_cap) hist[row] = zT;
}

// G shifts of one pack: their x_j and d_j loads go out together, then the arithmetic, then the stores.  c: the work-group's
// coefficients in LDS, [0 .. kShiftMax) alpha_j, then beta_j, then zeta'
template <typename T, int G, bool NT>
CG_DEV void shift_group(const Pack<T> &pr, T *x, T *d, long long pitch, const T *c) {
    constexpr int E = Pack<T>::N;
    Pack<T> px[G], pd[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        px[g] = NT ? ld_pack_nt(x + g * pitch) : ld_pack(x + g * pitch);
        pd[g] = NT ? ld_pack_nt(d + g * pitch) : ld_pack(d + g * pitch);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const T a = c[g], b = c[kShiftMax + g], z = c[2 * kShiftMax + g];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            px[g].v[k] = vadd(px[g].v[k], vmul(a, pd[g].v[k]));
            pd[g].v[k] = vadd(vmul(z, pr.v[k]), vmul(b, pd[g].v[k]));
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (NT) { st_pack_nt(x + g * pitch, px[g]); st_pack_nt(d + g * pitch, pd[g]); }
        else { st_pack(x + g * pitch, px[g]); st_pack(d + g * pitch, pd[g]); }
    }
}

// grid = (G, nrhs).  r: [nrhs][ld]; xs, ds: [S][nrhs][ld]; al_s, be_s, ze_s: [S][nrhs].  NT: x_j and d_j are touched by this launch
// alone, once per iteration, so they stream past the caches where the handle's x does (vec_nt bit 0); r is read again by the next r update
template <typename T, bool VEC, bool NT, bool GUARD>
__global__ __launch_bounds__(kBlock) void shift_update_kernel(int n, long long ld, int S, const T *__restrict__ rv, T *__restrict__ xs,
                                                              T *__restrict__ ds, const T *__restrict__ al_s, const T *__restrict__ be_s,
                                                              const T *__restrict__ ze_s, CgStop g) {
    __shared__ T c[3 * kShiftMax];
    const int r = blockIdx.y, nrhs = gridDim.y;
    if (GUARD && g.live[r] == 0) return;        // frozen before this iteration; uniform over the work-group, before the barrier
    if (threadIdx.x < 3 * kShiftMax) {
        const int w = threadIdx.x / kShiftMax, j = threadIdx.x - w * kShiftMax;
        const T *src = w == 0 ? al_s : w == 1 ? be_s : ze_s;
        c[threadIdx.x] = j < S ? src[(long long)j * nrhs + r] : vzero<T>();
    }
    __syncthreads();
    const long long off = (long long)r * ld, pitch = (long long)nrhs * ld;
    rv += off; xs += off; ds += off;
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * kBlock;
    long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            const Pack<T> pr = ld_pack(rv + i * E);
            int j = 0;
            for (; j + kShiftGroup <= S; j += kShiftGroup)
                shift_group<T, kShiftGroup, NT>(pr, xs + j * pitch + i * E, ds + j * pitch + i * E, pitch, c + j);
            for (; j < S; ++j) shift_group<T, 1, NT>(pr, xs + j * pitch + i * E, ds + j * pitch + i * E, pitch, c + j);
        }
        i0 += npack * E;  // scalar tail
    }
    for (long long i = i0; i < n; i += stride) {
        const T ri = rv[i];
        for (int j = 0; j < S; ++j) {
            T *x = xs + j * pitch, *d = ds + j * pitch;
            const T dv = d[i];
            x[i] = vadd(x[i], vmul(c[j], dv));
            d[i] = vadd(vmul(c[2 * kShiftMax + j], ri), vmul(c[kShiftMax + j], dv));
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
template <typename T> static int shift_init_impl(int nrhs, const ShiftScalars &sh, hipStream_t st) {
    using A = typename VT<T>::acc;
    const int count = sh.S * nrhs;
    hipLaunchKernelGGL((shift_init_kernel<T>), dim3((count + kWave - 1) / kWave), dim3(kWave), 0, st, count, (A *)sh.theta, (A *)sh.zeta, (A *)sh.aprev,
                       (A *)sh.bprev, (T *)sh.alpha_s, (T *)sh.beta_s, (T *)sh.zeta_s, (T *)sh.history);
    return check_launch("shift init");
}
int launch_shift_init(int dtype, int nrhs, const ShiftScalars &sh, hipStream_t st) {
    CG_DISPATCH(dtype, shift_init_impl, nrhs, sh, st);
}

template <typename T> static int shift_scalars_impl(int nrhs, const ShiftScalars &sh, const CgScalars &sc, hipStream_t st, const CgStop *stop) {
    using A = typename VT<T>::acc;
    const dim3 g((sh.S * nrhs + kWave - 1) / kWave), blk(kWave);
    const CgStop none;
#define CG_SS(G) hipLaunchKernelGGL((shift_scalars_kernel<T, G>), g, blk, 0, st, nrhs, sh.S, (const A *)sh.sigma, (A *)sh.theta, (A *)sh.zeta, (A *)sh.aprev, \
                                    (A *)sh.bprev, (const T *)sc.alpha, (const T *)sc.beta, (T *)sh.alpha_s, (T *)sh.beta_s, (T *)sh.zeta_s, (T *)sh.history, \
                                    sh.history_cap, (const int *)sc.iter, G ? *stop : none)
    if (stop) CG_SS(true); else CG_SS(false);
#undef CG_SS
    return check_launch("shift scalars");
}
int launch_shift_scalars(int dtype, int nrhs, const ShiftScalars &sh, const CgScalars &sc, hipStream_t st, const CgStop *stop) {
    CG_DISPATCH(dtype, shift_scalars_impl, nrhs, sh, sc, st, stop);
}

// one pack per thread per step, like the projection's combine pass (the measured kernel of the same shape: one base vector and many
// slot vectors); "vec_grid" overrides
static int shift_grid(int dtype, long long n) {
    const long long per_block = (long long)kBlock * (16 / (long long)dtype_size(dtype));
    long long g = (n + per_block - 1) / per_block;
    const long long cap = tune().vec_grid > 0 ? tune().vec_grid : kMaxGrid;
    if (g > cap) g = cap;
    return g < 1 ? 1 : (int)g;
}
template <typename T>
static int shift_update_impl(int n, long long ld, int nrhs, int S, const void *r, void *xs, void *ds, const void *al, const void *be, const void *ze,
                             bool vec, bool nt, hipStream_t st, const CgStop *stop) {
    const dim3 g(shift_grid(VT<T>::dtype, n), nrhs), blk(kBlock);
    const CgStop none;
#define CG_SU(V, N, G) hipLaunchKernelGGL((shift_update_kernel<T, V, N, G>), g, blk, 0, st, n, ld, S, (const T *)r, (T *)xs, (T *)ds, (const T *)al, \
                                          (const T *)be, (const T *)ze, G ? *stop : none)
    if (stop) { if (vec && nt) CG_SU(true, true, true); else if (vec) CG_SU(true, false, true); else CG_SU(false, false, true); }
    else if (vec && nt) CG_SU(true, true, false); else if (vec) CG_SU(true, false, false); else CG_SU(false, false, false);
#undef CG_SU
    return check_launch("shift update");
}
int launch_shift_update(int dtype, int n, long long ld, int nrhs, int S, const void *r, void *xs, void *ds, const void *alpha_s, const void *beta_s,
                        const void *zeta_s, hipStream_t st, int vec_nt, const CgStop *stop) {
    if (n <= 0 || S <= 0) return CGAMD_OK;
    if (S > kShiftMax) return fail(CGAMD_ERR_INVALID, "shift update: at most 16 shifts");
    // every (shift, right-hand side) vector starts ld values behind the one before
    const bool vec = vec_ok(dtype, ld, nrhs * S, {r, xs, ds});
    const int vnt = tune().vec_nt >= 0 ? tune().vec_nt : vec_nt;
    CG_DISPATCH(dtype, shift_update_impl, n, ld, nrhs, S, r, xs, ds, alpha_s, beta_s, zeta_s, vec, (vnt & 1) != 0, st, stop);
}

}  // namespace cgamd

// ---- context-level entry (development: the kernel test) ---------------------------------------------------------------------------
using namespace cgamd;

extern "C" int cgamd_shift_update(cgamd_ctx *ctx, int dtype, int size, long long ld, int nRHS, int nShifts, const void *r, void *xs, void *ds,
                                  const void *alpha_s, const void *beta_s, const void *zeta_s) {
    if (!ctx) return fail(CGAMD_ERR_INVALID, "shift_update: context is NULL");
    if (dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, "shift_update: bad dtype");
    if (size < 0 || nRHS < 1 || ld < size) return fail(CGAMD_ERR_INVALID, "shift_update: size >= 0, nRHS >= 1 and ld >= size are required");
    if (nShifts < 0 || nShifts > kShiftMax) return fail(CGAMD_ERR_INVALID, "shift_update: nShifts runs 0 ... 16");
    if (nShifts == 0 || size == 0) return CGAMD_OK;
    if (!r || !xs || !ds || !alpha_s || !beta_s || !zeta_s) return fail(CGAMD_ERR_INVALID, "shift_update: null pointer");
    thread_hip_setup();
    CG_HIP(hipSetDevice(ctx->device));
    if (int rc = stream_not_capturing(ctx->stream, "shift_update")) return rc;
    return launch_shift_update(dtype, size, ld, nRHS, nShifts, r, xs, ds, alpha_s, beta_s, zeta_s, ctx->stream, 0);
}
