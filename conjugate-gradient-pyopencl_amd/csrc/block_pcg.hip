// Preconditioned block CG: BCGrQ (block_cg.hip) carried in the M^-1 inner product.  R = Q xi with Q^T M^-1 Q = I; the handle's
// vectors carry the block as there -- x = X, r = Q, d = P, q = A P -- and q's storage also holds Z = M^-1 W, because A P is dead once
// W exists (the scalar PCG loops of solver.cpp keep z there too).  No n-sized buffer is added.  An iteration is the handle's SpMV,
// three launches of block_cg.hip as they are (the Gram of P^T A P, the G step, the x / w update with the partials of W^T W) and
// (include/cgamd.h "Preconditioned block CG"; solver.cpp):
//   z = M^-1 w into q          the V-cycle or the line sweeps; NOTHING for a diagonal M
//   the partials of C = W^T Z  block_gram_kernel(W, Z), or for a diagonal M block_gram_weighted_kernel: W read once, m once, no Z block
//   block_pcg_small_kernel     (W step) both sums; delta_k[j] = (xi e_j)^T (W^T W) (xi e_j) with the OLD xi (R_k+1 = W xi_k) into the
//                              history, the stop; C = L L^T, tau = L^T, tau^-1, xi <- tau xi
//   block_qp_z_kernel          Q <- W tau^-1 ; P <- Z tau^-1 + P tau^T, both in place; z_k read from Z, or m_i w_k rounded once
// The rules are block_cg.hip's: one thread owns a row's s values (s a template parameter), one path for every alignment of ld; the
// factors in LDS in the value type, each rounded once from the double the small step formed; every sum in a fixed order
// (tests/block_pcg_ref.py restates all of it); -ffp-contract=off; the freeze word written by the small steps only and read by every
// launch behind them.
// Registers (s = 16, double): the weighted Gram holds the 136 accumulators of block_gram_kernel (272 VGPRs) beside 2 x 16 values; a
// second accumulator set inside block_xw_kernel would be 272 more and spill, which is why W^T Z has a launch of its own.  The q / p
// launch holds three rows of 16 (w, z, p); its 2 s^2 factors stay in LDS behind lds_stays(), broadcast reads (all lanes one address).
#include "block_device.h"
#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"
#include "reduce_device.h"
#include "stop_device.h"

namespace cgamd {

// w: [S][ld], m: [n]; part: [S (S + 1) / 2][grid], entry j (j + 1) / 2 + i = w_i . (m w_j) (i <= j), in gram_add's order
template <typename T, int S>
__global__ __launch_bounds__(kBlock) void block_gram_weighted_kernel(int n, long long ld, const T *__restrict__ w, const T *__restrict__ m,
                                                                     double *__restrict__ part, const int *__restrict__ frozen) {
    constexpr int NP = S * (S + 1) / 2;
    __shared__ double sm[NP * 4];
    if (frozen && *frozen) return;
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const T mi = m[i];
        T wv[S], zv[S];
#pragma unroll
        for (int j = 0; j < S; ++j) { wv[j] = w[j * ld + i]; zv[j] = mi * wv[j]; }
        gram_add<T, S>(wv, zv, acc);
    }
    gram_store<NP>(acc, sm, part);
}

// Q <- W tau^-1 (W in Q's storage) ; P <- Z tau^-1 + P tau^T (init: P <- Z tau^-1).  TI = tau^-1, TA = tau: upper triangular [S][S]
// row-major.  Z: [S][ld], or NULL and z_k = m_i w_k
template <typename T, int S>
__global__ __launch_bounds__(kBlock) void block_qp_z_kernel(int n, long long ld, T *__restrict__ Q, T *__restrict__ P, const T *__restrict__ Z,
                                                            const T *__restrict__ m, const T *__restrict__ TI, const T *__restrict__ TA, int init,
                                                            const int *__restrict__ frozen) {
    __shared__ T ti[S * S], ta[S * S];
    if (frozen && *frozen) return;
    for (int t = threadIdx.x; t < S * S; t += kBlock) { ti[t] = TI[t]; ta[t] = TA[t]; }
    __syncthreads();
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        lds_stays();
        T w[S], z[S], p[S];
#pragma unroll
        for (int j = 0; j < S; ++j) w[j] = Q[j * ld + i];
        if (Z) {
#pragma unroll
            for (int j = 0; j < S; ++j) z[j] = Z[j * ld + i];
        } else {
            const T mi = m[i];
#pragma unroll
            for (int j = 0; j < S; ++j) z[j] = mi * w[j];
        }
        if (!init) {
#pragma unroll
            for (int j = 0; j < S; ++j) p[j] = P[j * ld + i];
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            T v = w[0] * ti[j], y = z[0] * ti[j];
#pragma unroll
            for (int k = 1; k <= j; ++k) { v = v + w[k] * ti[k * S + j]; y = y + z[k] * ti[k * S + j]; }
            Q[j * ld + i] = v;
            if (!init) {
#pragma unroll
                for (int k = j; k < S; ++k) y = y + p[k] * ta[j * S + k];
            }
            P[j * ld + i] = y;
        }
    }
}

// ---- the small step of the preconditioned form: one work-group of 1024 threads, everything in double ------------------------------
// mode 0: set_rhs (xi = I: delta_0[j] = (R0^T R0)_jj; C = R0^T Z0 = L L^T, xi = L^T; resets the record and the counter), 2: the W step.
// (The G step is block_small_kernel's mode 1 as it is.)  part: the partials of W^T W, part_z: of W^T Z
template <typename T>
__global__ __launch_bounds__(kScalarBlock) void block_pcg_small_kernel(int mode, int S, int grid, const double *__restrict__ part,
                                                                       const double *__restrict__ part_z, BlockDev bd, int *iter,
                                                                       T *__restrict__ history, int hist_cap, CgStop g, int has_stop) {
    __shared__ double C[kBlockMax * kBlockLd], D[kBlockMax * kBlockLd], L[kBlockMax * kBlockLd], X[kBlockMax * kBlockLd], XI[kBlockMax * kBlockLd];
    __shared__ int sh_status, sh_frozen;
    __shared__ double sh_ratio;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const double eps = sizeof(T) == 4 ? 0x1p-23 : 0x1p-52;
    if (tid == 0) sh_frozen = mode == 0 ? 0 : bd.rec[2];
    __syncthreads();
    if (sh_frozen) {        // (a block that broke down in set_rhs meets the host's word here, armed after it)
        if (tid == 0 && has_stop) *g.nactive = 0;
        return;
    }
    // the entries of both matrices, each by one wave: lane-strided over the partials, then the wave tree
    const int NP = S * (S + 1) / 2;
    for (int p = wv; p < 2 * NP; p += kScalarBlock / kWave) {
        const int e = p < NP ? p : p - NP;
        const double *src = p < NP ? part : part_z;
        small_sum_entry(src, grid, e, lane, p < NP ? D : C);
    }
    if (tid < S * S) {
        const int i = tid / S, j = tid - i * S;
        XI[i * kBlockLd + j] = mode == 0 ? (i == j ? 1. : 0.) : bd.xi[tid];
    }
    __syncthreads();
    if (tid < S * S) {
        bd.C[tid] = D[(tid / S) * kBlockLd + tid % S];
        bd.CZ[tid] = C[(tid / S) * kBlockLd + tid % S];
    }
    const int it = mode == 0 ? 0 : *iter;       // mode 2: advanced by this iteration's G step
    // delta_k[tid] = (xi e_tid)^T (W^T W) (xi e_tid) with the xi this step found (R_k+1 = W xi_k): t_i = sum_m<=j D_im xi_mj, then
    // sum_i<=j xi_ij t_i, every sum from its first product on, ascending.  Column tid's side of the stop
    int done = 1;
    if (tid < S) {
        const int j = tid;
        double acc = D[j * kBlockLd + j];
        if (mode != 0) {
            for (int i = 0; i <= j; ++i) {
                double t = D[i * kBlockLd] * XI[j];
                for (int m = 1; m <= j; ++m) t = t + D[i * kBlockLd + m] * XI[m * kBlockLd + j];
                acc = i == 0 ? XI[j] * t : acc + XI[i * kBlockLd + j] * t;
            }
        }
        const T dT = (T)acc;
        if (it < hist_cap) history[(long long)it * S + tid] = dT;
        done = has_stop && mode == 2 ? !(stop_norm(dT) >= g.tol[tid]) : 0;
    }
    if (tid == 0) {         // Cholesky of C = W^T Z, left-looking by columns, with the pivot rule
        double ratio = mode == 0 ? (double)INFINITY : *bd.min_ratio;
        const int status = small_cholesky(C, L, S, eps, 2, ratio);
        sh_status = status;
        sh_ratio = ratio;
    }
    const int all = __syncthreads_and(done);
    if (sh_status) {        // breakdown: the record, the freeze, the host's word; X stays the last complete iterate
        if (tid == 0) {
            bd.rec[0] = sh_status;
            bd.rec[1] = it;
            bd.rec[2] = 1;
            *bd.min_ratio = sh_ratio;
            if (mode == 0) *iter = 0;
            if (has_stop) *g.nactive = 0;
        }
        return;
    }
    if (tid < S) small_linv_column(L, X, S, tid);
    __syncthreads();
    // tau = L^T, tau^-1 = X^T, xi <- tau xi
    if (tid < S * S) {
        const int i = tid / S, j = tid - (tid / S) * S;
        const double t = i <= j ? L[j * kBlockLd + i] : 0., tinv = i <= j ? X[j * kBlockLd + i] : 0.;
        bd.tau[tid] = t;
        bd.tau_inv[tid] = tinv;
        static_cast<T *>(bd.tau_T)[tid] = (T)t;
        static_cast<T *>(bd.tinv_T)[tid] = (T)tinv;
        double acc = 0.;
        if (i <= j) {
            acc = L[i * kBlockLd + i] * XI[i * kBlockLd + j];
            for (int m = i + 1; m <= j; ++m) acc = acc + L[m * kBlockLd + i] * XI[m * kBlockLd + j];
        }
        bd.xi[tid] = acc;
    }
    if (tid == 0) {
        *bd.min_ratio = sh_ratio;
        if (mode == 0) { bd.rec[0] = 0; bd.rec[1] = 0; bd.rec[2] = 0; *iter = 0; }
    }
    if (all) {              // every column satisfies its own tolerance: all stop here
        if (tid < S) g.stop[tid] = it;
        if (tid == 0) { bd.rec[2] = 1; *g.nactive = 0; }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
template <typename T>
static int block_gram_weighted_impl(int n, long long ld, int S, const void *w, const void *m, double *part, int grid, const int *frozen, hipStream_t st) {
#define CG_BGW(N) hipLaunchKernelGGL((block_gram_weighted_kernel<T, N>), dim3(grid), dim3(kBlock), 0, st, n, ld, (const T *)w, (const T *)m, part, frozen)
    CG_BLOCK_S(S, CG_BGW)
#undef CG_BGW
    return check_launch("block weighted gram");
}
template <typename T>
static int block_qp_z_impl(int n, long long ld, int S, void *Q, void *P, const void *Z, const void *m, const void *TI, const void *TA, int init, int grid,
                           const int *frozen, hipStream_t st) {
#define CG_BQZ(N) hipLaunchKernelGGL((block_qp_z_kernel<T, N>), dim3(grid), dim3(kBlock), 0, st, n, ld, (T *)Q, (T *)P, (const T *)Z, (const T *)m, \
                                     (const T *)TI, (const T *)TA, init, frozen)
    CG_BLOCK_S(S, CG_BQZ)
#undef CG_BQZ
    return check_launch("block update q, p with z");
}
template <typename T>
static int block_pcg_small_impl(int mode, int S, int grid, const BlockDev &bd, const CgScalars &sc, const CgStop *stop, hipStream_t st) {
    const CgStop none;
    hipLaunchKernelGGL((block_pcg_small_kernel<T>), dim3(1), dim3(kScalarBlock), 0, st, mode, S, grid, bd.partials, bd.partials_z, bd, sc.iter,
                       (T *)sc.history, sc.history_cap, stop ? *stop : none, stop ? 1 : 0);
    return check_launch("block small step (preconditioned)");
}

int launch_block_gram_weighted(int dtype, int n, long long ld, int S, const void *w, const void *m, double *part, int grid, const int *frozen,
                               hipStream_t st) {
    CG_BLOCK_REAL(dtype, block_gram_weighted_impl, n, ld, S, w, m, part, grid, frozen, st);
}
int launch_block_qp_z(int dtype, int n, long long ld, int S, void *Q, void *P, const void *Z, const void *m, const void *TI, const void *TA, bool init,
                      const int *frozen, hipStream_t st) {
    if ((Z == nullptr) == (m == nullptr)) return fail(CGAMD_ERR_INVALID, "block update q, p with z: exactly one of z and m");
    CG_BLOCK_REAL(dtype, block_qp_z_impl, n, ld, S, Q, P, Z, m, TI, TA, init ? 1 : 0, block_gram_grid(n), frozen, st);
}
int launch_block_pcg_small(int dtype, int mode, const BlockState &b, const CgScalars &sc, const CgStop *stop, hipStream_t st) {
    if (!b.dev.CZ || (mode != 0 && mode != 2)) return fail(CGAMD_ERR_STATE, "block small step (preconditioned): not set up, or no such mode");
    CG_BLOCK_REAL(dtype, block_pcg_small_impl, mode, b.S, b.grid, b.dev, sc, stop, st);
}

// W^T Z as summed (s x s doubles) and the partials of its entries
int block_pcg_alloc(BlockState *b) {
    if (b->mem_pcg) return CGAMD_OK;
    if (!b->mem) return fail(CGAMD_ERR_STATE, "block CG state: not allocated");
    const size_t mat = (size_t)kBlockMax * kBlockMax * sizeof(double), np = (size_t)b->S * (b->S + 1) / 2;
    void *mem = nullptr;
    if (int rc = dmalloc(&mem, mat + np * b->grid * sizeof(double), "preconditioned block CG state")) return rc;
    b->mem_pcg = mem;
    b->dev.CZ = static_cast<double *>(mem);
    b->dev.partials_z = reinterpret_cast<double *>(static_cast<char *>(mem) + mat);
    return CGAMD_OK;
}

}  // namespace cgamd

// ---- context-level entries (development: the kernel test) -----------------------------------------------------------------------------
using namespace cgamd;

static int block_pcg_entry(cgamd_ctx *ctx, const char *who, int dtype, int size, long long ld, int s) {
    const std::string w = who;
    if (!ctx) return fail(CGAMD_ERR_INVALID, w + ": context is NULL");
    if (dtype != CGAMD_F32 && dtype != CGAMD_F64) return fail(CGAMD_ERR_INVALID, w + ": block CG serves the real value types");
    if (size < 1 || ld < size) return fail(CGAMD_ERR_INVALID, w + ": size >= 1 and ld >= size are required");
    if (s < 2 || s > kBlockMax) return fail(CGAMD_ERR_INVALID, w + ": the block size runs 2 ... 16");
    thread_hip_setup();
    CG_HIP(hipSetDevice(ctx->device));
    return stream_not_capturing(ctx->stream, who);
}

extern "C" int cgamd_block_gram_weighted(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, const void *w, const void *m, void *partials) {
    if (int rc = block_pcg_entry(ctx, "block_gram_weighted", dtype, size, ld, s)) return rc;
    if (!w || !m || !partials) return fail(CGAMD_ERR_INVALID, "block_gram_weighted: null pointer");
    return launch_block_gram_weighted(dtype, size, ld, s, w, m, static_cast<double *>(partials), block_gram_grid(size), nullptr, ctx->stream);
}

extern "C" int cgamd_block_update_qp_z(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, void *q, void *p, const void *z, const void *m,
                                       const void *tau_inv, const void *tau, int init) {
    if (int rc = block_pcg_entry(ctx, "block_update_qp_z", dtype, size, ld, s)) return rc;
    if (!q || !p || !tau_inv || !tau) return fail(CGAMD_ERR_INVALID, "block_update_qp_z: null pointer");
    if ((z == nullptr) == (m == nullptr)) return fail(CGAMD_ERR_INVALID, "block_update_qp_z: exactly one of z and m is given");
    return launch_block_qp_z(dtype, size, ld, s, q, p, z, m, tau_inv, tau, init != 0, nullptr, ctx->stream);
}
