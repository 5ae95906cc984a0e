// Block CG (O'Leary 1980) in the residual-orthonormalised form (Dubrulle 2001, "BCGrQ"): the s = nRHS right-hand sides of one real SPD
// matrix search the sum of their Krylov spaces.  The handle's vectors carry the block -- x = X, r = Q (R = Q xi), d = P, q = A P -- and
// an iteration is the handle's SpMV and five launches of this file, a linear chain (include/cgamd.h "Block CG"; solver.cpp):
//   block_gram_kernel    the partials of the s (s + 1) / 2 distinct entries of G = P^T (A P)
//   block_small_kernel   (G step)  their sum, G = L L^T, alpha = G^-1, M = alpha xi; one work-group, in double
//   block_xw_kernel      X += P M ; W = Q - (A P) alpha over Q ; the partials of W^T W.  P, AP, X, Q read once, X and Q written once
//   block_small_kernel   (W step)  W^T W = L L^T, tau = L^T, tau^-1, xi <- tau xi, delta_k[j] = |xi e_j|^2 into the history, the stop
//   block_qp_kernel      Q <- W tau^-1 ; P <- Q + P tau^T, both in place
// One thread owns a row's s values of each block (s is a template parameter: they live in registers), consecutive threads own
// consecutive rows, so every load and store of a column is coalesced whatever the leading dimension: one path for every alignment.
// The s x s factors of the vector launches sit in LDS, in the value type, each rounded once from the double the small step formed.
// Every sum has a fixed order (tests/block_ref.py restates all of it): a thread adds the products of its rows in row order, in
// double; block_sum's order per work-group (wave tree, then the wave sums in order); the small step adds the partials of an entry
// lane-strided in one wave, then the wave tree; the factorisations run left-looking by columns, every inner sum in index order.
// -ffp-contract=off: one rounding per operation, in the vectors and in the small matrices alike.
// FREEZE: a breakdown (a pivot v of either Cholesky with not v > s eps max_j C_jj, or NaN) and the stop of iterate_until set
// rec.frozen.  It is written by the small steps only (one work-group) and is the exit of every launch BEHIND the one that wrote it;
// no launch reads a word that one of its own work-groups writes.
#include "block_device.h"
#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"
#include "reduce_device.h"
#include "stop_device.h"

#include <algorithm>

namespace cgamd {

constexpr int kGramGridMax = 512;       // one work-group per CU holds the accumulators; two passes over the chip at the most

int block_gram_grid(long long n) { return (int)std::max(1LL, std::min((n + kBlock - 1) / kBlock, (long long)kGramGridMax)); }

// a, b: [S][ld]; part: [S (S + 1) / 2][grid], entry j (j + 1) / 2 + i = a_i . b_j (i <= j)
template <typename T, int S>
__global__ __launch_bounds__(kBlock) void block_gram_kernel(int n, long long ld, const T *__restrict__ a, const T *__restrict__ b,
                                                            double *__restrict__ part, const int *__restrict__ frozen) {
    constexpr int NP = S * (S + 1) / 2;
    __shared__ double sm[NP * 4];
    if (frozen && *frozen) return;
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        T av[S], bv[S];
#pragma unroll
        for (int j = 0; j < S; ++j) { av[j] = a[j * ld + i]; bv[j] = b[j * ld + i]; }
        gram_add<T, S>(av, bv, acc);
    }
    gram_store<NP>(acc, sm, part);
}

// X += P M ; W = Q - AP alpha, written over Q ; part: the partials of W^T W.  M, AL: [S][S] row-major in the value type
template <typename T, int S>
__global__ __launch_bounds__(kBlock) void block_xw_kernel(int n, long long ld, const T *__restrict__ P, const T *__restrict__ AP, T *__restrict__ X,
                                                          T *__restrict__ Q, const T *__restrict__ M, const T *__restrict__ AL,
                                                          double *__restrict__ part, const int *__restrict__ frozen) {
    constexpr int NP = S * (S + 1) / 2;
    __shared__ double sm[NP * 4];
    __shared__ T m[S * S], al[S * S];
    if (frozen && *frozen) return;
    for (int t = threadIdx.x; t < S * S; t += kBlock) { m[t] = M[t]; al[t] = AL[t]; }
    __syncthreads();
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        lds_stays();
        // k outside, j inside: every x_j and w_j still takes its terms in the order k = 0, 1, ..., one rounding per multiply and per
        // add, but the s chains advance side by side and a row of the factor is s consecutive values of LDS
        T w[S], c[S];
#pragma unroll
        for (int j = 0; j < S; ++j) { c[j] = P[j * ld + i]; w[j] = X[j * ld + i]; }
#pragma unroll
        for (int k = 0; k < S; ++k) {
#pragma unroll
            for (int j = 0; j < S; ++j) w[j] = w[j] + c[k] * m[k * S + j];
        }
#pragma unroll
        for (int j = 0; j < S; ++j) { X[j * ld + i] = w[j]; c[j] = AP[j * ld + i]; w[j] = Q[j * ld + i]; }
#pragma unroll
        for (int k = 0; k < S; ++k) {
#pragma unroll
            for (int j = 0; j < S; ++j) w[j] = w[j] - c[k] * al[k * S + j];
        }
#pragma unroll
        for (int j = 0; j < S; ++j) Q[j * ld + i] = w[j];
        gram_add<T, S>(w, w, acc);
    }
    gram_store<NP>(acc, sm, part);
}

// Q <- W tau^-1 (W in Q's storage) ; P <- Q + P tau^T (init: P <- Q).  TI = tau^-1, TA = tau: upper triangular [S][S] row-major
template <typename T, int S>
__global__ __launch_bounds__(kBlock) void block_qp_kernel(int n, long long ld, T *__restrict__ Q, T *__restrict__ P, const T *__restrict__ TI,
                                                          const T *__restrict__ TA, int init, const int *__restrict__ frozen) {
    __shared__ T ti[S * S], ta[S * S];
    if (frozen && *frozen) return;
    for (int t = threadIdx.x; t < S * S; t += kBlock) { ti[t] = TI[t]; ta[t] = TA[t]; }
    __syncthreads();
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        lds_stays();
        T w[S], p[S];
#pragma unroll
        for (int j = 0; j < S; ++j) w[j] = Q[j * ld + i];
        if (!init) {
#pragma unroll
            for (int j = 0; j < S; ++j) p[j] = P[j * ld + i];
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            T v = w[0] * ti[j];
#pragma unroll
            for (int k = 1; k <= j; ++k) v = v + w[k] * ti[k * S + j];
            Q[j * ld + i] = v;
            if (!init) {
#pragma unroll
                for (int k = j; k < S; ++k) v = v + p[k] * ta[j * S + k];
            }
            P[j * ld + i] = v;
        }
    }
}

// ---- the small steps: one work-group of 1024 threads, everything in double -----------------------------------------------------------
// mode 0: set_rhs (the W step on R0^T R0 with xi = I; resets the record and the counter, never frozen), 1: the G step, 2: the W step
template <typename T>
__global__ __launch_bounds__(kScalarBlock) void block_small_kernel(int mode, int S, int grid, const double *__restrict__ part, BlockDev bd, int *iter,
                                                                   T *__restrict__ history, int hist_cap, CgStop g, int has_stop) {
    __shared__ double C[kBlockMax * kBlockLd], L[kBlockMax * kBlockLd], X[kBlockMax * kBlockLd], A2[kBlockMax * kBlockLd], XI[kBlockMax * kBlockLd];
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
    // the entries, each by one wave: lane-strided over the partials, then the wave tree
    const int NP = S * (S + 1) / 2;
    for (int p = wv; p < NP; p += kScalarBlock / kWave) small_sum_entry(part, grid, p, lane, C);
    if (tid < S * S) {
        const int i = tid / S, j = tid - i * S;
        XI[i * kBlockLd + j] = mode == 0 ? (i == j ? 1. : 0.) : bd.xi[tid];
    }
    __syncthreads();
    if (tid < S * S) (mode == 1 ? bd.G : bd.C)[tid] = C[(tid / S) * kBlockLd + tid % S];
    if (tid == 0) {         // Cholesky, left-looking by columns, with the pivot rule
        double ratio = mode == 0 ? (double)INFINITY : *bd.min_ratio;
        const int status = small_cholesky(C, L, S, eps, mode == 1 ? 1 : 2, ratio);
        sh_status = status;
        sh_ratio = ratio;
    }
    __syncthreads();
    const int it = mode == 0 ? 0 : *iter;       // mode 2: advanced by this iteration's G step
    if (sh_status) {        // breakdown: the record, the freeze, the host's word; X stays the last complete iterate
        if (tid == 0) {
            bd.rec[0] = sh_status;
            bd.rec[1] = mode == 1 ? it + 1 : it;
            bd.rec[2] = 1;
            *bd.min_ratio = sh_ratio;
            if (mode == 0) *iter = 0;
            if (has_stop) *g.nactive = 0;
        }
        // a history row for the iteration that was counted: the squared norms themselves at set_rhs, else the row before
        if (mode != 1 && tid < S && it < hist_cap)
            history[(long long)it * S + tid] = mode == 0 ? (T)C[tid * kBlockLd + tid] : history[(long long)(it - 1) * S + tid];
        return;
    }
    if (tid < S) small_linv_column(L, X, S, tid);
    __syncthreads();
    const int i = tid / S, j = tid - (tid / S) * S;
    if (mode == 1) {
        if (tid < S * S) {  // alpha = L^-T L^-1
            const int m0 = i > j ? i : j;
            double acc = X[m0 * kBlockLd + i] * X[m0 * kBlockLd + j];
            for (int m = m0 + 1; m < S; ++m) acc = acc + X[m * kBlockLd + i] * X[m * kBlockLd + j];
            A2[i * kBlockLd + j] = acc;
            bd.alpha[tid] = acc;
            static_cast<T *>(bd.alpha_T)[tid] = (T)acc;
        }
        __syncthreads();
        if (tid < S * S) {  // M = alpha xi (xi upper triangular)
            double acc = A2[i * kBlockLd] * XI[j];
            for (int m = 1; m <= j; ++m) acc = acc + A2[i * kBlockLd + m] * XI[m * kBlockLd + j];
            bd.M[tid] = acc;
            static_cast<T *>(bd.M_T)[tid] = (T)acc;
        }
        if (tid == 0) {
            *iter = it + 1;
            *bd.min_ratio = sh_ratio;
        }
        return;
    }
    // tau = L^T, tau^-1 = X^T, xi <- tau xi
    if (tid < S * S) {
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
        A2[i * kBlockLd + j] = acc;
        bd.xi[tid] = acc;
    }
    __syncthreads();
    int done = 1;
    if (tid < S) {          // delta_k[tid] = |xi e_tid|^2, the history, this column's side of the stop
        double acc = A2[tid] * A2[tid];
        for (int m = 1; m <= tid; ++m) acc = acc + A2[m * kBlockLd + tid] * A2[m * kBlockLd + tid];
        const T dT = (T)acc;
        if (it < hist_cap) history[(long long)it * S + tid] = dT;
        done = has_stop && mode == 2 ? !(stop_norm(dT) >= g.tol[tid]) : 0;
    }
    const int all = __syncthreads_and(done);
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
static int block_gram_impl(int n, long long ld, int S, const void *a, const void *b, double *part, int grid, const int *frozen, hipStream_t st) {
#define CG_BG(N) hipLaunchKernelGGL((block_gram_kernel<T, N>), dim3(grid), dim3(kBlock), 0, st, n, ld, (const T *)a, (const T *)b, part, frozen)
    CG_BLOCK_S(S, CG_BG)
#undef CG_BG
    return check_launch("block gram");
}
template <typename T>
static int block_xw_impl(int n, long long ld, int S, const void *P, const void *AP, void *X, void *Q, const void *M, const void *AL, double *part,
                         int grid, const int *frozen, hipStream_t st) {
#define CG_BX(N) hipLaunchKernelGGL((block_xw_kernel<T, N>), dim3(grid), dim3(kBlock), 0, st, n, ld, (const T *)P, (const T *)AP, (T *)X, (T *)Q, \
                                    (const T *)M, (const T *)AL, part, frozen)
    CG_BLOCK_S(S, CG_BX)
#undef CG_BX
    return check_launch("block update x, w");
}
template <typename T>
static int block_qp_impl(int n, long long ld, int S, void *Q, void *P, const void *TI, const void *TA, int init, int grid, const int *frozen,
                         hipStream_t st) {
#define CG_BQ(N) hipLaunchKernelGGL((block_qp_kernel<T, N>), dim3(grid), dim3(kBlock), 0, st, n, ld, (T *)Q, (T *)P, (const T *)TI, (const T *)TA, init, frozen)
    CG_BLOCK_S(S, CG_BQ)
#undef CG_BQ
    return check_launch("block update q, p");
}
template <typename T>
static int block_small_impl(int mode, int S, int grid, const double *part, const BlockDev &bd, const CgScalars &sc, const CgStop *stop, hipStream_t st) {
    const CgStop none;
    hipLaunchKernelGGL((block_small_kernel<T>), dim3(1), dim3(kScalarBlock), 0, st, mode, S, grid, part, bd, sc.iter, (T *)sc.history, sc.history_cap,
                       stop ? *stop : none, stop ? 1 : 0);
    return check_launch("block small step");
}

int launch_block_gram(int dtype, int n, long long ld, int S, const void *a, const void *b, double *part, int grid, const int *frozen, hipStream_t st) {
    CG_BLOCK_REAL(dtype, block_gram_impl, n, ld, S, a, b, part, grid, frozen, st);
}
int launch_block_xw(int dtype, int n, long long ld, int S, const void *P, const void *AP, void *X, void *Q, const void *M, const void *AL, double *part,
                    int grid, const int *frozen, hipStream_t st) {
    CG_BLOCK_REAL(dtype, block_xw_impl, n, ld, S, P, AP, X, Q, M, AL, part, grid, frozen, st);
}
int launch_block_qp(int dtype, int n, long long ld, int S, void *Q, void *P, const void *TI, const void *TA, bool init, const int *frozen, hipStream_t st) {
    CG_BLOCK_REAL(dtype, block_qp_impl, n, ld, S, Q, P, TI, TA, init ? 1 : 0, block_gram_grid(n), frozen, st);
}
int launch_block_small(int dtype, int mode, const BlockState &b, const CgScalars &sc, const CgStop *stop, hipStream_t st) {
    CG_BLOCK_REAL(dtype, block_small_impl, mode, b.S, b.grid, b.dev.partials, b.dev, sc, stop, st);
}

// one allocation: the record (status, event, frozen, pad; the smallest pivot ratio), seven s x s matrices in double (xi, G, alpha, tau,
// W^T W, tau^-1, M), four in the value type (M, alpha, tau^-1, tau) and the Gram partials of a system of n rows
int block_alloc(BlockState *b, int S, long long n) {
    const int grid = block_gram_grid(n);
    const size_t mat = (size_t)kBlockMax * kBlockMax * sizeof(double), np = (size_t)S * (S + 1) / 2;
    void *mem = nullptr;
    if (int rc = dmalloc(&mem, 32 + 11 * mat + np * grid * sizeof(double), "block CG state")) return rc;
    char *p = static_cast<char *>(mem);
    BlockDev &d = b->dev;
    d.rec = reinterpret_cast<int *>(p);
    d.min_ratio = reinterpret_cast<double *>(p + 16);
    double **dm[] = {&d.xi, &d.G, &d.alpha, &d.tau, &d.C, &d.tau_inv, &d.M};
    p += 32;
    for (double **m : dm) { *m = reinterpret_cast<double *>(p); p += mat; }
    void **tm[] = {&d.M_T, &d.alpha_T, &d.tinv_T, &d.tau_T};
    for (void **m : tm) { *m = p; p += mat; }
    d.partials = reinterpret_cast<double *>(p);
    b->mem = mem;
    b->S = S;
    b->grid = grid;
    return CGAMD_OK;
}
void block_free(BlockState *b) {
    if (b->mem) (void)hipFree(b->mem);
    if (b->mem_pcg) (void)hipFree(b->mem_pcg);
    *b = BlockState();
}

}  // namespace cgamd

// ---- context-level entries (development: the kernel test) -----------------------------------------------------------------------------
using namespace cgamd;

static int block_entry(cgamd_ctx *ctx, const char *who, int dtype, int size, long long ld, int s) {
    const std::string w = who;
    if (!ctx) return fail(CGAMD_ERR_INVALID, w + ": context is NULL");
    if (dtype != CGAMD_F32 && dtype != CGAMD_F64) return fail(CGAMD_ERR_INVALID, w + ": block CG serves the real value types");
    if (size < 1 || ld < size) return fail(CGAMD_ERR_INVALID, w + ": size >= 1 and ld >= size are required");
    if (s < 2 || s > kBlockMax) return fail(CGAMD_ERR_INVALID, w + ": the block size runs 2 ... 16");
    thread_hip_setup();
    CG_HIP(hipSetDevice(ctx->device));
    return stream_not_capturing(ctx->stream, who);
}

extern "C" int cgamd_block_gram_grid(int size) { return size < 1 ? -fail(CGAMD_ERR_INVALID, "block_gram_grid: size >= 1 is required") : block_gram_grid(size); }

extern "C" int cgamd_block_gram(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, const void *a, const void *b, void *partials) {
    if (int rc = block_entry(ctx, "block_gram", dtype, size, ld, s)) return rc;
    if (!a || !b || !partials) return fail(CGAMD_ERR_INVALID, "block_gram: null pointer");
    return launch_block_gram(dtype, size, ld, s, a, b, static_cast<double *>(partials), block_gram_grid(size), nullptr, ctx->stream);
}

extern "C" int cgamd_block_update_xw(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, const void *p, const void *ap, void *x, void *q,
                                     const void *m, const void *alpha, void *partials) {
    if (int rc = block_entry(ctx, "block_update_xw", dtype, size, ld, s)) return rc;
    if (!p || !ap || !x || !q || !m || !alpha || !partials) return fail(CGAMD_ERR_INVALID, "block_update_xw: null pointer");
    return launch_block_xw(dtype, size, ld, s, p, ap, x, q, m, alpha, static_cast<double *>(partials), block_gram_grid(size), nullptr, ctx->stream);
}

extern "C" int cgamd_block_update_qp(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, void *q, void *p, const void *tau_inv, const void *tau,
                                     int init) {
    if (int rc = block_entry(ctx, "block_update_qp", dtype, size, ld, s)) return rc;
    if (!q || !p || !tau_inv || !tau) return fail(CGAMD_ERR_INVALID, "block_update_qp: null pointer");
    return launch_block_qp(dtype, size, ld, s, q, p, tau_inv, tau, init != 0, nullptr, ctx->stream);
}
