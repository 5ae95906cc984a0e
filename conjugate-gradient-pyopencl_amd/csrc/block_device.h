// What the vector kernels of block CG (block_cg.hip) and of its preconditioned form (block_pcg.hip) share: the Gram accumulation and
// its work-group sum, the barrier that keeps the small factors in LDS, and the dispatch on the block size and the value type.
#pragma once
#include "cgamd_internal.h"
#include "device_types.h"
#include "reduce_device.h"

namespace cgamd {

constexpr int kBlockLd = kBlockMax + 1; // row pitch of the small matrices in LDS

// The factors in LDS are the same for every row, and the compiler would lift all 2 s^2 of them out of the row loop into registers
// (s = 16 in double: 1024 of them, spilled to scratch).  A compiler-level memory barrier at the head of the loop body keeps them
// where they are: broadcast reads of LDS, row after row.  No instruction is emitted
CG_DEV void lds_stays() { asm volatile("" ::: "memory"); }

// the block_sum<256> of NP values per thread: the wave trees, then thread p adds entry p's four wave sums in order.  sm: NP x 4
template <int NP> CG_DEV void gram_store(const double (&acc)[NP], double *sm, double *__restrict__ part) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const double v = wave_sum(acc[p]);
        if (lane == 0) sm[p * 4 + w] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < NP) {
        double v = sm[threadIdx.x * 4];
        for (int i = 1; i < kBlock / kWave; ++i) v = v + sm[threadIdx.x * 4 + i];
        part[(long long)threadIdx.x * gridDim.x + blockIdx.x] = v;
    }
}
template <typename T, int S> CG_DEV void gram_add(const T (&a)[S], const T (&b)[S], double (&acc)[S * (S + 1) / 2]) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const double bj = (double)b[j];
#pragma unroll
        for (int i = 0; i <= j; ++i) acc[j * (j + 1) / 2 + i] = acc[j * (j + 1) / 2 + i] + (double)a[i] * bj;
    }
}

// ---- what the small steps (one work-group, double) of both files share; matrices in LDS at pitch kBlockLd ------------------------------
// entry e of a symmetric matrix from its partials [entries][grid], by ONE wave (all its lanes call): lane-strided, then the wave
// tree; lane 0 stores it on both sides of the diagonal
CG_DEV void small_sum_entry(const double *__restrict__ part, int grid, int e, int lane, double *C) {
    double acc = 0.;
    for (int k = lane; k < grid; k += kWave) acc = acc + part[(long long)e * grid + k];
    acc = wave_sum(acc);
    if (lane == 0) {
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= e) ++j;
        const int i = e - j * (j + 1) / 2;
        C[i * kBlockLd + j] = acc;
        C[j * kBlockLd + i] = acc;
    }
}
// C = L L^T by ONE thread, left-looking by columns, with the pivot rule not v > s eps max_j C_jj.  Returns 0, `failed` (a pivot
// failed the rule) or 3 (NaN); ratio: in, the smallest pivot ratio so far; out, with this factorisation's
CG_DEV int small_cholesky(const double *C, double *L, int S, double eps, int failed, double &ratio) {
    int status = 0;
    double maxd = C[0];
    for (int k = 1; k < S; ++k) maxd = C[k * kBlockLd + k] > maxd ? C[k * kBlockLd + k] : maxd;
    for (int k = 0; k < S; ++k)
        if (C[k * kBlockLd + k] != C[k * kBlockLd + k]) status = 3;
    const double thr = (double)S * eps * maxd;
    for (int k = 0; k < S && !status; ++k) {
        double v = C[k * kBlockLd + k];
        for (int m = 0; m < k; ++m) v = v - L[k * kBlockLd + m] * L[k * kBlockLd + m];
        if (v != v) { status = 3; break; }
        const double rk = v / maxd;
        if (rk < ratio) ratio = rk;
        if (!(v > thr)) { status = failed; break; }
        const double d = sqrt(v);
        L[k * kBlockLd + k] = d;
        for (int i = k + 1; i < S; ++i) {
            double w = C[i * kBlockLd + k];
            for (int m = 0; m < k; ++m) w = w - L[i * kBlockLd + m] * L[k * kBlockLd + m];
            L[i * kBlockLd + k] = w / d;
        }
    }
    return status;
}
// column j of X = L^-1, by one thread per column
CG_DEV void small_linv_column(const double *L, double *X, int S, int j) {
    X[j * kBlockLd + j] = 1. / L[j * kBlockLd + j];
    for (int i = j + 1; i < S; ++i) {
        double acc = L[i * kBlockLd + j] * X[j * kBlockLd + j];
        for (int m = j + 1; m < i; ++m) acc = acc + L[i * kBlockLd + m] * X[m * kBlockLd + j];
        X[i * kBlockLd + j] = -acc / L[i * kBlockLd + i];
    }
    for (int i = 0; i < j; ++i) X[i * kBlockLd + j] = 0.;
}

}  // namespace cgamd

#define CG_BLOCK_S(S, CALL)                                                                            \
    switch (S) {                                                                                        \
    case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break;     \
    case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; case 9: CALL(9); break;     \
    case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; case 13: CALL(13); break; \
    case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break;                       \
    default: return fail(CGAMD_ERR_INVALID, "block CG: the block size runs 2 ... 16");                  \
    }
#define CG_BLOCK_REAL(dtype, FN, ...)                                                       \
    switch (dtype) {                                                                        \
    case CGAMD_F32: return FN<float>(__VA_ARGS__);                                          \
    case CGAMD_F64: return FN<double>(__VA_ARGS__);                                         \
    default: return fail(CGAMD_ERR_INVALID, "block CG serves the real value types");        \
    }
