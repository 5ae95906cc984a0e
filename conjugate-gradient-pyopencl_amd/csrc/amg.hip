// Algebraic aggregation multigrid (cgamd_solver_set_preconditioner_amg): the device side of what the grid entry does by index
// arithmetic, here through stored maps.
//   aggregates  deterministic handshake matching, one pass at a time (include/cgamd.h states it): the row maximum of the strength
//               s_ij = -Re(b_ij); rounds of two launches, `pick` (reads the matching as it stood when the round began, writes pick[i]
//               alone) and `handshake` (reads pick, writes match[i] alone) -- no result depends on the order threads run in; the roots
//               (smallest members) flagged, scanned by mg_scan_kernel and numbered; the pass map composed into the level's map and
//               the sorted member lists merged, ONE THREAD PER AGGREGATE.  Member lists: kAmgWidth ints per aggregate, fine rows
//               ascending, -1 behind the last.
//   Galerkin    count and fill as in multigrid.hip (same sums, same orders, the same 64-column list), the rows of an aggregate from a
//               member list and the coarse column from a map.
//   V-cycle     restriction (fused with the residual and the coarse level's first smoothing step) through the member lists,
//               prolongation (fused with the correction) through the map: one thread's own fixed sequence per output element, no
//               atomics, no reductions, grid.y = right-hand side.
// Everything is stream-ordered on the caller's stream.
#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"

namespace cgamd {

CG_DEV double amg_strength(float v) { return -(double)v; }
CG_DEV double amg_strength(double v) { return -v; }
CG_DEV double amg_strength(float2 v) { return -(double)v.x; }
CG_DEV double amg_strength(double2 v) { return -v.x; }

// the symmetric 32-bit tie-break hash of a pair of rows
CG_DEV unsigned amg_hash(int i, int j) {
    const unsigned lo = (unsigned)(i < j ? i : j), hi = (unsigned)(i < j ? j : i);
    unsigned h = (lo * 0x9E3779B1u) ^ hi;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// smax[i] = the largest s_ij > 0 over the stored entries j != i of row i, 0 without one (a NaN compares above nothing)
template <typename T>
__global__ __launch_bounds__(kBlock) void amg_smax_kernel(int n, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                          const int *__restrict__ cols, double *__restrict__ smax) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double m = 0.;
    const int end = ptr[i + 1];
    for (int k = ptr[i]; k < end; ++k) {
        if (cols[k] == i) continue;
        const double s = amg_strength(vals[k]);
        if (s > m) m = s;
    }
    smax[i] = m;
}

// pick[i] of every unmatched row: among its strong entries with an unmatched column, larger s, then larger hash, then smaller column
template <typename T>
__global__ __launch_bounds__(kBlock) void amg_pick_kernel(int n, double theta, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                          const int *__restrict__ cols, const double *__restrict__ smax,
                                                          const int *__restrict__ match, int *__restrict__ pick) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int best = -1;
    if (match[i] < 0) {
        const double bound = theta * smax[i];
        double bs = 0.;
        unsigned bh = 0;
        const int end = ptr[i + 1];
        for (int k = ptr[i]; k < end; ++k) {
            const int j = cols[k];
            if (j == i || j < 0 || j >= n) continue;
            const double s = amg_strength(vals[k]);
            if (!(s > 0.) || !(s >= bound) || match[j] >= 0) continue;
            const unsigned h = amg_hash(i, j);
            if (best < 0 || s > bs || (s == bs && (h > bh || (h == bh && j < best)))) { best = j; bs = s; bh = h; }
        }
    }
    pick[i] = best;
}

// i and j are matched when each picked the other; *formed <- 1 when the round made a pair
__global__ __launch_bounds__(kBlock) void amg_handshake_kernel(int n, const int *__restrict__ pick, int *__restrict__ match,
                                                               int *__restrict__ formed) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = pick[i];
    if (j < 0 || pick[j] != i) return;
    match[i] = j;
    if (i < j) *formed = 1;
}

// flag[i] = 1 for the root (smallest member) of every aggregate of the pass
__global__ __launch_bounds__(kBlock) void amg_roots_kernel(int n, const int *__restrict__ match, int *__restrict__ flag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = match[i];
    flag[i] = (j < 0 || j > i) ? 1 : 0;
}

// rank = the scanned root flags: pmap[i] = the rank of i's root; pairs[2 I], pairs[2 I + 1] = the root of aggregate I and its partner (-1)
__global__ __launch_bounds__(kBlock) void amg_number_kernel(int n, const int *__restrict__ match, const int *__restrict__ rank,
                                                            int *__restrict__ pmap, int *__restrict__ pairs) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = match[i];
    if (j < 0 || j > i) {
        const int I = rank[i];
        pmap[i] = I;
        pairs[2 * (long long)I] = i;
        pairs[2 * (long long)I + 1] = j;
    } else pmap[i] = rank[j];
}

// the level's map after one more pass: agg_out[i] = pmap[agg_in[i]] (agg_in == nullptr: the pass map itself; agg_in == agg_out serves)
__global__ __launch_bounds__(kBlock) void amg_compose_kernel(int n, const int *__restrict__ pmap, const int *agg_in, int *agg_out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    agg_out[i] = pmap[agg_in ? agg_in[i] : i];
}

// the member lists after one more pass: the sorted lists of the pair's two members merged (old == nullptr: the members are fine rows)
__global__ __launch_bounds__(kBlock) void amg_members_kernel(int nc, const int *__restrict__ pairs, const int *__restrict__ old,
                                                             int *__restrict__ out) {
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    const int a = pairs[2 * (long long)I], b = pairs[2 * (long long)I + 1];
    int la[kAmgWidth], lb[kAmgWidth], na = 0, nb = 0;
    if (!old) {
        la[na++] = a;
        if (b >= 0) lb[nb++] = b;
    } else {
        for (int k = 0; k < kAmgWidth; ++k) {
            const int m = old[(long long)a * kAmgWidth + k];
            if (m < 0) break;
            la[na++] = m;
        }
        if (b >= 0)
            for (int k = 0; k < kAmgWidth; ++k) {
                const int m = old[(long long)b * kAmgWidth + k];
                if (m < 0) break;
                lb[nb++] = m;
            }
    }
    int pa = 0, pb = 0;
    for (int k = 0; k < kAmgWidth; ++k) {
        int m = -1;
        if (pa < na && (pb >= nb || la[pa] < lb[pb])) m = la[pa++];
        else if (pb < nb) m = lb[pb++];
        out[(long long)I * kAmgWidth + k] = m;
    }
}

// ---- Galerkin through a member list (width ints per coarse row, -1 behind the last) and a column map ------------------------------
CG_DEV int amg_collect(int I, int width, const int *__restrict__ mem, const int *__restrict__ agg, const int *__restrict__ ptr,
                       const int *__restrict__ cols, int *list) {
    int cnt = 0;
    for (int m = 0; m < width; ++m) {
        const int i = mem[(long long)I * width + m];
        if (i < 0) break;
        const int end = ptr[i + 1];
        for (int j = ptr[i]; j < end; ++j) {
            const int J = agg[cols[j]];
            int p = 0;
            while (p < cnt && list[p] < J) ++p;
            if (p < cnt && list[p] == J) continue;
            if (cnt == kMgMaxRow) return -1;
            for (int q = cnt; q > p; --q) list[q] = list[q - 1];
            list[p] = J;
            ++cnt;
        }
    }
    return cnt;
}

__global__ __launch_bounds__(kBlock) void amg_count_kernel(int nc, int width, const int *__restrict__ mem, const int *__restrict__ agg,
                                                           const int *__restrict__ ptr, const int *__restrict__ cols,
                                                           int *__restrict__ count, unsigned long long *__restrict__ err) {
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    int list[kMgMaxRow];
    int cnt = amg_collect(I, width, mem, agg, ptr, cols, list);
    if (cnt < 0) {
        atomicMin(err, (unsigned long long)I);
        cnt = 0;
    }
    count[I] = cnt;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void amg_fill_kernel(int nc, int width, const int *__restrict__ mem, const int *__restrict__ agg,
                                                          const T *__restrict__ vals, const int *__restrict__ ptr,
                                                          const int *__restrict__ cols, const int *__restrict__ ptrc,
                                                          int *__restrict__ colsc, T *__restrict__ valsc) {
    using A = typename VT<T>::acc;
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    int list[kMgMaxRow];
    A acc[kMgMaxRow];
    const int cnt = amg_collect(I, width, mem, agg, ptr, cols, list);
    if (cnt < 0) return;        // (refused by the count pass)
    for (int p = 0; p < cnt; ++p) acc[p] = vzero<A>();
    for (int m = 0; m < width; ++m) {
        const int i = mem[(long long)I * width + m];
        if (i < 0) break;
        const int end = ptr[i + 1];
        for (int j = ptr[i]; j < end; ++j) {
            const int J = agg[cols[j]];
            int p = 0;
            while (p < cnt - 1 && list[p] < J) ++p;
            acc[p] = vadd(acc[p], to_acc(vals[j]));
        }
    }
    const int base = ptrc[I];
    if (ptrc[I + 1] - base != cnt) return;      // (the scan clamped: refused by the caller)
    for (int p = 0; p < cnt; ++p) {
        colsc[base + p] = list[p];
        valsc[base + p] = from_acc<T>(acc[p]);
    }
}

// ---- V-cycle ---------------------------------------------------------------------------------------------------------------------
CG_DEV float amg_scale(float c, float v) { return c * v; }
CG_DEV double amg_scale(double c, double v) { return c * v; }
CG_DEV float2 amg_scale(float c, float2 v) { return make_float2(c * v.x, c * v.y); }
CG_DEV double2 amg_scale(double c, double2 v) { return make_double2(c * v.x, c * v.y); }

// bc[I] = sum over the members of aggregate I, ascending, of (b - w)[i]; then the coarse level's first smoothing step from zero:
// xc = dc = c1 dinvc bc
template <typename T>
__global__ __launch_bounds__(kBlock) void amg_restrict_kernel(int nc, const int *__restrict__ mem, long long ldf, long long ldc,
                                                              const T *__restrict__ b, const T *__restrict__ w, T *__restrict__ bc,
                                                              const T *__restrict__ dinvc, T *__restrict__ xc, T *__restrict__ dc,
                                                              typename VT<T>::real c1, int store_d) {
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    const long long of = (long long)blockIdx.y * ldf, oc = (long long)blockIdx.y * ldc + I;
    int m[kAmgWidth];
    const int4 *row = reinterpret_cast<const int4 *>(mem + (long long)I * kAmgWidth);
    const int4 m0 = row[0], m1 = row[1];
    m[0] = m0.x; m[1] = m0.y; m[2] = m0.z; m[3] = m0.w; m[4] = m1.x; m[5] = m1.y; m[6] = m1.z; m[7] = m1.w;
    T s = vzero<T>();
#pragma unroll
    for (int k = 0; k < kAmgWidth; ++k)
        if (m[k] >= 0) s = vadd(s, vsub(b[of + m[k]], w[of + m[k]]));
    bc[oc] = s;
    const T dn = amg_scale(c1, vmul(dinvc[I], s));
    xc[oc] = dn;
    if (store_d) dc[oc] = dn;
}

// x[i] += omega e[agg[i]] for the nf rows of the fine level
template <typename T>
__global__ __launch_bounds__(kBlock) void amg_prolong_kernel(int nf, const int *__restrict__ agg, long long ldf, long long ldc,
                                                             const T *__restrict__ e, T *__restrict__ x, typename VT<T>::real omega) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const long long of = (long long)blockIdx.y * ldf + i, oc = (long long)blockIdx.y * ldc + agg[i];
    x[of] = vadd(x[of], amg_scale(omega, e[oc]));
}

static dim3 amg_rows_grid(int n, int nrhs = 1) { return dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)nrhs); }

template <typename T>
static int amg_smax_impl(int n, const void *vals, const int *ptr, const int *cols, double *smax, hipStream_t st) {
    hipLaunchKernelGGL((amg_smax_kernel<T>), amg_rows_grid(n), dim3(kBlock), 0, st, n, (const T *)vals, ptr, cols, smax);
    return check_launch("amg_smax");
}
int launch_amg_smax(int dtype, int n, const void *vals, const int *ptr, const int *cols, double *smax, hipStream_t st) {
    CG_DISPATCH(dtype, amg_smax_impl, n, vals, ptr, cols, smax, st);
}
template <typename T>
static int amg_pick_impl(int n, double theta, const void *vals, const int *ptr, const int *cols, const double *smax, const int *match,
                         int *pick, hipStream_t st) {
    hipLaunchKernelGGL((amg_pick_kernel<T>), amg_rows_grid(n), dim3(kBlock), 0, st, n, theta, (const T *)vals, ptr, cols, smax, match, pick);
    return check_launch("amg_pick");
}
int launch_amg_pick(int dtype, int n, double theta, const void *vals, const int *ptr, const int *cols, const double *smax, const int *match,
                    int *pick, hipStream_t st) {
    CG_DISPATCH(dtype, amg_pick_impl, n, theta, vals, ptr, cols, smax, match, pick, st);
}
int launch_amg_handshake(int n, const int *pick, int *match, int *formed, hipStream_t st) {
    hipLaunchKernelGGL(amg_handshake_kernel, amg_rows_grid(n), dim3(kBlock), 0, st, n, pick, match, formed);
    return check_launch("amg_handshake");
}
int launch_amg_roots(int n, const int *match, int *flag, hipStream_t st) {
    hipLaunchKernelGGL(amg_roots_kernel, amg_rows_grid(n), dim3(kBlock), 0, st, n, match, flag);
    return check_launch("amg_roots");
}
int launch_amg_number(int n, const int *match, const int *rank, int *pmap, int *pairs, hipStream_t st) {
    hipLaunchKernelGGL(amg_number_kernel, amg_rows_grid(n), dim3(kBlock), 0, st, n, match, rank, pmap, pairs);
    return check_launch("amg_number");
}
int launch_amg_compose(int n, const int *pmap, const int *agg_in, int *agg_out, hipStream_t st) {
    hipLaunchKernelGGL(amg_compose_kernel, amg_rows_grid(n), dim3(kBlock), 0, st, n, pmap, agg_in, agg_out);
    return check_launch("amg_compose");
}
int launch_amg_members(int nc, const int *pairs, const int *old, int *out, hipStream_t st) {
    hipLaunchKernelGGL(amg_members_kernel, amg_rows_grid(nc), dim3(kBlock), 0, st, nc, pairs, old, out);
    return check_launch("amg_members");
}
int launch_amg_count(int nc, int width, const int *mem, const int *agg, const int *ptr, const int *cols, int *count, unsigned long long *err,
                     hipStream_t st) {
    hipLaunchKernelGGL(amg_count_kernel, amg_rows_grid(nc), dim3(kBlock), 0, st, nc, width, mem, agg, ptr, cols, count, err);
    return check_launch("amg_count");
}
template <typename T>
static int amg_fill_impl(int nc, int width, const int *mem, const int *agg, const void *vals, const int *ptr, const int *cols, const int *ptrc,
                         int *colsc, void *valsc, hipStream_t st) {
    hipLaunchKernelGGL((amg_fill_kernel<T>), amg_rows_grid(nc), dim3(kBlock), 0, st, nc, width, mem, agg, (const T *)vals, ptr, cols, ptrc, colsc,
                       (T *)valsc);
    return check_launch("amg_fill");
}
int launch_amg_fill(int dtype, int nc, int width, const int *mem, const int *agg, const void *vals, const int *ptr, const int *cols,
                    const int *ptrc, int *colsc, void *valsc, hipStream_t st) {
    CG_DISPATCH(dtype, amg_fill_impl, nc, width, mem, agg, vals, ptr, cols, ptrc, colsc, valsc, st);
}
template <typename T>
static int amg_restrict_impl(int nc, const int *mem, long long ldf, long long ldc, int nrhs, const void *b, const void *w, void *bc,
                             const void *dinvc, void *xc, void *dc, double c1, bool store_d, hipStream_t st) {
    using R = typename VT<T>::real;
    hipLaunchKernelGGL((amg_restrict_kernel<T>), amg_rows_grid(nc, nrhs), dim3(kBlock), 0, st, nc, mem, ldf, ldc, (const T *)b, (const T *)w,
                       (T *)bc, (const T *)dinvc, (T *)xc, (T *)dc, (R)c1, store_d ? 1 : 0);
    return check_launch("amg_restrict");
}
int launch_amg_restrict(int dtype, int nc, const int *mem, long long ldf, long long ldc, int nrhs, const void *b, const void *w, void *bc,
                        const void *dinvc, void *xc, void *dc, double c1, bool store_d, hipStream_t st) {
    if (store_d && !dc) return fail(CGAMD_ERR_INVALID, "amg_restrict: the coarse level needs its d vector");
    CG_DISPATCH(dtype, amg_restrict_impl, nc, mem, ldf, ldc, nrhs, b, w, bc, dinvc, xc, dc, c1, store_d, st);
}
template <typename T>
static int amg_prolong_impl(int nf, const int *agg, long long ldf, long long ldc, int nrhs, const void *e, void *x, double omega, hipStream_t st) {
    using R = typename VT<T>::real;
    hipLaunchKernelGGL((amg_prolong_kernel<T>), amg_rows_grid(nf, nrhs), dim3(kBlock), 0, st, nf, agg, ldf, ldc, (const T *)e, (T *)x, (R)omega);
    return check_launch("amg_prolong");
}
int launch_amg_prolong(int dtype, int nf, const int *agg, long long ldf, long long ldc, int nrhs, const void *e, void *x, double omega,
                       hipStream_t st) {
    CG_DISPATCH(dtype, amg_prolong_impl, nf, agg, ldf, ldc, nrhs, e, x, omega, st);
}

}  // namespace cgamd
