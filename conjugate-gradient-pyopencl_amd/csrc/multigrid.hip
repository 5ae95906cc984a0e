// Aggregation multigrid preconditioner on grid systems (cgamd_solver_set_preconditioner_multigrid): the device side.
//   setup     Galerkin coarse matrices A_c = P^T A P with piecewise-constant P over 2 x 2 x 2 boxes of a grid numbered x fastest, in
//             two passes: ONE THREAD PER COARSE ROW collects the distinct coarse columns of its <= 8 fine rows in a small sorted
//             list (count), one work-group scans the counts into row pointers, and the second pass collects the list again and adds
//             every fine entry to its slot -- fine rows ascending, entries in stored order, in double / complex double, rounded
//             once.  Structural zeros are kept, so the pattern depends on the pattern alone.  The Gershgorin bound of D^-1 A is one
//             more pass (a maximum: order-free, so one atomicMax per work-group on the bits of a non-negative double).
//   V-cycle   three element-wise kernels, grid.y = right-hand side: the Chebyshev update, the restriction fused with the residual
//             (and with the first smoothing step of the coarse level, which starts from zero and needs no product), the
//             prolongation fused with the correction.  No reductions: every output element is one thread's own sequence of
//             operations, so the bits do not depend on the launch geometry.
// Everything is stream-ordered on the caller's stream.
#include <algorithm>

#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"

namespace cgamd {

CG_DEV int mg_agg(int i, const MgGrid &g) {
    const int x = i % g.nx, t = i / g.nx, y = t % g.ny, z = t / g.ny;
    return (x >> 1) + g.cnx * ((y >> 1) + g.cny * (z >> 1));
}

// the sorted list of the distinct coarse columns of coarse row I; -1 when there are more than kMgMaxRow
CG_DEV int mg_collect(int I, const MgGrid &g, const int *__restrict__ ptr, const int *__restrict__ cols, int *list) {
    const int X = I % g.cnx, t = I / g.cnx, Y = t % g.cny, Z = t / g.cny;
    int cnt = 0;
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * X + dx, y = 2 * Y + dy, z = 2 * Z + dz;
                if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
                const int i = x + g.nx * (y + g.ny * z), end = ptr[i + 1];
                for (int j = ptr[i]; j < end; ++j) {
                    const int J = mg_agg(cols[j], g);
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

__global__ __launch_bounds__(kBlock) void mg_count_kernel(MgGrid g, int nc, const int *__restrict__ ptr, const int *__restrict__ cols,
                                                          int *__restrict__ count, unsigned long long *__restrict__ err) {
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    int list[kMgMaxRow];
    int cnt = mg_collect(I, g, ptr, cols, list);
    if (cnt < 0) {
        atomicMin(err, (unsigned long long)I);
        cnt = 0;
    }
    count[I] = cnt;
}

// a[0 .. n - 1] counts -> exclusive prefix sums in place, a[n] = the total; *overflow = 1 when the total does not fit an int.  One
// work-group: every thread sums a contiguous chunk, thread 0 scans the 1024 chunk sums, every thread writes its chunk's prefixes
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void mg_scan_kernel(int n, int *__restrict__ a, int *__restrict__ overflow) {
    __shared__ long long sums[kScanBlock];
    const int t = threadIdx.x;
    const long long chunk = ((long long)n + kScanBlock - 1) / kScanBlock;
    const long long lo = std::min((long long)n, t * chunk), hi = std::min((long long)n, lo + chunk);
    long long s = 0;
    for (long long i = lo; i < hi; ++i) s += a[i];
    sums[t] = s;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int k = 0; k < kScanBlock; ++k) {
            const long long v = sums[k];
            sums[k] = run;
            run += v;
        }
        if (run > 2147483647LL) { *overflow = 1; run = 2147483647LL; }
        a[n] = (int)run;
    }
    __syncthreads();
    long long run = sums[t];
    for (long long i = lo; i < hi; ++i) {
        const int c = a[i];
        a[i] = (int)std::min(run, 2147483647LL);
        run += c;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mg_fill_kernel(MgGrid g, int nc, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                         const int *__restrict__ cols, const int *__restrict__ ptrc,
                                                         int *__restrict__ colsc, T *__restrict__ valsc) {
    using A = typename VT<T>::acc;
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    int list[kMgMaxRow];
    A acc[kMgMaxRow];
    const int cnt = mg_collect(I, g, ptr, cols, list);
    if (cnt < 0) return;        // (refused by the count pass)
    for (int p = 0; p < cnt; ++p) acc[p] = vzero<A>();
    const int X = I % g.cnx, t = I / g.cnx, Y = t % g.cny, Z = t / g.cny;
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * X + dx, y = 2 * Y + dy, z = 2 * Z + dz;
                if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
                const int i = x + g.nx * (y + g.ny * z), end = ptr[i + 1];
                for (int j = ptr[i]; j < end; ++j) {
                    const int J = mg_agg(cols[j], g);
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

CG_DEV double mg_abs(float v) { return fabs((double)v); }
CG_DEV double mg_abs(double v) { return fabs(v); }
CG_DEV double mg_abs(float2 v) { return hypot((double)v.x, (double)v.y); }
CG_DEV double mg_abs(double2 v) { return hypot(v.x, v.y); }

// *out (preset to 0) <- max_i |dinv_i| sum_j |a_ij| in double, as the bits of a non-negative double (a NaN compares above everything)
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_gershgorin_kernel(int n, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                               const T *__restrict__ dinv, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sm[kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double v = 0.;
    if (i < n) {
        double s = 0.;
        const int end = ptr[i + 1];
        for (int j = ptr[i]; j < end; ++j) s += mg_abs(vals[j]);
        v = mg_abs(dinv[i]) * s;
    }
    sm[threadIdx.x] = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] = std::max(sm[threadIdx.x], sm[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, sm[0]);
}

// ---- V-cycle ---------------------------------------------------------------------------------------------------------------------
CG_DEV float mg_scale(float c, float v) { return c * v; }
CG_DEV double mg_scale(double c, double v) { return c * v; }
CG_DEV float2 mg_scale(float c, float2 v) { return make_float2(c * v.x, c * v.y); }
CG_DEV double2 mg_scale(double c, double2 v) { return make_double2(c * v.x, c * v.y); }

// One Chebyshev step.  MODE 0: x = 0 on entry, d = c1 dinv b, x = d (no product).  MODE 1: the first step from an x that is not
// zero, d = c1 dinv (b - w), x += d.  MODE 2: a later step, d = c0 d + c1 dinv (b - w), x += d.  w = A x.  d is stored when a later
// step reads it.  dinv is shared by the right-hand sides
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void mg_cheb_kernel(int n, long long ld, const T *__restrict__ dinv, const T *__restrict__ b,
                                                         const T *__restrict__ w, T *__restrict__ d, T *__restrict__ x,
                                                         typename VT<T>::real c0, typename VT<T>::real c1, int store_d) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long o = (long long)blockIdx.y * ld + i;
    T res = b[o];
    if (MODE != 0) res = vsub(res, w[o]);
    T dn = mg_scale(c1, vmul(dinv[i], res));
    if (MODE == 2) dn = vadd(mg_scale(c0, d[o]), dn);
    if (store_d) d[o] = dn;
    x[o] = MODE == 0 ? dn : vadd(x[o], dn);
}

// bc[I] = sum over the fine rows of aggregate I, ascending, of (b - w)[i]; then the coarse level's first smoothing step from zero:
// xc = dc = c1 dinvc bc
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_restrict_kernel(MgGrid g, int nc, long long ldf, long long ldc, const T *__restrict__ b,
                                                             const T *__restrict__ w, T *__restrict__ bc, const T *__restrict__ dinvc,
                                                             T *__restrict__ xc, T *__restrict__ dc, typename VT<T>::real c1, int store_d) {
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    const long long of = (long long)blockIdx.y * ldf, oc = (long long)blockIdx.y * ldc + I;
    const int X = I % g.cnx, t = I / g.cnx, Y = t % g.cny, Z = t / g.cny;
    T s = vzero<T>();
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * X + dx, y = 2 * Y + dy, z = 2 * Z + dz;
                if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
                const long long i = of + x + (long long)g.nx * (y + (long long)g.ny * z);
                s = vadd(s, vsub(b[i], w[i]));
            }
    bc[oc] = s;
    const T dn = mg_scale(c1, vmul(dinvc[I], s));
    xc[oc] = dn;
    if (store_d) dc[oc] = dn;
}

// x[i] += omega e[agg(i)] for the nf rows of the fine grid
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_prolong_kernel(MgGrid g, int nf, long long ldf, long long ldc, const T *__restrict__ e,
                                                            T *__restrict__ x, typename VT<T>::real omega) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const long long of = (long long)blockIdx.y * ldf + i, oc = (long long)blockIdx.y * ldc + mg_agg(i, g);
    x[of] = vadd(x[of], mg_scale(omega, e[oc]));
}

static dim3 mg_rows_grid(int n, int nrhs = 1) { return dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)nrhs); }

int launch_mg_count(const MgGrid &g, int nc, const int *ptr, const int *cols, int *count, unsigned long long *err, hipStream_t st) {
    hipLaunchKernelGGL(mg_count_kernel, mg_rows_grid(nc), dim3(kBlock), 0, st, g, nc, ptr, cols, count, err);
    return check_launch("mg_count");
}
int launch_mg_scan(int n, int *counts_to_ptr, int *overflow, hipStream_t st) {
    hipLaunchKernelGGL(mg_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, n, counts_to_ptr, overflow);
    return check_launch("mg_scan");
}
template <typename T>
static int mg_fill_impl(const MgGrid &g, int nc, const void *vals, const int *ptr, const int *cols, const int *ptrc, int *colsc, void *valsc,
                        hipStream_t st) {
    hipLaunchKernelGGL((mg_fill_kernel<T>), mg_rows_grid(nc), dim3(kBlock), 0, st, g, nc, (const T *)vals, ptr, cols, ptrc, colsc, (T *)valsc);
    return check_launch("mg_fill");
}
int launch_mg_fill(int dtype, const MgGrid &g, int nc, const void *vals, const int *ptr, const int *cols, const int *ptrc, int *colsc,
                   void *valsc, hipStream_t st) {
    CG_DISPATCH(dtype, mg_fill_impl, g, nc, vals, ptr, cols, ptrc, colsc, valsc, st);
}
template <typename T>
static int mg_gershgorin_impl(int n, const void *vals, const int *ptr, const void *dinv, unsigned long long *out, hipStream_t st) {
    hipLaunchKernelGGL((mg_gershgorin_kernel<T>), mg_rows_grid(n), dim3(kBlock), 0, st, n, (const T *)vals, ptr, (const T *)dinv, out);
    return check_launch("mg_gershgorin");
}
int launch_mg_gershgorin(int dtype, int n, const void *vals, const int *ptr, const void *dinv, unsigned long long *out, hipStream_t st) {
    CG_DISPATCH(dtype, mg_gershgorin_impl, n, vals, ptr, dinv, out, st);
}

template <typename T>
static int mg_cheb_impl(int mode, int n, long long ld, int nrhs, const void *dinv, const void *b, const void *w, void *d, void *x, double c0,
                        double c1, bool store_d, hipStream_t st) {
    using R = typename VT<T>::real;
    const dim3 g = mg_rows_grid(n, nrhs), bl(kBlock);
    const T *di = (const T *)dinv, *bb = (const T *)b, *ww = (const T *)w;
    T *dd = (T *)d, *xx = (T *)x;
    const int sd = store_d ? 1 : 0;
    if (mode == 0) hipLaunchKernelGGL((mg_cheb_kernel<T, 0>), g, bl, 0, st, n, ld, di, bb, ww, dd, xx, (R)c0, (R)c1, sd);
    else if (mode == 1) hipLaunchKernelGGL((mg_cheb_kernel<T, 1>), g, bl, 0, st, n, ld, di, bb, ww, dd, xx, (R)c0, (R)c1, sd);
    else hipLaunchKernelGGL((mg_cheb_kernel<T, 2>), g, bl, 0, st, n, ld, di, bb, ww, dd, xx, (R)c0, (R)c1, sd);
    return check_launch("mg_cheb");
}
int launch_mg_cheb(int dtype, int mode, int n, long long ld, int nrhs, const void *dinv, const void *b, const void *w, void *d, void *x,
                   double c0, double c1, bool store_d, hipStream_t st) {
    if (n <= 0) return CGAMD_OK;
    if ((mode == 2 || store_d) && !d) return fail(CGAMD_ERR_INVALID, "mg_cheb: the step needs the d vector");
    if (mode != 0 && !w) return fail(CGAMD_ERR_INVALID, "mg_cheb: the step needs w = A x");
    CG_DISPATCH(dtype, mg_cheb_impl, mode, n, ld, nrhs, dinv, b, w, d, x, c0, c1, store_d, st);
}
template <typename T>
static int mg_restrict_impl(const MgGrid &g, int nc, long long ldf, long long ldc, int nrhs, const void *b, const void *w, void *bc,
                            const void *dinvc, void *xc, void *dc, double c1, bool store_d, hipStream_t st) {
    using R = typename VT<T>::real;
    hipLaunchKernelGGL((mg_restrict_kernel<T>), mg_rows_grid(nc, nrhs), dim3(kBlock), 0, st, g, nc, ldf, ldc, (const T *)b, (const T *)w,
                       (T *)bc, (const T *)dinvc, (T *)xc, (T *)dc, (R)c1, store_d ? 1 : 0);
    return check_launch("mg_restrict");
}
int launch_mg_restrict(int dtype, const MgGrid &g, int nc, long long ldf, long long ldc, int nrhs, const void *b, const void *w, void *bc,
                       const void *dinvc, void *xc, void *dc, double c1, bool store_d, hipStream_t st) {
    if (store_d && !dc) return fail(CGAMD_ERR_INVALID, "mg_restrict: the coarse level needs its d vector");
    CG_DISPATCH(dtype, mg_restrict_impl, g, nc, ldf, ldc, nrhs, b, w, bc, dinvc, xc, dc, c1, store_d, st);
}
template <typename T>
static int mg_prolong_impl(const MgGrid &g, int nf, long long ldf, long long ldc, int nrhs, const void *e, void *x, double omega, hipStream_t st) {
    using R = typename VT<T>::real;
    hipLaunchKernelGGL((mg_prolong_kernel<T>), mg_rows_grid(nf, nrhs), dim3(kBlock), 0, st, g, nf, ldf, ldc, (const T *)e, (T *)x, (R)omega);
    return check_launch("mg_prolong");
}
int launch_mg_prolong(int dtype, const MgGrid &g, int nf, long long ldf, long long ldc, int nrhs, const void *e, void *x, double omega,
                      hipStream_t st) {
    CG_DISPATCH(dtype, mg_prolong_impl, g, nf, ldf, ldc, nrhs, e, x, omega, st);
}

}  // namespace cgamd
