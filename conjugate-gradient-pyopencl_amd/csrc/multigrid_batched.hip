// Aggregation multigrid on a BATCHED handle (cgamd_solver_set_preconditioner_batched_multigrid): the per-system forms of the setup and
// cycle kernels of multigrid.hip.  nsys systems share the box aggregates and every level's ptr / cols; what differs per system is the
// values (system r at vals + r * nnz_l, the layout of aValues), dinv (system r at dinv + r * ld) and the Chebyshev coefficients (a
// small device table of the real type, read by column).  The arithmetic of an output element is the very expression of the
// single-system kernel on (A_r, b_r): same order, same roundings, so the setup has the bits of a single-system handle made from A_r.
//   setup     the Galerkin fill collects the coarse columns of a coarse row ONCE (the pattern pass of mg_fill_kernel) and then adds
//             every system's values to its own slots; the Gershgorin bound is one word per system (a maximum: order-free).
//   V-cycle   grid.y = system.  Consecutive threads hold consecutive rows of one system, so every access is a whole cache line.
//             No reductions, no atomics: the bits do not depend on the launch geometry.  The prolongation is multigrid.hip's own
//             (the over-correction is shared); the products go through launch_spmv_batched with a plan per level.
// Everything is stream-ordered on the caller's stream.
#include <algorithm>

#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"

namespace cgamd {

CG_DEV int mgb_agg(int i, const MgGrid &g) {
    const int x = i % g.nx, t = i / g.nx, y = t % g.ny, z = t / g.ny;
    return (x >> 1) + g.cnx * ((y >> 1) + g.cny * (z >> 1));
}

// the sorted list of the distinct coarse columns of coarse row I, as mg_collect; -1 when there are more than kMgMaxRow
CG_DEV int mgb_collect(int I, const MgGrid &g, const int *__restrict__ ptr, const int *__restrict__ cols, int *list) {
    const int X = I % g.cnx, t = I / g.cnx, Y = t % g.cny, Z = t / g.cny;
    int cnt = 0;
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * X + dx, y = 2 * Y + dy, z = 2 * Z + dz;
                if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
                const int i = x + g.nx * (y + g.ny * z), end = ptr[i + 1];
                for (int j = ptr[i]; j < end; ++j) {
                    const int J = mgb_agg(cols[j], g);
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

// One thread per (coarse row, system): the list of the row once, then for every system of this thread (blockIdx.y, stepping by
// gridDim.y) the sums of mg_fill_kernel -- fine rows ascending, entries in stored order, in double / complex double, rounded once.
// The columns are written by the threads of blockIdx.y == 0
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_fill_batched_kernel(MgGrid g, int nc, int nsys, long long nnzf, long long nnzc,
                                                                 const T *__restrict__ vals, const int *__restrict__ ptr,
                                                                 const int *__restrict__ cols, const int *__restrict__ ptrc,
                                                                 int *__restrict__ colsc, T *__restrict__ valsc) {
    using A = typename VT<T>::acc;
    const int I = blockIdx.x * kBlock + threadIdx.x;
    if (I >= nc) return;
    int list[kMgMaxRow];
    A acc[kMgMaxRow];
    const int cnt = mgb_collect(I, g, ptr, cols, list);
    if (cnt < 0) return;        // (refused by the count pass)
    const int base = ptrc[I];
    if (ptrc[I + 1] - base != cnt) return;      // (the scan clamped: refused by the caller)
    if (blockIdx.y == 0)
        for (int p = 0; p < cnt; ++p) colsc[base + p] = list[p];
    const int X = I % g.cnx, t = I / g.cnx, Y = t % g.cny, Z = t / g.cny;
    for (int r = blockIdx.y; r < nsys; r += gridDim.y) {
        const T *vr = vals + (long long)r * nnzf;
        for (int p = 0; p < cnt; ++p) acc[p] = vzero<A>();
        for (int dz = 0; dz < 2; ++dz)
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    const int x = 2 * X + dx, y = 2 * Y + dy, z = 2 * Z + dz;
                    if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
                    const int i = x + g.nx * (y + g.ny * z), end = ptr[i + 1];
                    for (int j = ptr[i]; j < end; ++j) {
                        const int J = mgb_agg(cols[j], g);
                        int p = 0;
                        while (p < cnt - 1 && list[p] < J) ++p;
                        acc[p] = vadd(acc[p], to_acc(vr[j]));
                    }
                }
        T *out = valsc + (long long)r * nnzc + base;
        for (int p = 0; p < cnt; ++p) out[p] = from_acc<T>(acc[p]);
    }
}

CG_DEV double mgb_abs(float v) { return fabs((double)v); }
CG_DEV double mgb_abs(double v) { return fabs(v); }
CG_DEV double mgb_abs(float2 v) { return hypot((double)v.x, (double)v.y); }
CG_DEV double mgb_abs(double2 v) { return hypot(v.x, v.y); }

// out[r] (preset to 0) <- max_i |dinv_r[i]| sum_j |a_r[i][j]| in double, as the bits of a non-negative double: mg_gershgorin_kernel
// with blockIdx.y = system (a maximum of non-negative bit patterns: whatever the order, the same word)
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_gershgorin_batched_kernel(int n, long long nnz, long long pitch, const T *__restrict__ vals,
                                                                       const int *__restrict__ ptr, const T *__restrict__ dinv,
                                                                       unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sm[kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int r = blockIdx.y;
    double v = 0.;
    if (i < n) {
        const T *vr = vals + (long long)r * nnz;
        double s = 0.;
        const int end = ptr[i + 1];
        for (int j = ptr[i]; j < end; ++j) s += mgb_abs(vr[j]);
        v = mgb_abs(dinv[(long long)r * pitch + i]) * s;
    }
    sm[threadIdx.x] = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] = std::max(sm[threadIdx.x], sm[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out + r, sm[0]);
}

// ---- V-cycle ---------------------------------------------------------------------------------------------------------------------
CG_DEV float mgb_scale(float c, float v) { return c * v; }
CG_DEV double mgb_scale(double c, double v) { return c * v; }
CG_DEV float2 mgb_scale(float c, float2 v) { return make_float2(c * v.x, c * v.y); }
CG_DEV double2 mgb_scale(double c, double2 v) { return make_double2(c * v.x, c * v.y); }

// One Chebyshev step of mg_cheb_kernel for system blockIdx.y: dinv at r * ld, the two coefficients of this step from the table
// (c0[r], c1[r]; c0 is read by MODE 2 only)
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void mg_cheb_batched_kernel(int n, long long ld, const T *__restrict__ dinv, const T *__restrict__ b,
                                                                 const T *__restrict__ w, T *__restrict__ d, T *__restrict__ x,
                                                                 const typename VT<T>::real *__restrict__ c0,
                                                                 const typename VT<T>::real *__restrict__ c1, int store_d) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long o = (long long)blockIdx.y * ld + i;
    const typename VT<T>::real k1 = c1[blockIdx.y];
    T res = b[o];
    if (MODE != 0) res = vsub(res, w[o]);
    T dn = mgb_scale(k1, vmul(dinv[o], res));
    if (MODE == 2) dn = vadd(mgb_scale(c0[blockIdx.y], d[o]), dn);
    if (store_d) d[o] = dn;
    x[o] = MODE == 0 ? dn : vadd(x[o], dn);
}

// mg_restrict_kernel for system blockIdx.y: bc[I] = sum over the fine rows of aggregate I, ascending, of (b - w)[i]; then the coarse
// level's first smoothing step from zero with this system's dinv (at r * ldc) and coefficient: xc = dc = c1[r] dinvc bc
template <typename T>
__global__ __launch_bounds__(kBlock) void mg_restrict_batched_kernel(MgGrid g, int nc, long long ldf, long long ldc, const T *__restrict__ b,
                                                                     const T *__restrict__ w, T *__restrict__ bc,
                                                                     const T *__restrict__ dinvc, T *__restrict__ xc, T *__restrict__ dc,
                                                                     const typename VT<T>::real *__restrict__ c1, int store_d) {
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
    const T dn = mgb_scale(c1[blockIdx.y], vmul(dinvc[oc], s));
    xc[oc] = dn;
    if (store_d) dc[oc] = dn;
}

static dim3 mgb_rows_grid(int n, int ny) { return dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)ny); }

template <typename T>
static int mg_fill_batched_impl(const MgGrid &g, int nc, int nsys, long long nnzf, long long nnzc, const void *vals, const int *ptr,
                                const int *cols, const int *ptrc, int *colsc, void *valsc, hipStream_t st) {
    // systems along y: all of them in parallel while that leaves the launch below ~1024 work-groups, as the batched extractions
    const int rb = (nc + kBlock - 1) / kBlock;
    const int gy = std::max(1, std::min(std::min(nsys, 65535), (1024 + rb - 1) / rb));
    hipLaunchKernelGGL((mg_fill_batched_kernel<T>), mgb_rows_grid(nc, gy), dim3(kBlock), 0, st, g, nc, nsys, nnzf, nnzc, (const T *)vals, ptr,
                       cols, ptrc, colsc, (T *)valsc);
    return check_launch("mg_fill_batched");
}
int launch_mg_fill_batched(int dtype, const MgGrid &g, int nc, int nsys, long long nnzf, long long nnzc, const void *vals, const int *ptr,
                           const int *cols, const int *ptrc, int *colsc, void *valsc, hipStream_t st) {
    if (nc <= 0 || nsys <= 0) return CGAMD_OK;
    CG_DISPATCH(dtype, mg_fill_batched_impl, g, nc, nsys, nnzf, nnzc, vals, ptr, cols, ptrc, colsc, valsc, st);
}
template <typename T>
static int mg_gershgorin_batched_impl(int n, int nsys, long long nnz, long long pitch, const void *vals, const int *ptr, const void *dinv,
                                      unsigned long long *out, hipStream_t st) {
    hipLaunchKernelGGL((mg_gershgorin_batched_kernel<T>), mgb_rows_grid(n, nsys), dim3(kBlock), 0, st, n, nnz, pitch, (const T *)vals, ptr,
                       (const T *)dinv, out);
    return check_launch("mg_gershgorin_batched");
}
int launch_mg_gershgorin_batched(int dtype, int n, int nsys, long long nnz, long long pitch, const void *vals, const int *ptr,
                                 const void *dinv, unsigned long long *out, hipStream_t st) {
    if (n <= 0 || nsys <= 0) return CGAMD_OK;
    if (nsys > 65535) return fail(CGAMD_ERR_INVALID, "mg_gershgorin_batched: more than 65535 systems");
    CG_DISPATCH(dtype, mg_gershgorin_batched_impl, n, nsys, nnz, pitch, vals, ptr, dinv, out, st);
}

template <typename T>
static int mg_cheb_batched_impl(int mode, int n, long long ld, int nsys, const void *dinv, const void *b, const void *w, void *d, void *x,
                                const void *c0, const void *c1, bool store_d, hipStream_t st) {
    using R = typename VT<T>::real;
    const dim3 g = mgb_rows_grid(n, nsys), bl(kBlock);
    const T *di = (const T *)dinv, *bb = (const T *)b, *ww = (const T *)w;
    T *dd = (T *)d, *xx = (T *)x;
    const R *k0 = (const R *)c0, *k1 = (const R *)c1;
    const int sd = store_d ? 1 : 0;
    if (mode == 0) hipLaunchKernelGGL((mg_cheb_batched_kernel<T, 0>), g, bl, 0, st, n, ld, di, bb, ww, dd, xx, k0, k1, sd);
    else if (mode == 1) hipLaunchKernelGGL((mg_cheb_batched_kernel<T, 1>), g, bl, 0, st, n, ld, di, bb, ww, dd, xx, k0, k1, sd);
    else hipLaunchKernelGGL((mg_cheb_batched_kernel<T, 2>), g, bl, 0, st, n, ld, di, bb, ww, dd, xx, k0, k1, sd);
    return check_launch("mg_cheb_batched");
}
int launch_mg_cheb_batched(int dtype, int mode, int n, long long ld, int nsys, const void *dinv, const void *b, const void *w, void *d,
                           void *x, const void *c0, const void *c1, bool store_d, hipStream_t st) {
    if (n <= 0 || nsys <= 0) return CGAMD_OK;
    if (nsys > 65535) return fail(CGAMD_ERR_INVALID, "mg_cheb_batched: more than 65535 systems");
    if ((mode == 2 || store_d) && !d) return fail(CGAMD_ERR_INVALID, "mg_cheb_batched: the step needs the d vector");
    if (mode != 0 && !w) return fail(CGAMD_ERR_INVALID, "mg_cheb_batched: the step needs w = A x");
    if (!c1 || (mode == 2 && !c0)) return fail(CGAMD_ERR_INVALID, "mg_cheb_batched: the step needs its coefficients");
    CG_DISPATCH(dtype, mg_cheb_batched_impl, mode, n, ld, nsys, dinv, b, w, d, x, c0, c1, store_d, st);
}
template <typename T>
static int mg_restrict_batched_impl(const MgGrid &g, int nc, long long ldf, long long ldc, int nsys, const void *b, const void *w, void *bc,
                                    const void *dinvc, void *xc, void *dc, const void *c1, bool store_d, hipStream_t st) {
    using R = typename VT<T>::real;
    hipLaunchKernelGGL((mg_restrict_batched_kernel<T>), mgb_rows_grid(nc, nsys), dim3(kBlock), 0, st, g, nc, ldf, ldc, (const T *)b,
                       (const T *)w, (T *)bc, (const T *)dinvc, (T *)xc, (T *)dc, (const R *)c1, store_d ? 1 : 0);
    return check_launch("mg_restrict_batched");
}
int launch_mg_restrict_batched(int dtype, const MgGrid &g, int nc, long long ldf, long long ldc, int nsys, const void *b, const void *w,
                               void *bc, const void *dinvc, void *xc, void *dc, const void *c1, bool store_d, hipStream_t st) {
    if (nc <= 0 || nsys <= 0) return CGAMD_OK;
    if (nsys > 65535) return fail(CGAMD_ERR_INVALID, "mg_restrict_batched: more than 65535 systems");
    if (store_d && !dc) return fail(CGAMD_ERR_INVALID, "mg_restrict_batched: the coarse level needs its d vector");
    CG_DISPATCH(dtype, mg_restrict_batched_impl, g, nc, ldf, ldc, nsys, b, w, bc, dinvc, xc, dc, c1, store_d, st);
}

}  // namespace cgamd
