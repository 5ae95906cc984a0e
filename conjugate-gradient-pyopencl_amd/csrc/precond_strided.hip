// Line preconditioner along any grid axis: a tridiagonal M that couples rows i and i +- stride (stride = nx for y-lines, nx ny for
// z-lines of an x-fastest grid).  cgamd_solver_set_preconditioner_tridiag_strided factors M once on the host (Thomas LU without
// pivoting along every chain c, c + stride, c + 2 stride, ...) and passes per row, as precond.hip gets them,
//   nl[i] = -l_i            (l_i = M[i][i-stride] / u_{i-stride}; 0 at a segment start)
//   ne[i] = -w_i M[i][i+stride]  (0 at a segment end)
//   w[i]  = 1 / u_i
// and the plan: the segments (first row, length) the chains fall into, ordered by first row.  On a grid they are the grid lines.
//
// pcg_tri_strided_kernel takes the place of pcg_tri_kernel.  ONE THREAD PER SEGMENT, no scan: thousands of lines are independent,
// and lines next to each other in the grid are next to each other in memory, so the 64 threads of a wave hold 64 consecutive
// segments and every step of the walk reads and writes one contiguous run of 64 values per vector.
//   forward   r_i -= alpha q_i (stored, r.r term) ; y_i = nl_i y_prev + r_i ; w_i y_i stored in z's storage
//   backward  z_i = ne_i z_next + (w_i y_i) (stored) ; r.z term
// z's storage is q's (in place): row i of q is read before row i of z is written, by the same thread, and no other thread
// touches a row of this segment.  The forward walk takes tri_strided_rows() rows per step and issues all their loads before the
// first use, the backward walk likewise: that keeps enough bytes in flight with one wave per 64 lines.  The loop bound is per lane:
// lanes whose segment is shorter (grid edges, extra cuts in M) idle, nothing is sorted by length.  A segment may have any length;
// few long segments (a 1-D chain at stride 2) are solved correctly but serially, one thread each.
// Partial sums: per thread in VT<T>::acc in walk order, block_sum, one partial per work-group and right-hand side; no atomics, so
// results are run-to-run identical.  UPD = false (set_rhs) skips the r update.
#include <algorithm>

#include "cgamd_internal.h"
#include "device_types.h"
#include "reduce_device.h"
#include "stop_device.h"
#include "launch_util.h"

namespace cgamd {

// rows per step of a walk: up to 4 vectors of that many values in registers (64 VGPRs in fp64 / complex64 / complex128, 32 in fp32)
template <typename T> constexpr int tri_strided_rows() { return sizeof(T) == 16 ? 4 : 8; }

// grid = (G, nRHS); thread t of the grid takes segments t, t + G kBlock, ...; P = G partials per RHS and dot product.  fpitch: values
// between the factors of consecutive right-hand sides (a batched handle), 0 = one M shared by all
// GUARD: the instantiation cgamd_solver_iterate_until launches; a right-hand side that has stopped keeps its r, z and partials
template <typename T, bool UPD, bool GUARD = false>
__global__ __launch_bounds__(kBlock) void pcg_tri_strided_kernel(const int2 *__restrict__ segs, int nsegs, int stride,
                                                                 const T *__restrict__ nl, const T *__restrict__ ne,
                                                                 const T *__restrict__ w, long long fpitch, const T *q, T *rv, T *z,
                                                                 long long ld,
                                                                 const T *__restrict__ alpha, typename VT<T>::acc *__restrict__ part_rz,
                                                                 typename VT<T>::acc *__restrict__ part_rr, CgStop gd) {
    using A = typename VT<T>::acc;
    constexpr int U = tri_strided_rows<T>();
    __shared__ A red[kBlock / kWave];
    const int rhs = blockIdx.y;
    if (GUARD && gd.stop[rhs] != 0) return;
    const long long off = (long long)rhs * ld;
    rv += off; z += off;
    if (UPD) q += off;
    nl += rhs * fpitch; ne += rhs * fpitch; w += rhs * fpitch;
    const T zero = vzero<T>();
    const T al = UPD ? alpha[rhs] : zero;
    const long long st = stride;
    A arz = vzero<A>(), arr = vzero<A>();
    for (long long sg = (long long)blockIdx.x * kBlock + threadIdx.x; sg < nsegs; sg += (long long)gridDim.x * kBlock) {
        const int2 fl = segs[sg];
        const long long first = fl.x;
        const int len = fl.y;
        // ---- forward: rows first, first + stride, ...
        T y = zero;
        int k = 0;
        for (; k + U <= len; k += U) {
            const long long i0 = first + k * st;
            T r[U], a[U], ww[U], qq[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                r[j] = rv[i0 + j * st];
                a[j] = nl[i0 + j * st];
                ww[j] = w[i0 + j * st];
                if (UPD) qq[j] = q[i0 + j * st];
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                if (UPD) {
                    r[j] = vsub(r[j], vmul(al, qq[j]));
                    rv[i0 + j * st] = r[j];
                }
                arr = vadd(arr, to_acc(vmul(r[j], r[j])));
                y = vadd(vmul(a[j], y), r[j]);
                z[i0 + j * st] = vmul(ww[j], y);
            }
        }
        for (; k < len; ++k) {
            const long long i = first + k * st;
            T r = rv[i];
            if (UPD) {
                r = vsub(r, vmul(al, q[i]));
                rv[i] = r;
            }
            arr = vadd(arr, to_acc(vmul(r, r)));
            y = vadd(vmul(nl[i], y), r);
            z[i] = vmul(w[i], y);
        }
        // ---- backward: from the last row; the rows outside whole steps first (they are the last ones written)
        T zn = zero;
        const int whole = len / U * U;
        for (k = len - 1; k >= whole; --k) {
            const long long i = first + k * st;
            zn = vadd(vmul(ne[i], zn), z[i]);
            z[i] = zn;
            arz = vadd(arz, to_acc(vmul(rv[i], zn)));
        }
        for (k = whole - U; k >= 0; k -= U) {
            const long long i0 = first + k * st;
            T r[U], e[U], wy[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                wy[j] = z[i0 + j * st];
                e[j] = ne[i0 + j * st];
                r[j] = rv[i0 + j * st];
            }
#pragma unroll
            for (int j = U - 1; j >= 0; --j) {
                zn = vadd(vmul(e[j], zn), wy[j]);
                z[i0 + j * st] = zn;
                arz = vadd(arz, to_acc(vmul(r[j], zn)));
            }
        }
    }
    const A trz = block_sum<kBlock>(arz, red);
    if (threadIdx.x == 0) part_rz[(long long)rhs * gridDim.x + blockIdx.x] = trz;
    const A trr = block_sum<kBlock>(arr, red);
    if (threadIdx.x == 0) part_rr[(long long)rhs * gridDim.x + blockIdx.x] = trr;
}

int tri_strided_grid(int nsegs) { return std::max(1, std::min((nsegs + kBlock - 1) / kBlock, 1024)); }

template <typename T>
static int tri_strided_impl(const TriLaunch &t, bool update, const void *q, void *r, void *z, long long ld, const void *alpha, int nrhs,
                            void *part_rz, void *part_rr, hipStream_t st, const CgStop *stop) {
    using A = typename VT<T>::acc;
    const dim3 g(t.grid, nrhs), blk(kBlock);
    const int2 *segs = reinterpret_cast<const int2 *>(t.segs);
    const CgStop none;
#define CG_TRIS(U, G) hipLaunchKernelGGL((pcg_tri_strided_kernel<T, U, G>), g, blk, 0, st, segs, t.nsegs, t.stride, (const T *)t.nl, (const T *)t.ne, \
                                         (const T *)t.w, t.fpitch, (const T *)q, (T *)r, (T *)z, ld, (const T *)alpha, (A *)part_rz, (A *)part_rr, G ? *stop : none)
    if (update && stop) CG_TRIS(true, true); else if (update) CG_TRIS(true, false); else CG_TRIS(false, false);
#undef CG_TRIS
    return check_launch("pcg_tri_strided");
}
int launch_pcg_tri_strided(int dtype, const TriLaunch &t, bool update, const void *q, void *r, void *z, long long ld, const void *alpha,
                           int nrhs, void *part_rz, void *part_rr, hipStream_t st, const CgStop *stop) {
    CG_DISPATCH(dtype, tri_strided_impl, t, update, q, r, z, ld, alpha, nrhs, part_rz, part_rr, st, stop);
}

}  // namespace cgamd
