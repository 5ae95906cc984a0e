// The cut matrix of a rank of the row-partitioned handle (cgamd_dist_set_preconditioner_multigrid / _amg): the rank's rows with every
// entry whose column is a halo column (>= col_limit = n_local) removed, stored order kept -- the rank's diagonal block of A, which is
// what its rank-local multigrid hierarchy is built from.  Two passes and a scan, as the Galerkin products are made (multigrid.hip):
// ONE THREAD PER ROW counts the entries it keeps, launch_mg_scan turns the counts into row pointers, and the second pass walks the row
// again and writes the kept entries behind its pointer.  A third kernel writes the values alone (cgamd_dist_refresh_values on an
// unchanged pattern).  No atomics, every output element is one thread's own: the bits do not depend on the launch geometry.
#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"

namespace cgamd {

// count[i] <- kept entries of row i < nu; 0 for the padding rows nu <= i < n
__global__ __launch_bounds__(kBlock) void cut_count_kernel(int nu, int n, int col_limit, const int *__restrict__ ptr,
                                                           const int *__restrict__ cols, int *__restrict__ count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int cnt = 0;
    if (i < nu) {
        const int end = ptr[i + 1];
        for (int j = ptr[i]; j < end; ++j) cnt += cols[j] < col_limit ? 1 : 0;
    }
    count[i] = cnt;
}

// the kept entries of row i at ptrc[i] ..., in stored order; COLS = false: the values alone
template <typename T, bool COLS>
__global__ __launch_bounds__(kBlock) void cut_fill_kernel(int nu, int col_limit, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                          const int *__restrict__ cols, const int *__restrict__ ptrc,
                                                          int *__restrict__ colsc, T *__restrict__ valsc) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nu) return;
    const int end = ptr[i + 1], endc = ptrc[i + 1];
    int o = ptrc[i];
    for (int j = ptr[i]; j < end && o < endc; ++j) {
        const int c = cols[j];
        if (c >= col_limit) continue;
        if (COLS) colsc[o] = c;
        valsc[o] = vals[j];
        ++o;
    }
}

static dim3 cut_rows_grid(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

int launch_cut_count(int nu, int n, int col_limit, const int *ptr, const int *cols, int *count, hipStream_t st) {
    if (n <= 0) return CGAMD_OK;
    hipLaunchKernelGGL(cut_count_kernel, cut_rows_grid(n), dim3(kBlock), 0, st, nu, n, col_limit, ptr, cols, count);
    return check_launch("cut_count");
}
template <typename T>
static int cut_fill_impl(int nu, int col_limit, const void *vals, const int *ptr, const int *cols, const int *ptrc, int *colsc, void *valsc,
                         hipStream_t st) {
    if (colsc)
        hipLaunchKernelGGL((cut_fill_kernel<T, true>), cut_rows_grid(nu), dim3(kBlock), 0, st, nu, col_limit, (const T *)vals, ptr, cols, ptrc,
                           colsc, (T *)valsc);
    else
        hipLaunchKernelGGL((cut_fill_kernel<T, false>), cut_rows_grid(nu), dim3(kBlock), 0, st, nu, col_limit, (const T *)vals, ptr, cols, ptrc,
                           colsc, (T *)valsc);
    return check_launch("cut_fill");
}
int launch_cut_fill(int dtype, int nu, int col_limit, const void *vals, const int *ptr, const int *cols, const int *ptrc, int *colsc,
                    void *valsc, hipStream_t st) {
    if (nu <= 0) return CGAMD_OK;
    if (!colsc) return fail(CGAMD_ERR_INVALID, "cut_fill: the column array is NULL");
    CG_DISPATCH(dtype, cut_fill_impl, nu, col_limit, vals, ptr, cols, ptrc, colsc, valsc, st);
}
int launch_cut_refill(int dtype, int nu, int col_limit, const void *vals, const int *ptr, const int *cols, const int *ptrc, void *valsc,
                      hipStream_t st) {
    if (nu <= 0) return CGAMD_OK;
    CG_DISPATCH(dtype, cut_fill_impl, nu, col_limit, vals, ptr, cols, ptrc, nullptr, valsc, st);
}

}  // namespace cgamd
