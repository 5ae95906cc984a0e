// Preconditioners built on the device from the handle's own matrix (cgamd_solver_set_preconditioner_line / _jacobi): what
// tri_factor() and the planners of solver.cpp do on the host in serial loops over all rows, as a few passes over the matrix.
//   extract   one thread per row: the entries at column - row in {-stride, 0, +stride}, entries of a row at the same column summed
//             in stored order in double / complex double (as the SpMV adds them up), rounded once to the value type; Jacobi: 1/diag
//   flags     flag[i] = row i heads its chain (i < stride) or BOTH couplings to row i - stride are exactly zero.  On (lower, upper)
//             this is the pre-segmentation, known before factoring; on the stored factors (-l, -w c) it is the final segment rule of
//             the host route.  The final segments refine the pre-segments: an exact-zero coupling gives stored zeros.
//   factor    ONE THREAD PER PRE-SEGMENT, every row a thread: the flagged ones walk first, first + stride, ... up to the chain's
//             next flag with tri_factor's recurrence l = a / u_prev, u = b - l c_prev, w = 1 / u in double / complex double and
//             store -l, -w c, w rounded once.  On a grid the heads of the lines are consecutive rows, so the lanes of a wave walk
//             side by side and every step moves contiguous runs (the walk of pcg_tri_strided_kernel); at stride 1 the lanes are a
//             line apart and each walks contiguous rows -- a one-off setup.  The first bad row of a pre-segment goes into one
//             device word by atomicMin, (row << 2) | kind: chains are independent, so the minimum is the row the serial loop names.
//   plan      flags -> ordered start list: per 256-row block a count, an exclusive scan of the counts by one work-group, then every
//             flagged row writes itself at (block offset + rank in block); with lengths, each start walks the flags to its chain's
//             next start.  The same walk on the pre-flags, given up past the limit, tells whether a pre-segment is too long for one
//             thread (the host-route decision).
// Everything is stream-ordered on the caller's stream; the callers read back single words only (longest pre-segment, error word,
// segment count) -- and, at stride 1, the start list the host chunk planner packs.
#include <algorithm>

#include "cgamd_internal.h"
#include "device_types.h"
#include "launch_util.h"

namespace cgamd {

CG_DEV bool is_zero(float v) { return v == 0.f; }
CG_DEV bool is_zero(double v) { return v == 0.; }
CG_DEV bool is_zero(float2 v) { return v.x == 0.f && v.y == 0.f; }
CG_DEV bool is_zero(double2 v) { return v.x == 0. && v.y == 0.; }
CG_DEV bool is_finite(double v) { return isfinite(v); }
CG_DEV bool is_finite(double2 v) { return isfinite(v.x) && isfinite(v.y); }
CG_DEV double vneg(double v) { return -v; }
CG_DEV double2 vneg(double2 v) { return make_double2(-v.x, -v.y); }
template <typename A> CG_DEV A acc_one();
template <> CG_DEV double acc_one<double>() { return 1.; }
template <> CG_DEV double2 acc_one<double2>() { return make_double2(1., 0.); }

template <typename T>
__global__ __launch_bounds__(kBlock) void line_extract_kernel(int nu, int stride, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                              const int *__restrict__ cols, int col_limit, T *__restrict__ lower,
                                                              T *__restrict__ diag, T *__restrict__ upper) {
    using A = typename VT<T>::acc;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nu) return;
    A a = vzero<A>(), b = vzero<A>(), c = vzero<A>();
    const int end = ptr[i + 1];
    for (int j = ptr[i]; j < end; ++j) {
        if (cols[j] >= col_limit) continue;      // a halo column of a row-partitioned matrix: no line neighbour at any distance
        const long long off = (long long)cols[j] - i;
        if (off == 0) b = vadd(b, to_acc(vals[j]));
        else if (off == -(long long)stride) a = vadd(a, to_acc(vals[j]));
        else if (off == stride) c = vadd(c, to_acc(vals[j]));
    }
    lower[i] = from_acc<T>(a);
    diag[i] = from_acc<T>(b);
    upper[i] = from_acc<T>(c);
}

// m[i] = 1 / A[i][i]; err = smallest row whose diagonal is zero (or not stored) or not finite
template <typename T>
__global__ __launch_bounds__(kBlock) void jacobi_extract_kernel(int nu, const T *__restrict__ vals, const int *__restrict__ ptr,
                                                                const int *__restrict__ cols, T *__restrict__ m,
                                                                unsigned long long *__restrict__ err) {
    using A = typename VT<T>::acc;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nu) return;
    A b = vzero<A>();
    const int end = ptr[i + 1];
    for (int j = ptr[i]; j < end; ++j)
        if (cols[j] == i) b = vadd(b, to_acc(vals[j]));
    if (!is_finite(b) || is_zero(b)) {
        atomicMin(err, (unsigned long long)i);
        return;
    }
    m[i] = from_acc<T>(acc_div(acc_one<A>(), b));
}

// x, y: at least n values (zero beyond the caller's rows: the padding rows are decoupled)
template <typename T>
__global__ __launch_bounds__(kBlock) void line_flags_kernel(int n, int stride, const T *__restrict__ x, const T *__restrict__ y,
                                                            unsigned char *__restrict__ flags) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i < stride || (is_zero(x[i]) && is_zero(y[i - stride]))) ? 1 : 0;
}

constexpr int kFactorRows = 4;      // rows of a walk whose loads are issued together

// the walk of one pre-segment from its first row: tri_factor's recurrence, the factors stored rounded once.  The first bad row goes
// into *err by atomicMin as sys_bits | (row << 2) | kind (sys_bits: 0, or the system in the bits above the row for the batched form)
template <typename T>
CG_DEV void line_factor_walk(int nu, int stride, int first, const unsigned char *__restrict__ pre, const T *__restrict__ lower,
                             const T *__restrict__ diag, const T *__restrict__ upper, T *__restrict__ nl, T *__restrict__ ne,
                             T *__restrict__ w, unsigned long long *__restrict__ err, unsigned long long sys_bits) {
    using A = typename VT<T>::acc;
    constexpr int U = kFactorRows;
    const long long st = stride;
    const A zero = vzero<A>(), one = acc_one<A>();
    A u_prev = one, c_prev = zero;
    for (long long i0 = first; i0 < nu; i0 += U * st) {
        T a[U], b[U], c[U];
        bool stop[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const long long i = i0 + j * st;
            stop[j] = i >= nu || (i != first && pre[i]);
            if (!stop[j]) {
                a[j] = lower[i];
                b[j] = diag[i];
                c[j] = upper[i];
            }
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (stop[j]) return;        // the chain's end, or the next pre-segment's first row
            const long long i = i0 + j * st;
            // (a pre-segment's first row has a = 0 and c_prev = 0 exactly, or heads its chain: l = 0 and u = b, as the serial loop gets)
            const A av = i == first ? zero : to_acc(a[j]), bv = to_acc(b[j]), cv = to_acc(c[j]);
            if (!is_finite(av) || !is_finite(bv) || !is_finite(cv)) {
                atomicMin(err, sys_bits | ((unsigned long long)i << 2) | 0ull);
                return;
            }
            const A l = i == first ? zero : acc_div(av, u_prev);
            const A u = vsub(bv, vmul(l, c_prev));
            if (!is_finite(l) || !is_finite(u) || is_zero(u)) {
                atomicMin(err, sys_bits | ((unsigned long long)i << 2) | 1ull);
                return;
            }
            const A wi = acc_div(one, u);
            if (!is_finite(wi)) {
                atomicMin(err, sys_bits | ((unsigned long long)i << 2) | 2ull);
                return;
            }
            nl[i] = from_acc<T>(vneg(l));
            ne[i] = from_acc<T>(vneg(vmul(wi, cv)));
            w[i] = from_acc<T>(wi);
            u_prev = u;
            c_prev = cv;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void line_factor_kernel(int nu, int stride, const unsigned char *__restrict__ pre,
                                                             const T *__restrict__ lower, const T *__restrict__ diag,
                                                             const T *__restrict__ upper, T *__restrict__ nl, T *__restrict__ ne,
                                                             T *__restrict__ w, unsigned long long *__restrict__ err) {
    const int first = blockIdx.x * kBlock + threadIdx.x;
    if (first >= nu || !pre[first]) return;
    line_factor_walk<T>(nu, stride, first, pre, lower, diag, upper, nl, ne, w, err, 0ull);
}

// rows from a flagged row to its chain's next flagged row (or the chain's end); gives up once the count reaches cap (the result is
// then in [cap, cap + 8)).  Eight flags are loaded per step: the walk is a chain of dependent branches, not of dependent loads.
CG_DEV int walk_length(const unsigned char *__restrict__ flags, int n, int stride, int first, int cap) {
    int len = 1;
    for (long long j = (long long)first + stride; len < cap; j += 8ll * stride) {
        unsigned char f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long jj = j + (long long)k * stride;
            f[k] = jj < n ? flags[jj] : 1;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (f[k]) return len;
            ++len;
        }
    }
    return len;
}

__global__ __launch_bounds__(kBlock) void line_longest_kernel(int n, int stride, const unsigned char *__restrict__ flags, int cap,
                                                              int *__restrict__ longest) {
    __shared__ int top;
    if (threadIdx.x == 0) top = 0;
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && flags[i]) atomicMax(&top, walk_length(flags, n, stride, i, cap));
    __syncthreads();
    if (threadIdx.x == 0 && top) atomicMax(longest, top);
}

__global__ __launch_bounds__(kBlock) void line_count_kernel(int n, const unsigned char *__restrict__ flags, int *__restrict__ count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int c = __syncthreads_count(i < n && flags[i]);
    if (threadIdx.x == 0) count[blockIdx.x] = c;
}

// one work-group: count[0 .. nb) -> exclusive prefix sums in place, the total in count[nb]
__global__ __launch_bounds__(kBlock) void line_scan_kernel(int nb, int *__restrict__ count) {
    __shared__ int sh[kBlock];
    int carry = 0;
    for (int base = 0; base < nb; base += kBlock) {
        const int k = base + threadIdx.x;
        const int v = k < nb ? count[k] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < kBlock; d <<= 1) {
            const int t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (k < nb) count[k] = carry + sh[threadIdx.x] - v;
        carry += sh[kBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[nb] = carry;
}

// PAIRS: out[2 k] = first row, out[2 k + 1] = length of the k-th flagged row's segment; else out[k] = the k-th flagged row
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void line_emit_kernel(int n, int stride, const unsigned char *__restrict__ flags,
                                                           const int *__restrict__ block_off, int *__restrict__ out) {
    __shared__ int wave_count[kBlock / kWave];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool on = i < n && flags[i];
    const unsigned long long mask = __ballot(on);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    if (lane == 0) wave_count[wv] = __popcll(mask);
    __syncthreads();
    if (!on) return;
    int k = block_off[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int v = 0; v < wv; ++v) k += wave_count[v];
    if (PAIRS) {
        out[2 * (long long)k] = i;
        out[2 * (long long)k + 1] = walk_length(flags, n, stride, i, 0x7fffffff);
    } else {
        out[k] = i;
    }
}

// ---- the same passes for nsys matrices on one pattern (cgamd_solver_set_preconditioner_batched_jacobi / _batched_line): the values of
// system r at vals + r * nnz, the outputs of system r at r * pitch.  grid = (row blocks, gy): a thread takes one row (one pre-segment)
// of the systems blockIdx.y, blockIdx.y + gy, ...; the launch count does not depend on nsys.

// the entries of row i at column i + off, found in ONE pass over the row's columns: the position of the first and how many there are
struct RowHits {
    int first[3], count[3];      // off = -stride, 0, +stride
};
CG_DEV RowHits row_hits(const int *__restrict__ ptr, const int *__restrict__ cols, int i, int stride, bool diag_only) {
    RowHits h;
#pragma unroll
    for (int k = 0; k < 3; ++k) { h.first[k] = -1; h.count[k] = 0; }
    const int end = ptr[i + 1];
    for (int j = ptr[i]; j < end; ++j) {
        const long long off = (long long)cols[j] - i;
        const int k = off == 0 ? 1 : diag_only ? -1 : off == -(long long)stride ? 0 : off == stride ? 2 : -1;
        if (k < 0) continue;
        if (h.count[k]++ == 0) h.first[k] = j;
    }
    return h;
}
// their sum in one system, in stored order from +0 in the accumulator type (as line_extract_kernel adds them up); the row is walked
// again only where a column is stored more than once
template <typename T>
CG_DEV typename VT<T>::acc hit_sum(const T *__restrict__ vr, const int *__restrict__ cols, int i, long long want, int first, int count,
                                   int end) {
    using A = typename VT<T>::acc;
    A a = vzero<A>();
    if (count >= 1) a = vadd(a, to_acc(vr[first]));
    for (int j = first + 1; count > 1 && j < end; ++j)
        if ((long long)cols[j] - i == want) a = vadd(a, to_acc(vr[j]));
    return a;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void batched_line_extract_kernel(int nu, int stride, int nsys, long long nnz, const T *__restrict__ vals,
                                                                      const int *__restrict__ ptr, const int *__restrict__ cols,
                                                                      T *__restrict__ lower, T *__restrict__ diag, T *__restrict__ upper,
                                                                      long long pitch) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nu) return;
    const RowHits h = row_hits(ptr, cols, i, stride, false);
    const int end = ptr[i + 1];
    for (int r = blockIdx.y; r < nsys; r += gridDim.y) {
        const T *vr = vals + (long long)r * nnz;
        const long long o = (long long)r * pitch + i;
        lower[o] = from_acc<T>(hit_sum<T>(vr, cols, i, -(long long)stride, h.first[0], h.count[0], end));
        diag[o] = from_acc<T>(hit_sum<T>(vr, cols, i, 0, h.first[1], h.count[1], end));
        upper[o] = from_acc<T>(hit_sum<T>(vr, cols, i, stride, h.first[2], h.count[2], end));
    }
}

// m_r[i] = 1 / A_r[i][i]; err = (system << 32) | row of the smallest system, then the smallest row in it, with a bad diagonal
template <typename T>
__global__ __launch_bounds__(kBlock) void batched_jacobi_extract_kernel(int nu, int nsys, long long nnz, const T *__restrict__ vals,
                                                                        const int *__restrict__ ptr, const int *__restrict__ cols,
                                                                        T *__restrict__ m, long long pitch,
                                                                        unsigned long long *__restrict__ err) {
    using A = typename VT<T>::acc;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nu) return;
    const RowHits h = row_hits(ptr, cols, i, 0, true);
    const int end = ptr[i + 1];
    for (int r = blockIdx.y; r < nsys; r += gridDim.y) {
        const A b = hit_sum<T>(vals + (long long)r * nnz, cols, i, 0, h.first[1], h.count[1], end);
        if (!is_finite(b) || is_zero(b)) {
            atomicMin(err, ((unsigned long long)r << 32) | (unsigned long long)i);
            continue;
        }
        m[(long long)r * pitch + i] = from_acc<T>(acc_div(acc_one<A>(), b));
    }
}

// the rule of line_flags_kernel AND-ed over the systems: row i starts a (pre-)segment when it heads its chain or x_r[i] and
// y_r[i - stride] are exactly zero in EVERY system
template <typename T>
__global__ __launch_bounds__(kBlock) void batched_line_flags_kernel(int n, int stride, int nsys, const T *__restrict__ x,
                                                                    const T *__restrict__ y, long long pitch,
                                                                    unsigned char *__restrict__ flags) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool cut = true;
    if (i >= stride)
        for (int r = 0; r < nsys && cut; ++r) cut = is_zero(x[(long long)r * pitch + i]) && is_zero(y[(long long)r * pitch + i - stride]);
    flags[i] = cut ? 1 : 0;
}

// one thread per (pre-segment, system); the error word carries the system above the row: its minimum is the smallest system, then the
// smallest row in it.  A system whose own couplings vanish inside a shared pre-segment gets l = 0 and u = b there, as on its own
template <typename T>
__global__ __launch_bounds__(kBlock) void batched_line_factor_kernel(int nu, int stride, int nsys, const unsigned char *__restrict__ pre,
                                                                     const T *__restrict__ lower, const T *__restrict__ diag,
                                                                     const T *__restrict__ upper, T *__restrict__ nl, T *__restrict__ ne,
                                                                     T *__restrict__ w, long long pitch,
                                                                     unsigned long long *__restrict__ err) {
    const int first = blockIdx.x * kBlock + threadIdx.x;
    if (first >= nu || !pre[first]) return;
    for (int r = blockIdx.y; r < nsys; r += gridDim.y) {
        const long long o = (long long)r * pitch;
        line_factor_walk<T>(nu, stride, first, pre, lower + o, diag + o, upper + o, nl + o, ne + o, w + o, err,
                            (unsigned long long)r << kBatchedErrSystemShift);
    }
}

static int row_blocks(int n) { return (n + kBlock - 1) / kBlock; }

template <typename T>
static int extract_impl(int nu, int stride, const void *vals, const int *ptr, const int *cols, int col_limit, void *lower, void *diag,
                        void *upper, hipStream_t st) {
    hipLaunchKernelGGL((line_extract_kernel<T>), dim3(row_blocks(nu)), dim3(kBlock), 0, st, nu, stride, (const T *)vals, ptr, cols,
                       col_limit, (T *)lower, (T *)diag, (T *)upper);
    return check_launch("line_extract");
}
int launch_line_extract(int dtype, int n_user, int stride, const void *vals, const int *ptr, const int *cols, int col_limit, void *lower,
                        void *diag, void *upper, hipStream_t st) {
    CG_DISPATCH(dtype, extract_impl, n_user, stride, vals, ptr, cols, col_limit, lower, diag, upper, st);
}

template <typename T>
static int jacobi_impl(int nu, const void *vals, const int *ptr, const int *cols, void *m, unsigned long long *err, hipStream_t st) {
    hipLaunchKernelGGL((jacobi_extract_kernel<T>), dim3(row_blocks(nu)), dim3(kBlock), 0, st, nu, (const T *)vals, ptr, cols, (T *)m, err);
    return check_launch("jacobi_extract");
}
int launch_jacobi_extract(int dtype, int n_user, const void *vals, const int *ptr, const int *cols, void *m, unsigned long long *err,
                          hipStream_t st) {
    CG_DISPATCH(dtype, jacobi_impl, n_user, vals, ptr, cols, m, err, st);
}

template <typename T>
static int flags_impl(int n, int stride, const void *x, const void *y, unsigned char *flags, hipStream_t st) {
    hipLaunchKernelGGL((line_flags_kernel<T>), dim3(row_blocks(n)), dim3(kBlock), 0, st, n, stride, (const T *)x, (const T *)y, flags);
    return check_launch("line_flags");
}
int launch_line_flags(int dtype, int n, int stride, const void *x, const void *y, unsigned char *flags, hipStream_t st) {
    CG_DISPATCH(dtype, flags_impl, n, stride, x, y, flags, st);
}

template <typename T>
static int factor_impl(int nu, int stride, const unsigned char *pre, const void *lower, const void *diag, const void *upper, void *nl,
                       void *ne, void *w, unsigned long long *err, hipStream_t st) {
    hipLaunchKernelGGL((line_factor_kernel<T>), dim3(row_blocks(nu)), dim3(kBlock), 0, st, nu, stride, pre, (const T *)lower,
                       (const T *)diag, (const T *)upper, (T *)nl, (T *)ne, (T *)w, err);
    return check_launch("line_factor");
}
int launch_line_factor(int dtype, int n_user, int stride, const unsigned char *pre, const void *lower, const void *diag,
                       const void *upper, void *nl, void *ne, void *w, unsigned long long *err, hipStream_t st) {
    CG_DISPATCH(dtype, factor_impl, n_user, stride, pre, lower, diag, upper, nl, ne, w, err, st);
}

int launch_line_longest(int n, int stride, const unsigned char *flags, int cap, int *longest, hipStream_t st) {
    hipLaunchKernelGGL(line_longest_kernel, dim3(row_blocks(n)), dim3(kBlock), 0, st, n, stride, flags, cap, longest);
    return check_launch("line_longest");
}

int line_count_ints(int n) { return row_blocks(n) + 1; }
int launch_line_count(int n, const unsigned char *flags, int *count, hipStream_t st) {
    hipLaunchKernelGGL(line_count_kernel, dim3(row_blocks(n)), dim3(kBlock), 0, st, n, flags, count);
    if (int rc = check_launch("line_count")) return rc;
    hipLaunchKernelGGL(line_scan_kernel, dim3(1), dim3(kBlock), 0, st, row_blocks(n), count);
    return check_launch("line_scan");
}

int launch_line_emit(int n, int stride, bool pairs, const unsigned char *flags, const int *block_off, int *out, hipStream_t st) {
    if (pairs) hipLaunchKernelGGL((line_emit_kernel<true>), dim3(row_blocks(n)), dim3(kBlock), 0, st, n, stride, flags, block_off, out);
    else hipLaunchKernelGGL((line_emit_kernel<false>), dim3(row_blocks(n)), dim3(kBlock), 0, st, n, stride, flags, block_off, out);
    return check_launch("line_emit");
}

// work-groups along y for nsys systems: all of them in parallel while that leaves the launch below ~1024 work-groups
static dim3 batched_grid(int rows, int nsys) {
    const int rb = row_blocks(rows);
    return dim3(rb, std::max(1, std::min(std::min(nsys, 65535), (1024 + rb - 1) / rb)));
}

template <typename T>
static int batched_extract_impl(int nu, int stride, int nsys, long long nnz, const void *vals, const int *ptr, const int *cols, void *lower,
                                void *diag, void *upper, long long pitch, hipStream_t st) {
    hipLaunchKernelGGL((batched_line_extract_kernel<T>), batched_grid(nu, nsys), dim3(kBlock), 0, st, nu, stride, nsys, nnz, (const T *)vals,
                       ptr, cols, (T *)lower, (T *)diag, (T *)upper, pitch);
    return check_launch("batched_line_extract");
}
int launch_batched_line_extract(int dtype, int n_user, int stride, int nsys, long long nnz, const void *vals, const int *ptr, const int *cols,
                                void *lower, void *diag, void *upper, long long pitch, hipStream_t st) {
    CG_DISPATCH(dtype, batched_extract_impl, n_user, stride, nsys, nnz, vals, ptr, cols, lower, diag, upper, pitch, st);
}

template <typename T>
static int batched_jacobi_impl(int nu, int nsys, long long nnz, const void *vals, const int *ptr, const int *cols, void *m, long long pitch,
                               unsigned long long *err, hipStream_t st) {
    hipLaunchKernelGGL((batched_jacobi_extract_kernel<T>), batched_grid(nu, nsys), dim3(kBlock), 0, st, nu, nsys, nnz, (const T *)vals, ptr,
                       cols, (T *)m, pitch, err);
    return check_launch("batched_jacobi_extract");
}
int launch_batched_jacobi_extract(int dtype, int n_user, int nsys, long long nnz, const void *vals, const int *ptr, const int *cols, void *m,
                                  long long pitch, unsigned long long *err, hipStream_t st) {
    CG_DISPATCH(dtype, batched_jacobi_impl, n_user, nsys, nnz, vals, ptr, cols, m, pitch, err, st);
}

template <typename T>
static int batched_flags_impl(int n, int stride, int nsys, const void *x, const void *y, long long pitch, unsigned char *flags,
                              hipStream_t st) {
    hipLaunchKernelGGL((batched_line_flags_kernel<T>), dim3(row_blocks(n)), dim3(kBlock), 0, st, n, stride, nsys, (const T *)x, (const T *)y,
                       pitch, flags);
    return check_launch("batched_line_flags");
}
int launch_batched_line_flags(int dtype, int n, int stride, int nsys, const void *x, const void *y, long long pitch, unsigned char *flags,
                              hipStream_t st) {
    CG_DISPATCH(dtype, batched_flags_impl, n, stride, nsys, x, y, pitch, flags, st);
}

template <typename T>
static int batched_factor_impl(int nu, int stride, int nsys, const unsigned char *pre, const void *lower, const void *diag, const void *upper,
                               void *nl, void *ne, void *w, long long pitch, unsigned long long *err, hipStream_t st) {
    hipLaunchKernelGGL((batched_line_factor_kernel<T>), batched_grid(nu, nsys), dim3(kBlock), 0, st, nu, stride, nsys, pre, (const T *)lower,
                       (const T *)diag, (const T *)upper, (T *)nl, (T *)ne, (T *)w, pitch, err);
    return check_launch("batched_line_factor");
}
int launch_batched_line_factor(int dtype, int n_user, int stride, int nsys, const unsigned char *pre, const void *lower, const void *diag,
                               const void *upper, void *nl, void *ne, void *w, long long pitch, unsigned long long *err, hipStream_t st) {
    CG_DISPATCH(dtype, batched_factor_impl, n_user, stride, nsys, pre, lower, diag, upper, nl, ne, w, pitch, err, st);
}

}  // namespace cgamd
