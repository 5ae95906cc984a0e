// CGAMD_SPLIT_LONG_ROWS: the SpMV of the few 256-row blocks that no block form can hold ("heavy" blocks: hub rows of graph Laplacians,
// supply nets, one coupled unknown of a grid system), cut across work-groups.  spmv_impl (spmv.hip) runs every other block through
// the row-block or chunked kernel on a block list and then the two launches of this file on the same stream:
//
//   long_rows_segment_kernel   one work-group per SEGMENT of seg_len entries of a heavy block's span [ptr[r0] & ~3, ptr[r1]).  The
//                              segment's values and columns are streamed into LDS (stage_slice: 16 bytes per lane, every load
//                              instruction of a wave covers contiguous memory, non-temporal per plan.nt), the products a x replace the
//                              values there, and for every row of the block the work-group forms the row's PIECE, the sum of the row's
//                              entries inside this segment:
//                                * a piece of up to kLongRowPiece entries by ONE lane (thread t <-> row r0 + t) in stored order from
//                                  +0, sum = T(sum + T(a x)) -- the expression of every one-lane form;
//                                * a longer piece by the 64 lanes of the wave that holds its thread (wave t / 64: a rule of the matrix
//                                  alone), pieces of one wave in ascending row order: lane l adds entries l, l + 64, ... from +0, then
//                                  the tree v[l] += v[l + off], off = 32 ... 1, lane 0 (the tree wave_sum documents).
//                              A row that lies inside one segment is stored to y.  At most two rows cross a segment's edges: the piece
//                              of the row that came in over the front edge goes to scratch[seg][0] (also when it leaves over the back
//                              edge), the piece of a row that begins here and leaves over the back edge to scratch[seg][1].
//   long_rows_combine_kernel   one work-group per heavy block, thread t completes row t: an empty row is +0, a row inside one
//                              segment is read back from y, a split row is the sum of its pieces in ASCENDING segment order from +0
//                              and is stored.  Fused: the block's d.q partial, block_sum<256> of to_acc(vmul(d_i, y_i)) into
//                              partials[rb] -- tree and slot of the row-block kernel, so the alpha fold reads it unchanged.
//
// Work-groups never communicate inside a launch: the launch boundary is the synchronisation, there are no atomics and no spins, and
// every output element is one thread's own, so the bits do not depend on the launch geometry, the graph or the run.
// The lists (heavy blocks, their segments, the regular blocks in the order rowblock_of deals them) are built once per pattern by
// count, scan (launch_mg_scan) and fill, like the cut matrix of dist_cut.hip.
#include "cgamd_internal.h"
#include "device_types.h"
#include "device_mem.h"
#include "spmv_device.h"
#include "launch_util.h"

#include <algorithm>

namespace cgamd {

// ---- the lists ------------------------------------------------------------------------------------------------------------------------
// heavy_cnt[rb] <- 1 when an 8-row slice of row block rb spans more than heavy_entries entries, seg_cnt[rb] <- its segments (else 0)
__global__ __launch_bounds__(kBlock) void long_rows_mark_kernel(int n, const int *__restrict__ ptr, int row_blocks, int heavy_entries,
                                                                 int seg_len, int *heavy_cnt, int *seg_cnt) {
    const int rb = blockIdx.x * kBlock + threadIdx.x;
    if (rb >= row_blocks) return;
    const int r0 = rb * kBlock, r1 = min(r0 + kBlock, n);
    int heavy = 0;
    for (int ra = r0; ra < r1; ra += 8) heavy |= (ptr[min(ra + 8, n)] - (ptr[ra] & ~3)) > heavy_entries;
    heavy_cnt[rb] = heavy;
    const long long span = (long long)ptr[r1] - (ptr[r0] & ~3);
    seg_cnt[rb] = heavy ? (int)((span + seg_len - 1) / seg_len) : 0;
}
// after the scans: hptr[rb] = heavy blocks before rb, sptr[rb] = segments before rb
__global__ __launch_bounds__(kBlock) void long_rows_fill_kernel(const int *__restrict__ ptr, int row_blocks, int seg_len,
                                                                 const int *__restrict__ hptr, const int *__restrict__ sptr, int *heavy,
                                                                 int *seg0, int *segtab) {
    const int rb = blockIdx.x * kBlock + threadIdx.x;
    if (rb > row_blocks) return;
    if (rb == row_blocks) { seg0[hptr[rb]] = sptr[rb]; return; }
    const int h = hptr[rb];
    if (hptr[rb + 1] == h) return;          // a regular block
    heavy[h] = rb;
    seg0[h] = sptr[rb];
    const int cfirst = ptr[rb * kBlock] & ~3;
    for (int k = 0, e = sptr[rb + 1] - sptr[rb]; k < e; ++k) {
        segtab[2 * (sptr[rb] + k)] = h;
        segtab[2 * (sptr[rb] + k) + 1] = cfirst + k * seg_len;
    }
}
// the regular blocks in the order the block-cyclic schedule deals them (work-group b of a full launch takes rowblock_of(b)):
// FILL = false: cnt[b] <- 1 where work-group b has a regular block; FILL = true, after the scan: regular[dptr[b]] <- that block
template <bool FILL>
__global__ __launch_bounds__(kBlock) void long_rows_deal_kernel(int G, int row_blocks, int cycle, const int *__restrict__ hptr, int *cnt_or_ptr,
                                                                 int *regular) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= G) return;
    const int rb = rowblock_of(b, row_blocks, cycle);
    const bool reg = rb >= 0 && hptr[rb + 1] == hptr[rb];
    if constexpr (FILL) {
        if (reg) regular[cnt_or_ptr[b]] = rb;
    } else {
        cnt_or_ptr[b] = reg ? 1 : 0;
    }
}
// spmv_span_kernel over the regular blocks only: what the body's kernel is chosen from
__global__ void long_rows_span_kernel(int n, const int *__restrict__ ptr, int row_blocks, const int *__restrict__ hptr, int *out) {
    int m[6] = {0, 0, 0, 0, 0, 0}, mr = 0;
    for (int rb = blockIdx.x * blockDim.x + threadIdx.x; rb < row_blocks; rb += gridDim.x * blockDim.x) {
        if (hptr[rb + 1] != hptr[rb]) continue;
#pragma unroll
        for (int lv = 0; lv < 6; ++lv) {
            const int rows = kBlock >> lv;
            for (int c = 0; c < (1 << lv); ++c) {
                const int ra = rb * kBlock + c * rows;
                if (ra >= n) break;
                m[lv] = max(m[lv], ptr[min(ra + rows, n)] - (ptr[ra] & ~3));
            }
        }
        for (int ra = rb * kBlock; ra < min(rb * kBlock + kBlock, n); ++ra) mr = max(mr, ptr[ra + 1] - ptr[ra]);
    }
#pragma unroll
    for (int lv = 0; lv < 6; ++lv)
        if (m[lv] > 0) atomicMax(out + lv, m[lv]);
    if (mr > 0) atomicMax(out + 7, mr);
}

void free_long_rows(LongRows *lr) {
    for (void *p : {(void *)lr->regular, (void *)lr->heavy, (void *)lr->seg0, (void *)lr->segtab, lr->scratch})
        if (p) (void)hipFree(p);
    *lr = LongRows();
}

int build_long_rows(int n, const int *ptr_dev, int row_blocks, int heavy_entries, int seg_len, size_t value_bytes, int cycle, hipStream_t st,
                    LongRows *out, int spans[8]) {
    *out = LongRows();
    for (int i = 0; i < 8; ++i) spans[i] = 0;
    const int G = rowblock_grid(row_blocks, cycle);
    const size_t nh = (size_t)row_blocks + 1 + 64, nd = (size_t)G + 1 + 64;
    int *tmp = nullptr;
    CG_HIP(hipMalloc((void **)&tmp, (16 + 2 * nh + nd) * sizeof(int)));
    int *words = tmp, *hptr = tmp + 16, *sptr = hptr + nh, *dptr = sptr + nh;      // words: [0..2] scan overflow flags, [8..15] spans
    const dim3 gb((unsigned)(row_blocks / kBlock + 1)), gd((unsigned)((G + kBlock - 1) / kBlock)), blk(kBlock);
    int rc = CGAMD_OK;
    LongRows lr;
    int tot[3] = {0, 0, 0}, flags[3] = {0, 0, 0};
    auto run = [&]() -> int {
        CG_HIP(hipMemsetAsync(words, 0, 16 * sizeof(int), st));
        hipLaunchKernelGGL(long_rows_mark_kernel, gb, blk, 0, st, n, ptr_dev, row_blocks, heavy_entries, seg_len, hptr, sptr);
        if (int e = check_launch("long_rows_mark")) return e;
        if (int e = launch_mg_scan(row_blocks, hptr, words + 0, st)) return e;
        if (int e = launch_mg_scan(row_blocks, sptr, words + 1, st)) return e;
        hipLaunchKernelGGL((long_rows_deal_kernel<false>), gd, blk, 0, st, G, row_blocks, cycle, hptr, dptr, (int *)nullptr);
        if (int e = check_launch("long_rows_deal")) return e;
        if (int e = launch_mg_scan(G, dptr, words + 2, st)) return e;
        // the one host read of the totals
        CG_HIP(hipMemcpyAsync(&tot[0], hptr + row_blocks, sizeof(int), hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(&tot[1], sptr + row_blocks, sizeof(int), hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(&tot[2], dptr + G, sizeof(int), hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(flags, words, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        if (flags[0] || flags[1] || flags[2]) return fail(CGAMD_ERR_INVALID, "long rows: the segment count does not fit an int");
        if (tot[0] <= 0) return CGAMD_OK;
        lr.n_heavy = tot[0]; lr.n_seg = tot[1]; lr.n_regular = tot[2]; lr.seg_len = seg_len;
        lr.scratch_bytes = (size_t)lr.n_seg * 2 * value_bytes;
        CG_HIP(hipMalloc((void **)&lr.heavy, sizeof(int) * (size_t)lr.n_heavy));
        CG_HIP(hipMalloc((void **)&lr.seg0, sizeof(int) * ((size_t)lr.n_heavy + 1)));
        CG_HIP(hipMalloc((void **)&lr.segtab, sizeof(int) * 2 * (size_t)std::max(lr.n_seg, 1)));
        CG_HIP(hipMalloc((void **)&lr.regular, sizeof(int) * (size_t)std::max(lr.n_regular, 1)));
        CG_HIP(hipMalloc(&lr.scratch, std::max(lr.scratch_bytes, (size_t)16)));
        CG_HIP(hipMemsetAsync(lr.scratch, 0, std::max(lr.scratch_bytes, (size_t)16), st));
        hipLaunchKernelGGL(long_rows_fill_kernel, gb, blk, 0, st, ptr_dev, row_blocks, seg_len, hptr, sptr, lr.heavy, lr.seg0, lr.segtab);
        if (int e = check_launch("long_rows_fill")) return e;
        hipLaunchKernelGGL((long_rows_deal_kernel<true>), gd, blk, 0, st, G, row_blocks, cycle, hptr, dptr, lr.regular);
        if (int e = check_launch("long_rows_deal")) return e;
        int g = (row_blocks + 255) / 256;
        if (g > 1024) g = 1024;
        hipLaunchKernelGGL(long_rows_span_kernel, dim3(g), dim3(256), 0, st, n, ptr_dev, row_blocks, hptr, words + 8);
        if (int e = check_launch("long_rows_span")) return e;
        CG_HIP(hipMemcpyAsync(spans, words + 8, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        return CGAMD_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp);
    if (rc) { free_long_rows(&lr); return rc; }
    *out = lr;
    return CGAMD_OK;
}

// ---- the kernels ----------------------------------------------------------------------------------------------------------------------
template <typename T> struct LongRowsArgs {
    int n;
    long long nnz;
    const T *vals;
    const int *ptr;
    const int *cols;
    const T *x;
    T *y;
    const T *dvec;
    typename VT<T>::acc *partials;
    const int *heavy, *seg0, *segtab;
    T *scratch;
    int seg_len, n_seg, n_heavy;
};

CG_DEV float lr_shfl(float v, int src) { return __shfl(v, src, kWave); }
CG_DEV double lr_shfl(double v, int src) { return __shfl(v, src, kWave); }
CG_DEV float2 lr_shfl(float2 v, int src) { return make_float2(__shfl(v.x, src, kWave), __shfl(v.y, src, kWave)); }
CG_DEV double2 lr_shfl(double2 v, int src) { return make_double2(__shfl(v.x, src, kWave), __shfl(v.y, src, kWave)); }
CG_DEV float lr_down(float v, int off) { return __shfl_down(v, off, kWave); }
CG_DEV double lr_down(double v, int off) { return __shfl_down(v, off, kWave); }
CG_DEV float2 lr_down(float2 v, int off) { return make_float2(__shfl_down(v.x, off, kWave), __shfl_down(v.y, off, kWave)); }
CG_DEV double2 lr_down(double2 v, int off) { return make_double2(__shfl_down(v.x, off, kWave), __shfl_down(v.y, off, kWave)); }
// the tree of wave_sum in the VALUE type: v[l] += v[l + off], off = 32, 16, 8, 4, 2, 1; lane 0 holds the sum
template <typename T> CG_DEV T lr_wave_tree(T v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = vadd(v, lr_down(v, off));
    return v;
}

template <typename T, int BLOCK, bool NT>
__global__ __launch_bounds__(BLOCK) void long_rows_segment_kernel(LongRowsArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
    T *sv = reinterpret_cast<T *>(dyn_smem);                                          // [seg_len] values, then products
    int *sc = reinterpret_cast<int *>(dyn_smem + (size_t)a.seg_len * sizeof(T));      // [seg_len] columns
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int seg = blockIdx.x;
    if (seg >= a.n_seg) return;
    const int rb = a.heavy[a.segtab[2 * seg]];
    const int e0 = a.segtab[2 * seg + 1];                 // 4-aligned
    const int r0 = rb * BLOCK, r1 = min(r0 + BLOCK, a.n);
    const int row = r0 + t;
    const int rclamp = min(row, a.n - 1);
    const int s_raw = a.ptr[rclamp], e_raw = a.ptr[rclamp + 1];
    const int e1 = (int)min((long long)e0 + a.seg_len, (long long)a.ptr[r1]);
    const int len = e1 - e0;
    // entries in front of ptr[r0] (first segment: the slice start is rounded down) belong to the previous block; they are staged and
    // multiplied like the others -- valid entries of the matrix -- and no piece reads them.  The tail of the arrays: stage_slice
    stage_slice<T, BLOCK, NT>(a.vals, a.cols, a.nnz, e0, e1, sv, sc);
    __syncthreads();
    for (int i0 = t; i0 < len; i0 += 4 * BLOCK) {         // four gathers in flight per lane; a thread rewrites only what it read
        T av[4], xv[4];
        int idx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            idx[u] = min(i0 + u * BLOCK, len - 1);
            av[u] = sv[idx[u]];
            xv[u] = a.x[sc[idx[u]]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * BLOCK < len) sv[idx[u]] = vmul(av[u], xv[u]);
    }
    __syncthreads();
    const int s = s_raw, e = row < a.n ? e_raw : s_raw;
    const int lo = max(s, e0), hi = min(e, e1);
    const int plen = hi - lo;
    const bool longp = plen > kLongRowPiece;
    T sum = vzero<T>();
    if (!longp)
        for (int k = lo - e0; k < hi - e0; ++k) sum = vadd(sum, sv[k]);
    // the long pieces of this wave's 64 rows, in ascending row order, by the whole wave
    unsigned long long todo = __ballot(longp);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int plo = __shfl(lo, src, kWave) - e0, phi = __shfl(hi, src, kWave) - e0;
        T part = vzero<T>();
        for (int k = plo + lane; k < phi; k += kWave) part = vadd(part, sv[k]);
        part = lr_shfl(lr_wave_tree(part), 0);
        if (lane == src) sum = part;
    }
    if (plen > 0) {
        if (s >= e0 && e <= e1) a.y[row] = sum;                   // the row lies inside this segment
        else if (s < e0) a.scratch[2 * (size_t)seg] = sum;        // came in over the front edge
        else a.scratch[2 * (size_t)seg + 1] = sum;                // begins here, leaves over the back edge
    }
}

template <typename T, int BLOCK, bool FUSE_DOT>
__global__ __launch_bounds__(BLOCK) void long_rows_combine_kernel(LongRowsArgs<T> a) {
    using A = typename VT<T>::acc;
    __shared__ A red[BLOCK / kWave];
    const int t = threadIdx.x;
    const int h = blockIdx.x;
    if (h >= a.n_heavy) return;
    const int rb = a.heavy[h];
    const int r0 = rb * BLOCK;
    const int row = r0 + t;
    const int cfirst = a.ptr[r0] & ~3;
    const size_t sg0 = (size_t)a.seg0[h];
    T yv = vzero<T>();
    if (row < a.n) {
        const int s = a.ptr[row], e = a.ptr[row + 1];
        if (e > s) {
            const int ks = (s - cfirst) / a.seg_len, ke = (e - 1 - cfirst) / a.seg_len;
            if (ks == ke) yv = a.y[row];
            else {
                yv = vadd(yv, a.scratch[2 * (sg0 + ks) + 1]);
                for (int k = ks + 1; k <= ke; ++k) yv = vadd(yv, a.scratch[2 * (sg0 + k)]);
                a.y[row] = yv;
            }
        } else {
            a.y[row] = yv;
        }
    }
    if (FUSE_DOT) {
        const A dot1 = row < a.n ? to_acc(vmul(a.dvec[row], yv)) : vzero<A>();
        const A tot = block_sum<BLOCK>(dot1, red);
        if (t == 0) a.partials[rb] = tot;
    }
}

template <typename T>
static int long_rows_impl(const LongRows &lr, bool nt, int n, long long nnz, const void *vals, const int *ptr, const int *cols, const void *x,
                          void *y, const void *dvec, void *partials, hipStream_t st) {
    LongRowsArgs<T> a;
    a.n = n; a.nnz = nnz;
    a.vals = static_cast<const T *>(vals); a.ptr = ptr; a.cols = cols;
    a.x = static_cast<const T *>(x); a.y = static_cast<T *>(y);
    a.dvec = static_cast<const T *>(dvec);
    a.partials = static_cast<typename VT<T>::acc *>(partials);
    a.heavy = lr.heavy; a.seg0 = lr.seg0; a.segtab = lr.segtab;
    a.scratch = static_cast<T *>(lr.scratch);
    a.seg_len = lr.seg_len; a.n_seg = lr.n_seg; a.n_heavy = lr.n_heavy;
    const size_t lds = (size_t)lr.seg_len * (sizeof(T) + 4);
    const dim3 block(kBlock);
    if (lr.n_seg > 0) {
        auto kern = nt ? long_rows_segment_kernel<T, kBlock, true> : long_rows_segment_kernel<T, kBlock, false>;
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("long rows: hipFuncSetAttribute: ") + hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)lr.n_seg), block, lds, st, a);
        if (int rc = check_launch("long_rows_segment")) return rc;
    }
    if (partials) hipLaunchKernelGGL((long_rows_combine_kernel<T, kBlock, true>), dim3((unsigned)lr.n_heavy), block, 0, st, a);
    else hipLaunchKernelGGL((long_rows_combine_kernel<T, kBlock, false>), dim3((unsigned)lr.n_heavy), block, 0, st, a);
    return check_launch("long_rows_combine");
}
int launch_long_rows(int dtype, const LongRows &lr, bool nt, int n, long long nnz, const void *vals, const int *ptr, const int *cols,
                     const void *x, void *y, const void *dvec, void *partials, hipStream_t st) {
    CG_DISPATCH(dtype, long_rows_impl, lr, nt, n, nnz, vals, ptr, cols, x, y, dvec, partials, st);
}

}  // namespace cgamd
