// Batched SpMV: nsys matrices on ONE sparsity pattern (shared aPointers / aCols, the values of system r at vals + r * nnz),
// y_r = A_r x_r.  The shape of the reference's additive-Schwarz step with variable coefficients (as_prec with VarCoeff,
// p_h-PY_C-CL.py:1970-1985: every sub-domain has its own P[p] on the same grid), which the reference solves one sub-domain at a time.
//
// Row-block form, as spmv_rowblock_kernel: a work-group owns 256 consecutive rows.  Their column indices are one contiguous slice of
// aCols; it is read from memory ONCE per work-group (coalesced 16-byte loads into LDS) and serves every system the work-group
// walks.  Per system the value slice vals + r * nnz + [p0, p1) is streamed with the same 16-byte loads into LDS, then lane t sums
// row t in stored order from +0 (vfma = vadd(c, vmul(a, b)), -ffp-contract=off) against x + r * ldx: row i of system r has the bits
// of the single-system row-block kernel on (A_r, x_r), and the d.q partial of a block is block_sum<256> like everywhere.
//
// Alignment.  The byte offset r * nnz * sizeof(T) of a system is not a multiple of 16 in general (nor need the caller's arrays be):
// the whole value array is treated as ONE array of nsys * nnz entries and every slice is loaded from the 16-byte boundary at or
// below its first entry, so the loads are aligned whatever nnz is; `lead` entries in front of the slice travel along and are skipped
// by the row walk.  Only the very first and the very last slice of the array can reach outside it: those take guarded scalar loads
// (block-uniform branch, as stage_slice does).  The column slice is realigned the same way.
//
// Two value buffers: system r + 1 is staged while the rows of system r are walked (one barrier per system).  Where two value
// buffers and the columns exceed that limit the kernel runs on one buffer and two barriers per system.
//
// Small systems are bound by round trips, not bytes: the launcher then gives every work-group fewer systems (grid.y groups of
// `spw` systems), down to one, and the index slice is re-read out of L2 per group -- the "wide" trade of the multi-RHS kernels.
//
// Slices beyond the limit (kMaxSpmmSliceBytes for one system: values + columns of 256 rows as staged), or arrays that are not aligned to
// their own element size, take spmv_batched_direct_kernel: lane t walks row t straight from memory, one work-group per (row block,
// system).  Same order of summation, same bits, same [nsys][P] partials; uncoalesced, so slow -- it is the any-CSR fallback.
#include "cgamd_internal.h"
#include "device_types.h"
#include "device_mem.h"
#include "spmv_device.h"
#include "launch_util.h"

#include <algorithm>

namespace cgamd {

template <typename T> struct BatchedArgs {
    int n, nsys;
    long long nnz;
    const T *vals;                  // [nsys][nnz]
    const int *ptr;
    const int *cols;
    const T *x;
    long long ldx;
    T *y;
    long long ldy;
    const T *dvec;                  // fused dot: sum dvec[row + r * ldx] * y_r[row]
    typename VT<T>::acc *partials;  // [nsys][P], null = no dot
    int P;
    int row_blocks, cycle;
    int capc, capv;                 // LDS entries of the column slice and of ONE value buffer (multiples of 4)
    int vbufs;                      // value buffers: 2, or 1 where two do not fit
    int spw;                        // systems per work-group (blockIdx.y selects the group)
};

// Stage entries [g0, g1) of base[0 .. total) in LDS from the 16-byte boundary at or below base + g0: entry g lands at
// lds[g - g0 + lead], lead (the return value) < 16 / sizeof(E).  `lds` is 16-byte aligned and holds g1 - g0 + 2 * (16 / sizeof(E))
// entries.  base must be aligned to sizeof(E).
template <typename E, typename V, bool NT, int BLOCK>
CG_DEV int stage_realigned(const E *__restrict__ base, long long total, long long g0, long long g1, E *lds) {
    constexpr int EPC = 16 / (int)sizeof(E);
    const int mis = (int)((reinterpret_cast<unsigned long long>(base) / sizeof(E)) & (EPC - 1));      // entries past a boundary
    const int lead = (int)((g0 + mis) & (EPC - 1));
    const long long gfirst = g0 - lead;
    const int nchunks = (int)((g1 - gfirst + EPC - 1) / EPC);
    const int t = threadIdx.x;
    if (gfirst >= 0 && gfirst + (long long)nchunks * EPC <= total) {      // block-uniform: every chunk lies inside the array
        for (int c0 = 0; c0 < nchunks; c0 += 4 * BLOCK) {
            V ch[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c0 + i * BLOCK + t;
                if (c < nchunks) ch[i] = ld16<V, NT>(base + gfirst + (long long)c * EPC);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c0 + i * BLOCK + t;
                if (c < nchunks) *reinterpret_cast<V *>(lds + (size_t)c * EPC) = ch[i];
            }
        }
    } else {                                                               // first / last slice of the array: entry by entry
        const int cnt = (int)(g1 - g0);
        for (int j = t; j < cnt; j += BLOCK) lds[lead + j] = base[g0 + j];
    }
    return lead;
}

template <typename T, int BLOCK, bool NT, int UNROLL>
__global__ __launch_bounds__(BLOCK) void spmv_batched_kernel(BatchedArgs<T> a) {
    using A = typename VT<T>::acc;
    using V = typename Chunk16<T>::V;
    extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
    A *red = reinterpret_cast<A *>(dyn_smem);                                          // [BLOCK / 64], 64 bytes reserved
    int *sc = reinterpret_cast<int *>(dyn_smem + 64);                                  // [capc]
    T *sv = reinterpret_cast<T *>(dyn_smem + 64 + (size_t)a.capc * sizeof(int));       // [vbufs][capv]

    const int t = threadIdx.x;
    const int rb = rowblock_of(blockIdx.x, a.row_blocks, a.cycle);
    if (rb < 0) return;
    const int r_begin = blockIdx.y * a.spw, r_end = min(a.nsys, r_begin + a.spw);
    const int r0 = rb * BLOCK;
    const int row = r0 + t;
    const int rclamp = min(row, a.n - 1);
    const int s_raw = a.ptr[rclamp], e_raw = a.ptr[rclamp + 1];
    const int p0 = a.ptr[r0], p1 = a.ptr[min(r0 + BLOCK, a.n)];
    // the index slice: once per work-group, for all its systems
    const int leadc = stage_realigned<int, i32x4, NT, BLOCK>(a.cols, a.nnz, p0, p1, sc);
    const long long total = a.nnz * a.nsys;
    int leadv = stage_realigned<T, V, NT, BLOCK>(a.vals, total, (long long)r_begin * a.nnz + p0, (long long)r_begin * a.nnz + p1, sv);
    const int s = s_raw - p0, e = (row < a.n) ? e_raw - p0 : s_raw - p0;      // the row's entries, relative to the slice
    const int *scl = sc + leadc;
    __syncthreads();
    for (int r = r_begin; r < r_end; ++r) {
        const int cur = a.vbufs == 2 ? ((r - r_begin) & 1) : 0;
        int leadn = 0;
        if (a.vbufs == 2 && r + 1 < r_end)       // the next system's values travel while this one's rows are walked
            leadn = stage_realigned<T, V, NT, BLOCK>(a.vals, total, (long long)(r + 1) * a.nnz + p0, (long long)(r + 1) * a.nnz + p1,
                                                     sv + (size_t)(cur ^ 1) * a.capv);
        const T *svl = sv + (size_t)cur * a.capv + leadv;
        const T *xr = a.x + (long long)r * a.ldx;
        // row walk of spmv_rowblock_kernel: branch-free inside a batch, slots past the row's end re-read its last entry and are dropped
        T sum = vzero<T>();
        for (int k = s; k < e; k += UNROLL) {
            T xv[UNROLL], av[UNROLL];
            int cj[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int idx = min(k + j, e - 1);
                cj[j] = scl[idx];
                av[j] = svl[idx];
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) xv[j] = xr[cj[j]];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const T nxt = vfma(av[j], xv[j], sum);
                sum = vsel(k + j < e, nxt, sum);
            }
        }
        A dot1 = vzero<A>();
        if (row < a.n) {
            a.y[row + (long long)r * a.ldy] = sum;
            if (a.partials) dot1 = to_acc(vmul(a.dvec[row + (long long)r * a.ldx], sum));
        }
        if (a.partials) {                        // (block-uniform; block_sum synchronises the work-group)
            const A tot = block_sum<BLOCK>(dot1, red);
            if (t == 0) a.partials[(long long)r * a.P + rb] = tot;
        }
        if (r + 1 < r_end) {
            if (a.vbufs == 2) leadv = leadn;
            else {
                __syncthreads();                 // every row of system r is summed: the one buffer may be refilled
                leadv = stage_realigned<T, V, NT, BLOCK>(a.vals, total, (long long)(r + 1) * a.nnz + p0, (long long)(r + 1) * a.nnz + p1, sv);
            }
            __syncthreads();
        }
    }
}

// Any CSR, any alignment: lane t walks row t of system blockIdx.y straight from memory (stored order from +0: the same bits).
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void spmv_batched_direct_kernel(BatchedArgs<T> a) {
    using A = typename VT<T>::acc;
    __shared__ A red[BLOCK / kWave];
    const int t = threadIdx.x;
    const int rb = rowblock_of(blockIdx.x, a.row_blocks, a.cycle);
    if (rb < 0) return;
    const int r = blockIdx.y;
    const int row = rb * BLOCK + t;
    const T *vr = a.vals + (long long)r * a.nnz;
    const T *xr = a.x + (long long)r * a.ldx;
    T sum = vzero<T>();
    A dot1 = vzero<A>();
    if (row < a.n) {
        const int s = a.ptr[row], e = a.ptr[row + 1];
        for (int k = s; k < e; ++k) sum = vfma(vr[k], xr[a.cols[k]], sum);
        a.y[row + (long long)r * a.ldy] = sum;
        if (a.partials) dot1 = to_acc(vmul(a.dvec[row + (long long)r * a.ldx], sum));
    }
    if (a.partials) {
        const A tot = block_sum<BLOCK>(dot1, red);
        if (t == 0) a.partials[(long long)r * a.P + rb] = tot;
    }
}

template <typename T>
static int spmv_batched_impl(const SpmvPlan &plan, int n, long long nnz, int nsys, const void *vals, const int *ptr, const int *cols,
                             const void *x, long long ldx, void *y, long long ldy, const void *dvec, void *partials, hipStream_t st) {
    BatchedArgs<T> a;
    a.n = n; a.nsys = nsys; a.nnz = nnz;
    a.vals = static_cast<const T *>(vals); a.ptr = ptr; a.cols = cols;
    a.x = static_cast<const T *>(x); a.ldx = ldx;
    a.y = static_cast<T *>(y); a.ldy = ldy;
    a.dvec = static_cast<const T *>(dvec);
    a.partials = static_cast<typename VT<T>::acc *>(partials);
    a.P = plan.n_partials;
    a.row_blocks = plan.row_blocks;
    a.cycle = spmv_cycle_now(tune());
    a.capc = a.capv = 0; a.vbufs = 1; a.spw = 1;
    const bool fuse = partials != nullptr;
    const dim3 block(kBlock);
    const unsigned gx = (unsigned)rowblock_grid(plan.row_blocks, a.cycle);
    const int span = (plan.max_span + 3) & ~3;      // >= p1 - p0 of every 256-row slice
    constexpr int EPC = 16 / (int)sizeof(T);
    a.capc = span + 8;                              // lead (< 4) and the last quad's tail
    a.capv = ((span + 2 * EPC) + 3) & ~3;
    const size_t fixed = 64 + (size_t)a.capc * 4;   // the block sum's wave slots, then the columns
    const bool elem_aligned = (reinterpret_cast<uintptr_t>(vals) % sizeof(T)) == 0 && (reinterpret_cast<uintptr_t>(cols) % 4) == 0;
    const bool nt = spmv_nt_now(tune(), plan);
    if (nsys > 65535) return fail(CGAMD_ERR_INVALID, "batched spmv: more than 65535 systems");
    // the limit holds for the slice as it is staged: one system's values and the columns, with their alignment slack
    if (plan.max_span <= 0 || !elem_aligned || fixed + (size_t)a.capv * sizeof(T) > (size_t)kMaxSpmmSliceBytes) {
        const int form[kSpmvFormFields] = {6, 0, 1, 0, 0, 0, fuse, 1, (int)gx, fuse ? a.P : 0};
        record_spmv_form(form);
        hipLaunchKernelGGL((spmv_batched_direct_kernel<T, kBlock>), dim3(gx, nsys), block, 0, st, a);
        return check_launch("spmv_batched_direct");
    }
    a.vbufs = fixed + 2 * (size_t)a.capv * sizeof(T) <= (size_t)kMaxSpmmSliceBytes ? 2 : 1;
    const size_t lds = fixed + (size_t)a.vbufs * a.capv * sizeof(T);
    // systems per work-group: all of them where the row blocks alone fill the chip (the indices are then read once per SpMV), fewer
    // where that leaves CUs idle -- the largest group size that still gives ~4 work-groups per CU, else one system per work-group
    a.spw = 1;
    for (int w = nsys; w > 1; --w)
        if ((long long)plan.row_blocks * ((nsys + w - 1) / w) >= 1024) { a.spw = w; break; }
    const dim3 grid(gx, (nsys + a.spw - 1) / a.spw);
    const int fit = batch_fit(plan.max_row);
    const int unroll = sizeof(T) > 8 ? 4 : fit;
    const int form[kSpmvFormFields] = {6, 1, unroll, 0, 0, nt, fuse, 0, (int)gx, fuse ? a.P : 0};
    record_spmv_form(form);
#define CG_BT(UNR)                                                                                     \
    do {                                                                                               \
        if (nt) hipLaunchKernelGGL((spmv_batched_kernel<T, kBlock, true, UNR>), grid, block, lds, st, a);  \
        else hipLaunchKernelGGL((spmv_batched_kernel<T, kBlock, false, UNR>), grid, block, lds, st, a);    \
    } while (0)
    if constexpr (sizeof(T) > 8) CG_BT(4);
    else {
        if (unroll == 4) CG_BT(4);
        else if (unroll == 5) CG_BT(5);
        else if (unroll == 7) CG_BT(7);
        else CG_BT(8);
    }
#undef CG_BT
    return check_launch("spmv_batched");
}

int launch_spmv_batched(int dtype, const SpmvPlan &plan, int n, long long nnz, int nsys, const void *vals, const int *ptr, const int *cols,
                        const void *x, long long ldx, void *y, long long ldy, const void *dvec, void *partials, hipStream_t st) {
    if (n <= 0 || nsys <= 0) return CGAMD_OK;
    CG_DISPATCH(dtype, spmv_batched_impl, plan, n, nnz, nsys, vals, ptr, cols, x, ldx, y, ldy, dvec, partials, st);
}

}  // namespace cgamd
