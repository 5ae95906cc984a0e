// Column indices of a CSR matrix re-encoded for the single-RHS row-block SpMV (exact: the kernel rebuilds the very same column).
#include "cgamd_internal.h"
#include "device_types.h"
#include "device_mem.h"
#include "spmv_device.h"
#include "reduce_device.h"
#include "launch_util.h"
#include "row_pairs.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <functional>
#include <mutex>
#include <vector>

namespace cgamd {

// ---- one-byte column codes (SpmvPlan::codes) ---------------------------------------------------------------------------
constexpr int kDictSlots = 1024;            // open-addressing table of the distinct offsets (<= 256 accepted)
constexpr int kDictEmpty = -2147483647 - 1;
CG_DEV unsigned dict_hash(int d) { return ((unsigned)d * 2654435761u) >> 22; }   // 10 bits
// one lane per row: every (column - row) offset goes into the table; count[0] = distinct offsets so far
__global__ __launch_bounds__(256) void index_offsets_kernel(int n, const int *__restrict__ ptr, const int *__restrict__ cols,
                                                            int *table, int *count) {
    for (long long row = blockIdx.x * 256LL + threadIdx.x; row < n; row += 256LL * gridDim.x) {
        if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 256) return;     // not codable: stop early
        int last = kDictEmpty;
        for (int j = ptr[row], e = ptr[row + 1]; j < e; ++j) {
            const int d = cols[j] - (int)row;
            if (d == last) continue;
            last = d;
            unsigned h = dict_hash(d);
            int probes = 0;
            for (; probes < kDictSlots; ++probes, h = (h + 1) & (kDictSlots - 1)) {
                int v = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v == kDictEmpty) {
                    v = atomicCAS(table + h, kDictEmpty, d);
                    if (v == kDictEmpty) { atomicAdd(count, 1); break; }
                }
                if (v == d) break;
            }
            if (probes == kDictSlots) { atomicAdd(count, kDictSlots); return; }       // table full
        }
    }
}
// table slot -> code (position of the offset in the sorted dictionary); one lane per row writes its codes
__global__ __launch_bounds__(256) void index_encode_kernel(int n, const int *__restrict__ ptr, const int *__restrict__ cols,
                                                           const int *__restrict__ table, const unsigned char *__restrict__ slot_code,
                                                           unsigned char *__restrict__ codes) {
    __shared__ int stab[kDictSlots];
    __shared__ unsigned char scode[kDictSlots];
    for (int i = threadIdx.x; i < kDictSlots; i += 256) { stab[i] = table[i]; scode[i] = slot_code[i]; }
    __syncthreads();
    for (long long row = blockIdx.x * 256LL + threadIdx.x; row < n; row += 256LL * gridDim.x) {
        for (int j = ptr[row], e = ptr[row + 1]; j < e; ++j) {
            const int d = cols[j] - (int)row;
            unsigned h = dict_hash(d);
            while (stab[h] != d) h = (h + 1) & (kDictSlots - 1);      // every offset is in the table
            codes[j] = scode[h];
        }
    }
}

int build_index_codes(int n, long long nnz, const int *ptr_dev, const int *cols_dev, hipStream_t st, unsigned char **codes_out,
                      int **dict_out, int *distinct_out) {
    *codes_out = nullptr;
    *dict_out = nullptr;
    *distinct_out = 0;
    if (n <= 0 || nnz <= 0) return CGAMD_OK;
    int *work = nullptr;        // [1024 table | 1 count | 256 dict]
    CG_HIP(hipMalloc((void **)&work, (kDictSlots + 64 + 256) * sizeof(int) + kDictSlots));
    std::vector<int> table(kDictSlots + 1, kDictEmpty);
    table[kDictSlots] = 0;
    hipError_t e = hipMemcpyAsync(work, table.data(), (kDictSlots + 1) * sizeof(int), hipMemcpyHostToDevice, st);
    int g = (int)std::min<long long>((n + 255LL) / 256, 8192);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(index_offsets_kernel, dim3(g), dim3(256), 0, st, n, ptr_dev, cols_dev, work, work + kDictSlots);
        e = hipMemcpyAsync(table.data(), work, (kDictSlots + 1) * sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(work); return fail(CGAMD_ERR_HIP, std::string("build_index_codes: ") + hipGetErrorString(e)); }
    const int distinct = table[kDictSlots];
    if (distinct < 1 || distinct > 256) { (void)hipFree(work); return CGAMD_OK; }
    std::vector<int> dict;
    for (int i = 0; i < kDictSlots; ++i)
        if (table[i] != kDictEmpty) dict.push_back(table[i]);
    std::sort(dict.begin(), dict.end());
    std::vector<unsigned char> slot_code(kDictSlots, 0);
    for (int i = 0; i < kDictSlots; ++i)
        if (table[i] != kDictEmpty) slot_code[i] = (unsigned char)(std::lower_bound(dict.begin(), dict.end(), table[i]) - dict.begin());
    dict.resize(256, dict[0]);
    unsigned char *codes = nullptr;
    int *dict_dev = nullptr;
    unsigned char *slot_dev = reinterpret_cast<unsigned char *>(work + kDictSlots + 64 + 256);
    e = hipMalloc((void **)&codes, (size_t)nnz + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&dict_dev, 256 * sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(codes + nnz, 0, 64, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dict_dev, dict.data(), 256 * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(slot_dev, slot_code.data(), kDictSlots, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(index_encode_kernel, dim3(g), dim3(256), 0, st, n, ptr_dev, cols_dev, work, slot_dev, codes);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(work);
    if (e != hipSuccess) {
        if (codes) (void)hipFree(codes);
        if (dict_dev) (void)hipFree(dict_dev);
        return fail(CGAMD_ERR_HIP, std::string("build_index_codes: ") + hipGetErrorString(e));
    }
    *codes_out = codes;
    *dict_out = dict_dev;
    *distinct_out = distinct;
    return CGAMD_OK;
}

// ---- 16-bit block-relative columns ---------------------------------------------------------------------------------------
// For matrices with more than 256 distinct (column - row) offsets -- unstructured meshes, banded random patterns, everything a
// Matrix-Market file may hold (reference main.c:20-33) -- whose 256-row blocks still span fewer than 65 536 columns each (any
// matrix with a bandwidth below ~32k: a reasonable ordering of a mesh): codes16[j] = aCols[j] - base[rb(j)], base[rb] = the
// smallest column of row block rb.  2 instead of 4 index bytes per non-zero; exact like the one-byte codes.
__global__ __launch_bounds__(256) void rowblock_colrange_kernel(int n, const int *__restrict__ ptr, const int *__restrict__ cols, int row_blocks,
                                                                int *__restrict__ base, int *flag) {
    __shared__ int smin, smax;
    const int rb = blockIdx.x;
    if (threadIdx.x == 0) { smin = 0x7fffffff; smax = -1; }
    __syncthreads();
    const int p0 = ptr[rb * 256], p1 = ptr[min(rb * 256 + 256, n)];
    int cmin = 0x7fffffff, cmax = -1;
    for (int j = p0 + (int)threadIdx.x; j < p1; j += 256) { cmin = min(cmin, cols[j]); cmax = max(cmax, cols[j]); }
    atomicMin(&smin, cmin);
    atomicMax(&smax, cmax);
    __syncthreads();
    if (threadIdx.x == 0) {
        base[rb] = smax >= 0 ? smin : 0;
        if (smax >= 0 && smax - smin > 65535) atomicOr(flag, 1);
    }
}
__global__ __launch_bounds__(256) void index_encode16_kernel(int n, const int *__restrict__ ptr, const int *__restrict__ cols,
                                                             const int *__restrict__ base, unsigned short *__restrict__ codes) {
    const int rb = blockIdx.x;
    const int p0 = ptr[rb * 256], p1 = ptr[min(rb * 256 + 256, n)], b = base[rb];
    for (int j = p0 + (int)threadIdx.x; j < p1; j += 256) codes[j] = (unsigned short)(cols[j] - b);
}

// *codes_out (2 nnz + 64 bytes) and *base_out (row_blocks ints) are device allocations the caller frees; both null when some row
// block spans 65 536 columns or more.  Synchronises `st`.
int build_index_codes16(int n, long long nnz, const int *ptr_dev, const int *cols_dev, hipStream_t st, unsigned char **codes_out, int **base_out) {
    *codes_out = nullptr;
    *base_out = nullptr;
    if (n <= 0 || nnz <= 0) return CGAMD_OK;
    const int row_blocks = (n + 255) / 256;
    int *base = nullptr, *flag = nullptr;
    CG_HIP(hipMalloc((void **)&base, sizeof(int) * (size_t)row_blocks + 16));
    flag = base + row_blocks;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
    int bad = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rowblock_colrange_kernel, dim3(row_blocks), dim3(256), 0, st, n, ptr_dev, cols_dev, row_blocks, base, flag);
        e = hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || bad) {
        (void)hipFree(base);
        return e == hipSuccess ? CGAMD_OK : fail(CGAMD_ERR_HIP, std::string("build_index_codes16: ") + hipGetErrorString(e));
    }
    unsigned char *codes = nullptr;
    e = hipMalloc((void **)&codes, 2 * (size_t)nnz + 64);
    if (e == hipSuccess) e = hipMemsetAsync(codes + 2 * (size_t)nnz, 0, 64, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(index_encode16_kernel, dim3(row_blocks), dim3(256), 0, st, n, ptr_dev, cols_dev, base, reinterpret_cast<unsigned short *>(codes));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        if (codes) (void)hipFree(codes);
        (void)hipFree(base);
        return fail(CGAMD_ERR_HIP, std::string("build_index_codes16: ") + hipGetErrorString(e));
    }
    *codes_out = codes;
    *base_out = base;
    return CGAMD_OK;
}

// -------------------------------------------------------------------------------------------------
// VALUE codes: matrices with at most 256 distinct entries (constant-coefficient stencils, graph Laplacians, lattice operators: the
// headline system has 2) keep `vcodes[nnz]` (one byte each) and `vdict[256]` with aValues[j] == vdict[vcodes[j]] -- the same bits, so
// every product, sum and history is bit-identical to the kernels that read aValues.  With the column codes the SpMV then streams 2
// bytes per non-zero instead of sizeof(T) + 1 (fp64: 9).  Built with an open-addressing table of the value bits (4096 slots): a pass
// that inserts (it stops as soon as a 257th value shows up), a one-work-group pass that numbers the occupied slots, a pass that
// encodes.  Which code a value gets may differ from run to run (insertion races); the value it stands for does not.
// -------------------------------------------------------------------------------------------------
constexpr int kVSlots = 4096;
constexpr unsigned long long kVEmpty = ~0ULL;      // (a NaN pattern: a matrix that holds it is not coded)
template <typename T> CG_DEV unsigned long long value_key(const T &v) {
    if constexpr (sizeof(T) == 4) { unsigned b; __builtin_memcpy(&b, &v, 4); return b; }
    else { unsigned long long b; __builtin_memcpy(&b, &v, 8); return b; }
}
CG_DEV unsigned vhash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 29;
    return (unsigned)k & (kVSlots - 1);
}
// state: [0] number of distinct values, [1] failure flag
template <typename T>
__global__ __launch_bounds__(256) void value_insert_kernel(long long nnz, const T *__restrict__ vals, unsigned long long *table, int *state) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride) {
        if (__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const unsigned long long key = value_key(vals[j]);
        if (key == kVEmpty) { atomicExch(state + 1, 1); return; }
        unsigned s = vhash(key);
        for (int probe = 0; probe < kVSlots; ++probe, s = (s + 1) & (kVSlots - 1)) {
            unsigned long long cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == key) break;
            if (cur == kVEmpty) {
                cur = atomicCAS(table + s, kVEmpty, key);
                if (cur == kVEmpty) {                       // a new value
                    if (atomicAdd(state, 1) >= 256) atomicExch(state + 1, 1);
                    break;
                }
                if (cur == key) break;
            }
        }
    }
}
// one work-group: occupied slot -> code (slot order), dictionary entries
template <typename T>
__global__ __launch_bounds__(1024) void value_number_kernel(const unsigned long long *table, unsigned short *slot_code, T *vdict) {
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    int mine = 0;
    for (int k = 0; k < kVSlots / 1024; ++k) mine += table[t * (kVSlots / 1024) + k] != kVEmpty;
    int incl = mine;                                        // inclusive scan over the wave, then over the waves
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if ((t & 63) >= off) incl += o; }
    if ((t & 63) == 63) wsum[t >> 6] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < (t >> 6); ++w) base += wsum[w];
    int code = base + incl - mine;
    for (int k = 0; k < kVSlots / 1024; ++k) {
        const int s = t * (kVSlots / 1024) + k;
        const unsigned long long key = table[s];
        if (key != kVEmpty) {
            slot_code[s] = (unsigned short)code;
            if (code < 256) {
                T v;
                if constexpr (sizeof(T) == 4) { const unsigned b = (unsigned)key; __builtin_memcpy(&v, &b, 4); }
                else __builtin_memcpy(&v, &key, 8);
                vdict[code] = v;
            }
            ++code;
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void value_encode_kernel(long long nnz, const T *__restrict__ vals, const unsigned long long *__restrict__ table,
                                                           const unsigned short *__restrict__ slot_code, unsigned char *__restrict__ vcodes) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride) {
        const unsigned long long key = value_key(vals[j]);
        unsigned s = vhash(key);
        while (table[s] != key) s = (s + 1) & (kVSlots - 1);     // present: the insert pass put it there
        vcodes[j] = (unsigned char)slot_code[s];
    }
}

template <typename T>
static int build_value_codes_impl(long long nnz, const void *vals_dev, hipStream_t st, unsigned char **vcodes_out, void **vdict_out, int *n_values) {
    // scratch: table | slot codes | state
    char *scratch = nullptr;
    const size_t tb = sizeof(unsigned long long) * kVSlots, sb = sizeof(unsigned short) * kVSlots;
    CG_HIP(hipMalloc((void **)&scratch, tb + sb + 16));
    auto *table = reinterpret_cast<unsigned long long *>(scratch);
    auto *slot_code = reinterpret_cast<unsigned short *>(scratch + tb);
    int *state = reinterpret_cast<int *>(scratch + tb + sb);
    int h[2] = {0, 1};
    hipError_t e = hipMemsetAsync(table, 0xff, tb, st);
    if (e == hipSuccess) e = hipMemsetAsync(state, 0, 8, st);
    const int grid = (int)std::min<long long>((nnz + 255) / 256, 4096);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((value_insert_kernel<T>), dim3(grid), dim3(256), 0, st, nnz, static_cast<const T *>(vals_dev), table, state);
        e = hipMemcpyAsync(h, state, 8, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || h[1] != 0 || h[0] < 1 || h[0] > 256) {
        (void)hipFree(scratch);
        return e == hipSuccess ? CGAMD_OK : fail(CGAMD_ERR_HIP, std::string("build_value_codes: ") + hipGetErrorString(e));
    }
    unsigned char *vcodes = nullptr;
    void *vdict = nullptr;
    e = hipMalloc((void **)&vcodes, (size_t)nnz + 64);
    if (e == hipSuccess) e = hipMalloc(&vdict, 256 * sizeof(T));
    if (e == hipSuccess) e = hipMemsetAsync(vcodes + (size_t)nnz, 0, 64, st);
    if (e == hipSuccess) e = hipMemsetAsync(vdict, 0, 256 * sizeof(T), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((value_number_kernel<T>), dim3(1), dim3(1024), 0, st, table, slot_code, static_cast<T *>(vdict));
        hipLaunchKernelGGL((value_encode_kernel<T>), dim3(grid), dim3(256), 0, st, nnz, static_cast<const T *>(vals_dev), table, slot_code, vcodes);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (e != hipSuccess) {
        if (vcodes) (void)hipFree(vcodes);
        if (vdict) (void)hipFree(vdict);
        return fail(CGAMD_ERR_HIP, std::string("build_value_codes: ") + hipGetErrorString(e));
    }
    *vcodes_out = vcodes; *vdict_out = vdict; *n_values = h[0];
    return CGAMD_OK;
}
// *vcodes_out (nnz + 64 bytes) and *vdict_out (256 values) are device allocations the caller frees; both null when the matrix has more
// than 256 distinct values (or is complex128).  Synchronises `st`.
int build_value_codes(int dtype, long long nnz, const void *vals_dev, hipStream_t st, unsigned char **vcodes_out, void **vdict_out, int *n_values) {
    *vcodes_out = nullptr; *vdict_out = nullptr; *n_values = 0;
    if (nnz <= 0 || dtype == CGAMD_C128) return CGAMD_OK;
    if (dtype == CGAMD_F32) return build_value_codes_impl<float>(nnz, vals_dev, st, vcodes_out, vdict_out, n_values);
    if (dtype == CGAMD_F64) return build_value_codes_impl<double>(nnz, vals_dev, st, vcodes_out, vdict_out, n_values);
    return build_value_codes_impl<float2>(nnz, vals_dev, st, vcodes_out, vdict_out, n_values);
}

// -------------------------------------------------------------------------------------------------
// JOINT codes: where a matrix has both one-byte column codes and one-byte value codes and at most 256 distinct (offset, value)
// PAIRS (a constant-coefficient stencil has as many pairs as offsets: 7), one byte per non-zero names the pair: jdict_off[code] /
// jdict_val[code].  The SpMV then streams 1 byte per non-zero and does one look-up per entry instead of two.  Built from the two
// code arrays: mark the pairs that occur (65 536 possible), number them in order, encode.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_mark_kernel(long long nnz, const unsigned char *__restrict__ codes, const unsigned char *__restrict__ vcodes,
                                                        unsigned char *present) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride) {
        const unsigned k = ((unsigned)codes[j] << 8) | vcodes[j];
        if (!present[k]) present[k] = 1;            // (racing writers store the same byte)
    }
}
template <typename T>
__global__ __launch_bounds__(1024) void pair_number_kernel(const unsigned char *present, const int *__restrict__ dict, const T *__restrict__ vdict,
                                                           unsigned short *pair_code, int *joff, T *jval, int *count) {
    // joff[256 + code]: the value code of pair `code` (joint_value_map; what refresh_value_dicts rewrites jval from)
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    int mine = 0;
    for (int k = 0; k < 64; ++k) mine += present[t * 64 + k] != 0;
    int incl = mine;
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if ((t & 63) >= off) incl += o; }
    if ((t & 63) == 63) wsum[t >> 6] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < (t >> 6); ++w) base += wsum[w];
    int code = base + incl - mine;
    for (int k = 0; k < 64; ++k) {
        const int p = t * 64 + k;
        if (present[p]) {
            pair_code[p] = (unsigned short)code;
            if (code < 256) { joff[code] = dict[p >> 8]; jval[code] = vdict[p & 255]; joff[256 + code] = p & 255; }
            ++code;
        }
    }
    if (t == 1023) *count = code;
}
__global__ __launch_bounds__(256) void pair_encode_kernel(long long nnz, const unsigned char *__restrict__ codes, const unsigned char *__restrict__ vcodes,
                                                          const unsigned short *__restrict__ pair_code, unsigned char *__restrict__ jcodes) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride)
        jcodes[j] = (unsigned char)pair_code[((unsigned)codes[j] << 8) | vcodes[j]];
}
template <typename T>
static int build_joint_codes_impl(long long nnz, const unsigned char *codes, const unsigned char *vcodes, const int *dict, const void *vdict,
                                  hipStream_t st, unsigned char **jcodes_out, int **joff_out, void **jval_out, int *n_pairs) {
    char *scratch = nullptr;
    CG_HIP(hipMalloc((void **)&scratch, 65536 + 65536 * 2 + 16));
    unsigned char *present = reinterpret_cast<unsigned char *>(scratch);
    unsigned short *pair_code = reinterpret_cast<unsigned short *>(scratch + 65536);
    int *count = reinterpret_cast<int *>(scratch + 65536 * 3);
    unsigned char *jcodes = nullptr;
    int *joff = nullptr;
    void *jval = nullptr;
    int h = 0;
    hipError_t e = hipMemsetAsync(scratch, 0, 65536 * 3 + 16, st);
    if (e == hipSuccess) e = hipMalloc((void **)&joff, 512 * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&jval, 256 * sizeof(T));
    if (e == hipSuccess) e = hipMemsetAsync(joff, 0, 512 * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(jval, 0, 256 * sizeof(T), st);
    const int grid = (int)std::min<long long>((nnz + 255) / 256, 4096);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pair_mark_kernel, dim3(grid), dim3(256), 0, st, nnz, codes, vcodes, present);
        hipLaunchKernelGGL((pair_number_kernel<T>), dim3(1), dim3(1024), 0, st, present, dict, static_cast<const T *>(vdict), pair_code, joff, static_cast<T *>(jval), count);
        e = hipMemcpyAsync(&h, count, sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h >= 1 && h <= 256) {
        e = hipMalloc((void **)&jcodes, (size_t)nnz + 64);
        if (e == hipSuccess) e = hipMemsetAsync(jcodes + (size_t)nnz, 0, 64, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(pair_encode_kernel, dim3(grid), dim3(256), 0, st, nnz, codes, vcodes, pair_code, jcodes);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(scratch);
    if (e != hipSuccess || !jcodes) {
        if (jcodes) (void)hipFree(jcodes);
        if (joff) (void)hipFree(joff);
        if (jval) (void)hipFree(jval);
        return e == hipSuccess ? CGAMD_OK : fail(CGAMD_ERR_HIP, std::string("build_joint_codes: ") + hipGetErrorString(e));
    }
    *jcodes_out = jcodes; *joff_out = joff; *jval_out = jval; *n_pairs = h;
    return CGAMD_OK;
}
// all three outputs null when the matrix has more than 256 distinct (offset, value) pairs.  Synchronises `st`.
int build_joint_codes(int dtype, long long nnz, const unsigned char *codes, const unsigned char *vcodes, const int *dict, const void *vdict,
                      hipStream_t st, unsigned char **jcodes_out, int **joff_out, void **jval_out, int *n_pairs) {
    *jcodes_out = nullptr; *joff_out = nullptr; *jval_out = nullptr; *n_pairs = 0;
    if (nnz <= 0 || !codes || !vcodes || dtype == CGAMD_C128) return CGAMD_OK;
    if (dtype == CGAMD_F32) return build_joint_codes_impl<float>(nnz, codes, vcodes, dict, vdict, st, jcodes_out, joff_out, jval_out, n_pairs);
    if (dtype == CGAMD_F64) return build_joint_codes_impl<double>(nnz, codes, vcodes, dict, vdict, st, jcodes_out, joff_out, jval_out, n_pairs);
    return build_joint_codes_impl<float2>(nnz, codes, vcodes, dict, vdict, st, jcodes_out, joff_out, jval_out, n_pairs);
}

// -------------------------------------------------------------------------------------------------
// ROW-PATTERN codes: a row's pattern is its sequence of joint codes in stored order -- the (offset, value) pairs it multiplies, one
// after the other.  A constant-coefficient stencil has few of them (the 7-point Laplacian 27: interior, 6 faces, 12 edges, 8 corners;
// the 5-point one 9), so where no row is longer than 7 entries and at most 256 patterns occur, ONE byte per ROW names the pattern and
// the SpMV streams n bytes of matrix instead of nnz bytes and the row pointers.  The key of a row is one 64-bit word: the length in
// byte 0, the joint codes in bytes 1 .. 7, unused bytes 0 (rows without entries: key 0).  Passes as for the value codes: insert into
// an open-addressing table (stops at the 257th key), one work-group numbers the keys BY ASCENDING KEY (a dump of the dictionary is
// the same run to run; the SpMV does not depend on the numbering) and writes the dictionary, encode.
// -------------------------------------------------------------------------------------------------
constexpr int kRSlots = 2048;
constexpr unsigned long long kREmpty = ~0ULL;      // (length byte 255: no row has it)
CG_DEV unsigned rhash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 29;
    return (unsigned)k & (kRSlots - 1);
}
CG_DEV unsigned long long row_key(const int *__restrict__ ptr, const unsigned char *__restrict__ jcodes, long long row) {
    const int s = ptr[row], len = ptr[row + 1] - s;        // (len <= 7: the caller checked the longest row)
    unsigned long long key = (unsigned long long)len;
    for (int j = 0; j < len; ++j) key |= (unsigned long long)jcodes[s + j] << (8 * (j + 1));
    return key;
}
// state: [0] number of distinct keys, [1] failure flag, [2] set when one of the caller's rows (row < n_user) has no entry: the rows a
// handle appends (pad_rows) are empty too, and the length-0 pattern they bring is not one of the caller's matrix
__global__ __launch_bounds__(256) void rowcode_insert_kernel(int n, int n_user, const int *__restrict__ ptr, const unsigned char *__restrict__ jcodes,
                                                             unsigned long long *table, int *state) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += stride) {
        if (__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const unsigned long long key = row_key(ptr, jcodes, row);
        if (key == 0 && row < n_user && !__hip_atomic_load(state + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicExch(state + 2, 1);
        unsigned s = rhash(key);
        for (int probe = 0; probe < kRSlots; ++probe, s = (s + 1) & (kRSlots - 1)) {
            unsigned long long cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == key) break;
            if (cur == kREmpty) {
                cur = atomicCAS(table + s, kREmpty, key);
                if (cur == kREmpty) {                       // a new pattern
                    if (atomicAdd(state, 1) >= 256) atomicExch(state + 1, 1);
                    break;
                }
                if (cur == key) break;
            }
        }
    }
}
// one work-group: occupied slot -> number of smaller keys in the table; dictionary entry of that number (unused slots stay 0)
template <typename T>
__global__ __launch_bounds__(1024) void rowcode_number_kernel(const unsigned long long *table, const int *__restrict__ joff, const T *__restrict__ jval,
                                                              unsigned short *slot_code, int *rlen, int *roff, T *rval, unsigned char *rjmap) {
    __shared__ unsigned long long keys[kRSlots];
    for (int s = threadIdx.x; s < kRSlots; s += 1024) keys[s] = table[s];
    __syncthreads();
    for (int s = threadIdx.x; s < kRSlots; s += 1024) {
        const unsigned long long key = keys[s];
        if (key == kREmpty) continue;
        int code = 0;
        for (int o = 0; o < kRSlots; ++o) code += keys[o] < key;        // (empty slots hold the largest word)
        slot_code[s] = (unsigned short)code;
        if (code >= 256) continue;                                      // (cannot happen: the caller checked the count)
        const int len = (int)(key & 255);
        rlen[code] = len;
        for (int j = 0; j < len; ++j) {
            const int jc = (int)((key >> (8 * (j + 1))) & 255);
            roff[code * 8 + j] = joff[jc] * (int)sizeof(T);             // byte offsets, as the kernel adds them
            rval[code * 8 + j] = jval[jc];
            rjmap[code * 8 + j] = (unsigned char)jc;                    // (row_dict_jmap_at: what refresh_value_dicts rewrites rval from)
        }
    }
}
__global__ __launch_bounds__(256) void rowcode_encode_kernel(int n, const int *__restrict__ ptr, const unsigned char *__restrict__ jcodes,
                                                             const unsigned long long *__restrict__ table, const unsigned short *__restrict__ slot_code,
                                                             unsigned char *__restrict__ rcodes) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += stride) {
        const unsigned long long key = row_key(ptr, jcodes, row);
        unsigned s = rhash(key);
        while (table[s] != key) s = (s + 1) & (kRSlots - 1);     // present: the insert pass put it there
        rcodes[row] = (unsigned char)slot_code[s];
    }
}

template <typename T>
static int build_row_codes_impl(int n, int n_user, const int *ptr, const unsigned char *jcodes, const int *joff, const void *jval, hipStream_t st,
                                unsigned char **rcodes_out, void **rdict_out, int *n_patterns, int *n_user_patterns) {
    char *scratch = nullptr;
    const size_t tb = sizeof(unsigned long long) * kRSlots, sb = sizeof(unsigned short) * kRSlots;
    CG_HIP(hipMalloc((void **)&scratch, tb + sb + 16));
    auto *table = reinterpret_cast<unsigned long long *>(scratch);
    auto *slot_code = reinterpret_cast<unsigned short *>(scratch + tb);
    int *state = reinterpret_cast<int *>(scratch + tb + sb);
    int h[3] = {0, 1, 0};
    hipError_t e = hipMemsetAsync(table, 0xff, tb, st);
    if (e == hipSuccess) e = hipMemsetAsync(state, 0, 12, st);
    const int grid = (int)std::min<long long>((n + 255LL) / 256, 4096);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rowcode_insert_kernel, dim3(grid), dim3(256), 0, st, n, n_user, ptr, jcodes, table, state);
        e = hipMemcpyAsync(h, state, 12, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || h[1] != 0 || h[0] < 1 || h[0] > 256) {
        (void)hipFree(scratch);
        return e == hipSuccess ? CGAMD_OK : fail(CGAMD_ERR_HIP, std::string("build_row_codes: ") + hipGetErrorString(e));
    }
    unsigned char *rcodes = nullptr;
    char *rdict = nullptr;
    const size_t db = row_dict_alloc_bytes(sizeof(T));
    e = hipMalloc((void **)&rcodes, (size_t)n + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&rdict, db);
    if (e == hipSuccess) e = hipMemsetAsync(rcodes + (size_t)n, 0, 64, st);
    if (e == hipSuccess) e = hipMemsetAsync(rdict, 0, db, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((rowcode_number_kernel<T>), dim3(1), dim3(1024), 0, st, table, joff, static_cast<const T *>(jval), slot_code,
                           reinterpret_cast<int *>(rdict + row_dict_len_at(sizeof(T))), reinterpret_cast<int *>(rdict + row_dict_off_at(sizeof(T))),
                           reinterpret_cast<T *>(rdict), reinterpret_cast<unsigned char *>(rdict + row_dict_jmap_at(sizeof(T))));
        hipLaunchKernelGGL(rowcode_encode_kernel, dim3(grid), dim3(256), 0, st, n, ptr, jcodes, table, slot_code, rcodes);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (e != hipSuccess) {
        if (rcodes) (void)hipFree(rcodes);
        if (rdict) (void)hipFree(rdict);
        return fail(CGAMD_ERR_HIP, std::string("build_row_codes: ") + hipGetErrorString(e));
    }
    *rcodes_out = rcodes; *rdict_out = rdict; *n_patterns = h[0];
    *n_user_patterns = h[0] - ((n > n_user && !h[2]) ? 1 : 0);
    return CGAMD_OK;
}
// *rcodes_out (n + 64 bytes) and *rdict_out (row_dict_alloc_bytes: values [256][8] | byte offsets [256][8] | lengths [256] | joint codes [256][8]) are device
// allocations the caller frees; both null when the rows have more than 256 patterns.  n rows of which the first n_user are the
// caller's: *n_patterns counts the dictionary entries (what the kernel stages), *n_user_patterns the patterns of the caller's rows
// (one fewer where only the appended rows are empty).  The caller has checked that no row is longer than 7 entries.  Synchronises `st`.
int build_row_codes(int dtype, int n, int n_user, const int *ptr_dev, const unsigned char *jcodes, const int *joff, const void *jval, hipStream_t st,
                    unsigned char **rcodes_out, void **rdict_out, int *n_patterns, int *n_user_patterns) {
    *rcodes_out = nullptr; *rdict_out = nullptr; *n_patterns = 0; *n_user_patterns = 0;
    if (n <= 0 || !jcodes || dtype == CGAMD_C128) return CGAMD_OK;
    if (dtype == CGAMD_F32) return build_row_codes_impl<float>(n, n_user, ptr_dev, jcodes, joff, jval, st, rcodes_out, rdict_out, n_patterns, n_user_patterns);
    if (dtype == CGAMD_F64) return build_row_codes_impl<double>(n, n_user, ptr_dev, jcodes, joff, jval, st, rcodes_out, rdict_out, n_patterns, n_user_patterns);
    return build_row_codes_impl<float2>(n, n_user, ptr_dev, jcodes, joff, jval, st, rcodes_out, rdict_out, n_patterns, n_user_patterns);
}

// -------------------------------------------------------------------------------------------------
// REFRESH: the matrix values changed in place on the same pattern (cgamd_solver_refresh_values).  Where every equal-value class of
// the old matrix is still one (a constant-coefficient operator with rescaled coefficients: new tau in I + tau L, a new wavenumber),
// the code ARRAYS are still right and only the dictionaries are stale.  One pass over vals and vcodes decides it: the first non-zero
// of a class claims the class's new value bits in a 256-entry table (compare-and-swap on the bits; kVEmpty = unclaimed, and a matrix
// that holds that NaN pattern is not coded, as for the builder), every other one compares against the claim, a mismatch raises the
// flag.  Values are compared as bits (-0.0 and +0.0 differ).  A work-group keeps the claims it has seen in LDS, so the table in
// memory is touched once per (work-group, class).  With the flag clear one work-group rewrites vdict from the table, jdict_val from
// vdict (joint code -> value code) and the values of rdict from jdict_val (pattern slot -> joint code), all IN PLACE: no pointer a
// captured graph holds changes.  Classes that now hold equal values keep their codes; the products are formed from the same bits.
// -------------------------------------------------------------------------------------------------
CG_DEV void refresh_claim(unsigned long long key, unsigned code, unsigned long long *stab, unsigned long long *table, int *flag) {
    unsigned long long cur = __hip_atomic_load(stab + code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == key && key != kVEmpty) return;
    if (key != kVEmpty && cur == kVEmpty) {             // not seen by this work-group yet: claim, or read the claim
        cur = __hip_atomic_load(table + code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kVEmpty) {
            cur = atomicCAS(table + code, kVEmpty, key);
            if (cur == kVEmpty) cur = key;
        }
        __hip_atomic_store(stab + code, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == key) return;
    }
    atomicExch(flag, 1);                                // the class split (or the matrix holds the pattern the builder refuses)
}
// vals is 16-byte aligned: value codes are built for plan.kind == 5 only (value_codes_apply in solver.cpp / dist.cpp), and
// finalize_spmv_plan chooses that kind only for 16-byte aligned aValues and aCols, so no handle carries value codes of an unaligned
// array (refresh_value_dicts still checks, and answers "rebuild").  One 16-byte load of E = 16 / sizeof(T) values and one E-byte load
// of their codes per step; the nnz % E last non-zeros go one by one
template <typename T>
__global__ __launch_bounds__(256) void refresh_check_kernel(long long nnz, const T *__restrict__ vals, const unsigned char *__restrict__ vcodes,
                                                            unsigned long long *table, int *flag) {
    __shared__ unsigned long long stab[256];
    stab[threadIdx.x] = __hip_atomic_load(table + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    constexpr int E = (int)(16 / sizeof(T));
    const long long packs = nnz / E, stride = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < packs; p += stride) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const uint4 w = *reinterpret_cast<const uint4 *>(vals + p * E);
        if constexpr (sizeof(T) == 4) {
            unsigned c;
            __builtin_memcpy(&c, vcodes + p * 4, 4);       // (vcodes is an allocation of its own: p * 4 is 4-byte aligned)
            refresh_claim(w.x, c & 255, stab, table, flag);
            refresh_claim(w.y, (c >> 8) & 255, stab, table, flag);
            refresh_claim(w.z, (c >> 16) & 255, stab, table, flag);
            refresh_claim(w.w, c >> 24, stab, table, flag);
        } else {
            unsigned short c;
            __builtin_memcpy(&c, vcodes + p * 2, 2);
            refresh_claim(((unsigned long long)w.y << 32) | w.x, c & 255u, stab, table, flag);
            refresh_claim(((unsigned long long)w.w << 32) | w.z, c >> 8, stab, table, flag);
        }
    }
    const long long j = packs * E + threadIdx.x;
    if (blockIdx.x == 0 && j < nnz) refresh_claim(value_key(vals[j]), vcodes[j], stab, table, flag);
}
// one work-group.  jmap: joint code -> value code [n_pairs]; rlen / rjmap: pattern lengths and pattern slot -> joint code
template <typename T>
__global__ __launch_bounds__(256) void refresh_dicts_kernel(const unsigned long long *__restrict__ table, T *vdict, int n_pairs, const int *__restrict__ jmap,
                                                            T *jval, int n_patterns, const int *__restrict__ rlen,
                                                            const unsigned char *__restrict__ rjmap, T *rval) {
    __shared__ T sv[256], sj[256];
    const int t = threadIdx.x;
    const unsigned long long key = table[t];
    T v = vdict[t];                                     // (codes no non-zero carries keep their entry)
    if (key != kVEmpty) {
        if constexpr (sizeof(T) == 4) { const unsigned b = (unsigned)key; __builtin_memcpy(&v, &b, 4); }
        else __builtin_memcpy(&v, &key, 8);
        vdict[t] = v;
    }
    sv[t] = v;
    __syncthreads();
    if (!jval) return;
    if (t < n_pairs) { sj[t] = sv[jmap[t] & 255]; jval[t] = sj[t]; }
    __syncthreads();
    if (!rval) return;
    for (int p = t; p < n_patterns * 8; p += 256)
        if ((p & 7) < rlen[p >> 3]) rval[p] = sj[rjmap[p]];
}
template <typename T>
static int refresh_value_dicts_impl(long long nnz, const void *vals, const unsigned char *vcodes, void *vdict, int n_pairs, const int *joff, void *jval,
                                    int n_patterns, void *rdict, hipStream_t st, bool *kept) {
    char *scratch = nullptr;
    const size_t tb = sizeof(unsigned long long) * 256;
    CG_HIP(hipMalloc((void **)&scratch, tb + 16));
    auto *table = reinterpret_cast<unsigned long long *>(scratch);
    int *flag = reinterpret_cast<int *>(scratch + tb);
    int h = 1;
    hipError_t e = hipMemsetAsync(table, 0xff, tb, st);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, 16, st);
    const long long packs = nnz / (long long)(16 / sizeof(T));
    const int grid = (int)std::max<long long>(1, std::min<long long>((packs + 255) / 256, kMaxGrid));
    if (e == hipSuccess) {
        hipLaunchKernelGGL((refresh_check_kernel<T>), dim3(grid), dim3(256), 0, st, nnz, static_cast<const T *>(vals), vcodes, table, flag);
        e = hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h == 0) {
        char *rd = static_cast<char *>(rdict);
        hipLaunchKernelGGL((refresh_dicts_kernel<T>), dim3(1), dim3(256), 0, st, table, static_cast<T *>(vdict), n_pairs, joff ? joff + 256 : nullptr,
                           static_cast<T *>(jval), n_patterns, rd ? reinterpret_cast<const int *>(rd + row_dict_len_at(sizeof(T))) : nullptr,
                           rd ? reinterpret_cast<const unsigned char *>(rd + row_dict_jmap_at(sizeof(T))) : nullptr, reinterpret_cast<T *>(rd));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(scratch);
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("refresh_value_dicts: ") + hipGetErrorString(e));
    *kept = h == 0;
    return CGAMD_OK;
}
// vals [nnz] against the value codes made from the array's earlier contents: *kept = every class still holds one value, and the
// dictionaries (vdict; jdict_val behind joff, rdict where the handle has them, else null / 0) now hold the new values.  *kept false:
// nothing was written, the caller rebuilds the codes.  Synchronises `st`.
int refresh_value_dicts(int dtype, long long nnz, const void *vals_dev, const unsigned char *vcodes, void *vdict, int n_pairs, const int *joff,
                        void *jval, int n_patterns, void *rdict, hipStream_t st, bool *kept) {
    *kept = false;
    if (nnz <= 0 || !vcodes || !vdict || dtype == CGAMD_C128 || !aligned16(vals_dev)) return CGAMD_OK;
    if (!joff || !jval) { joff = nullptr; jval = nullptr; rdict = nullptr; }
    if (dtype == CGAMD_F32) return refresh_value_dicts_impl<float>(nnz, vals_dev, vcodes, vdict, n_pairs, joff, jval, n_patterns, rdict, st, kept);
    if (dtype == CGAMD_F64) return refresh_value_dicts_impl<double>(nnz, vals_dev, vcodes, vdict, n_pairs, joff, jval, n_patterns, rdict, st, kept);
    return refresh_value_dicts_impl<float2>(nnz, vals_dev, vcodes, vdict, n_pairs, joff, jval, n_patterns, rdict, st, kept);
}

// -------------------------------------------------------------------------------------------------
// ROW-PAIR codes: rows 2p and 2p + 1 of a stencil matrix almost always carry the same pattern, and for a slot of offset o row 2p needs
// x[2p + o] and row 2p + 1 needs x[2p + 1 + o] -- the two halves of ONE 16-byte load.  One byte per pair names a PAIR pattern: the
// union of the two rows' slots (merge_pair_slots, row_pairs.cpp), at most 8 of them, with the value either row multiplies and a mask
// of the slots either row uses.  Passes: mark the (rcodes[2p], rcodes[2p + 1]) combinations that occur (the partner of a lone last
// row is the empty pattern kPairEmpty, whether the dictionary holds one or not), read the marks and the row dictionary back, number
// the combinations ascending and merge them on the HOST (at most 256 patterns of at most 7 slots), upload, encode.
// -------------------------------------------------------------------------------------------------
constexpr int kPairEmpty = 256;
constexpr int kPairCombos = 256 * 257;
__global__ __launch_bounds__(256) void rowpair_mark_kernel(int n, const unsigned char *__restrict__ rcodes, unsigned char *present) {
    const long long npairs = ((long long)n + 1) / 2, stride = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npairs; p += stride) {
        const int c0 = rcodes[2 * p], c1 = 2 * p + 1 < n ? (int)rcodes[2 * p + 1] : kPairEmpty;
        if (!present[c0 * 257 + c1]) present[c0 * 257 + c1] = 1;
    }
}
__global__ __launch_bounds__(256) void rowpair_encode_kernel(int n, const unsigned char *__restrict__ rcodes, const unsigned char *__restrict__ combo_code,
                                                             unsigned char *__restrict__ pcodes) {
    const long long npairs = ((long long)n + 1) / 2, stride = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npairs; p += stride) {
        const int c0 = rcodes[2 * p], c1 = 2 * p + 1 < n ? (int)rcodes[2 * p + 1] : kPairEmpty;
        pcodes[p] = combo_code[c0 * 257 + c1];
    }
}
// W: a value as bits (4 or 8 bytes).  src [np][16]: where in rval the value of (pair pattern, row of the pair, union slot) came from
template <typename W>
__global__ __launch_bounds__(256) void rowpair_values_kernel(int np, const W *__restrict__ rval, const unsigned short *__restrict__ src, W *val0, W *val1) {
    for (int k = threadIdx.x; k < np * 16; k += 256) {
        const int p = k >> 4, u = k & 7;
        const unsigned s = src[k];
        const W v = s == 0xffffu ? (W)0 : rval[s];
        ((k & 8) ? val1 : val0)[p * 8 + u] = v;
    }
}
static void launch_rowpair_values(size_t vs, int np, const void *rdict, char *pdict, hipStream_t st) {
    const auto *src = reinterpret_cast<const unsigned short *>(pdict + pair_dict_src_at(np, vs));
    if (vs == 4)
        hipLaunchKernelGGL((rowpair_values_kernel<unsigned>), dim3(1), dim3(256), 0, st, np, static_cast<const unsigned *>(rdict), src,
                           reinterpret_cast<unsigned *>(pdict), reinterpret_cast<unsigned *>(pdict + pair_dict_val1_at(np, vs)));
    else
        hipLaunchKernelGGL((rowpair_values_kernel<unsigned long long>), dim3(1), dim3(256), 0, st, np, static_cast<const unsigned long long *>(rdict), src,
                           reinterpret_cast<unsigned long long *>(pdict), reinterpret_cast<unsigned long long *>(pdict + pair_dict_val1_at(np, vs)));
}
int build_row_pairs(int dtype, int n, const unsigned char *rcodes, const void *rdict, int n_patterns, hipStream_t st,
                    unsigned char **pcodes_out, void **pdict_out, int *n_pair_patterns, int *max_slots) {
    *pcodes_out = nullptr; *pdict_out = nullptr; *n_pair_patterns = 0; *max_slots = 0;
    if (n < 2 || !rcodes || !rdict || n_patterns < 1 || dtype == CGAMD_C128) return CGAMD_OK;
    const size_t vs = dtype_size(dtype);
    unsigned char *marks = nullptr;         // present [kPairCombos], then the code of every combination [kPairCombos]
    CG_HIP(hipMalloc((void **)&marks, 2 * (size_t)kPairCombos));
    std::vector<unsigned char> present(kPairCombos), combo_code(kPairCombos, 0);
    std::vector<int> roff(256 * 8), rlen(256);
    const int grid = (int)std::min<long long>((((long long)n + 1) / 2 + 255) / 256, 4096);
    hipError_t e = hipMemsetAsync(marks, 0, kPairCombos, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rowpair_mark_kernel, dim3(grid), dim3(256), 0, st, n, rcodes, marks);
        e = hipMemcpyAsync(present.data(), marks, kPairCombos, hipMemcpyDeviceToHost, st);
    }
    const char *rd = static_cast<const char *>(rdict);
    if (e == hipSuccess) e = hipMemcpyAsync(roff.data(), rd + row_dict_off_at(vs), 256 * 8 * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(rlen.data(), rd + row_dict_len_at(vs), 256 * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // number the combinations that occur, ascending, and merge each
    std::vector<PairPattern> pats;
    std::vector<int> combos;
    bool fits = e == hipSuccess;
    for (int c = 0; fits && c < kPairCombos; ++c) {
        if (!present[c]) continue;
        const int c0 = c / 257, c1 = c % 257;
        if (pats.size() == 256 || c0 >= n_patterns || (c1 != kPairEmpty && c1 >= n_patterns)) { fits = false; break; }
        const int len0 = rlen[c0], len1 = c1 == kPairEmpty ? 0 : rlen[c1];
        PairPattern pp;
        if (!merge_pair_slots(len0, &roff[c0 * 8], len1, c1 == kPairEmpty ? nullptr : &roff[c1 * 8], &pp)) { fits = false; break; }
        combo_code[c] = (unsigned char)pats.size();
        pats.push_back(pp);
        combos.push_back(c);
    }
    const int np = (int)pats.size();
    if (fits && (np < 1 || pair_dict_stage_bytes(np, vs) > kPairDictLdsCap)) fits = false;
    unsigned char *pcodes = nullptr;
    char *pdict = nullptr;
    int slots = 0;
    for (const PairPattern &pp : pats) slots = std::max(slots, pp.n);
    if (fits) {
        std::vector<char> img(pair_dict_alloc_bytes(np, vs), 0);
        int *off = reinterpret_cast<int *>(img.data() + pair_dict_off_at(np, vs));
        int *mask = reinterpret_cast<int *>(img.data() + pair_dict_mask_at(np, vs));
        auto *src = reinterpret_cast<unsigned short *>(img.data() + pair_dict_src_at(np, vs));
        for (int p = 0; p < np; ++p) {
            const int c0 = combos[p] / 257, c1 = combos[p] % 257;
            int m = 0;
            for (int u = 0; u < kPairSlots; ++u) {
                const PairPattern &pp = pats[p];
                off[p * 8 + u] = u < pp.n ? pp.off[u] : 0;
                const bool use0 = u < pp.n && pp.src0[u] >= 0, use1 = u < pp.n && pp.src1[u] >= 0;
                src[p * 16 + u] = use0 ? (unsigned short)(c0 * 8 + pp.src0[u]) : (unsigned short)0xffffu;
                src[p * 16 + 8 + u] = use1 ? (unsigned short)(c1 * 8 + pp.src1[u]) : (unsigned short)0xffffu;
                m |= (use0 ? 1 << u : 0) | (use1 ? 256 << u : 0);
            }
            mask[p] = m;
        }
        e = hipMalloc((void **)&pcodes, ((size_t)n + 1) / 2 + 64);
        if (e == hipSuccess) e = hipMalloc((void **)&pdict, img.size());
        if (e == hipSuccess) e = hipMemsetAsync(pcodes + ((size_t)n + 1) / 2, 0, 64, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pdict, img.data(), img.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(marks + kPairCombos, combo_code.data(), kPairCombos, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            launch_rowpair_values(vs, np, rdict, pdict, st);
            hipLaunchKernelGGL(rowpair_encode_kernel, dim3(grid), dim3(256), 0, st, n, rcodes, marks + kPairCombos, pcodes);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);      // (img and combo_code go away)
    }
    (void)hipFree(marks);
    if (e != hipSuccess) {
        if (pcodes) (void)hipFree(pcodes);
        if (pdict) (void)hipFree(pdict);
        return fail(CGAMD_ERR_HIP, std::string("build_row_pairs: ") + hipGetErrorString(e));
    }
    *pcodes_out = pcodes; *pdict_out = pdict; *n_pair_patterns = fits ? np : 0;
    if (fits) *max_slots = slots;
    return CGAMD_OK;
}
int refresh_pair_dict(int dtype, int n_pair_patterns, const void *rdict, void *pdict, hipStream_t st) {
    if (!rdict || !pdict || n_pair_patterns < 1 || dtype == CGAMD_C128) return CGAMD_OK;
    launch_rowpair_values(dtype_size(dtype), n_pair_patterns, rdict, static_cast<char *>(pdict), st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("refresh_pair_dict: ") + hipGetErrorString(e));
    return CGAMD_OK;
}

}  // namespace cgamd
