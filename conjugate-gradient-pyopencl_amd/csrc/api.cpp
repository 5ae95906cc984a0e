// C ABI: context, memory helpers, the five stand-alone kernels, generators, legacy cg()/connect().
// The ABI mirrors the reference's Python operator surface (cl.py:16-42) and C entry (clcg.h:3-5).
#include <atomic>
#include <pthread.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clcg.h"
#include "cgamd_internal.h"

namespace cgamd {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(int status, const std::string &msg) {
    g_err = msg;
    return status;
}
}  // namespace cgamd
using namespace cgamd;

extern "C" {

const char *cgamd_last_error(void) { return g_err.c_str(); }
int cgamd_version(void) { return 100; }
size_t cgamd_dtype_size(int dtype) { return dtype_size(dtype); }

static std::atomic<unsigned long long> g_tune_generation{1};     // bumped by every cgamd_tune: cached cg() handles carry the one they were made under

int cgamd_tune(const char *key, int value) {
    if (!key) return fail(CGAMD_ERR_INVALID, "tune: null key");
    const std::string k(key);
    bool known = true;
    if (k == "dev.x_lag" && value != -1 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
        return fail(CGAMD_ERR_INVALID, "tune: dev.x_lag takes -1 (default rule), 0 or 1 (off), 2, 4 or 8");
    if (k == "dev.row_pipe" && value != 0 && value != 1 && value != 2 && value != 4)
        return fail(CGAMD_ERR_INVALID, "tune: dev.row_pipe takes 0 (default rule), 1, 2 or 4");
    if (k == "dev.row_pairs" && value != -1 && value != 0 && value != 1)
        return fail(CGAMD_ERR_INVALID, "tune: dev.row_pairs takes -1 (default rule), 0 or 1");
    if (k == "dev.long_row_bytes" && value < 0) return fail(CGAMD_ERR_INVALID, "tune: dev.long_row_bytes takes 0 (the rule) or a byte count");
    if (k == "dev.long_row_segment" && (value < 0 || (value & 3)))
        return fail(CGAMD_ERR_INVALID, "tune: dev.long_row_segment takes 0 (default) or a multiple of 4 entries");
    if (k == "dev.spmv_plane" && value != -1 && value != 0 && value != 1)
        return fail(CGAMD_ERR_INVALID, "tune: dev.spmv_plane takes -1 (default rule), 0 or 1");
    g_tune_generation.fetch_add(1, std::memory_order_relaxed);     // cached cg() handles were created under the old configuration
    tune_set([&](Tuning &g_tune) {
    // public keys (include/cgamd.h)
    if (k == "index_codes") g_tune.index_codes = value;
    else if (k == "index_codes16") g_tune.index_codes16 = value;
    else if (k == "index_codes_min_mb") g_tune.index_codes_min_mb = value;
    else if (k == "resident") g_tune.resident = value;
    else if (k == "resident_min") g_tune.resident_min = value;
    else if (k == "resident_wide") g_tune.resident_wide = value;
    else if (k == "resident_wide_min") g_tune.resident_wide_min = value;
    else if (k == "resident_claim_ms") g_tune.resident_claim_ms = value;
    else if (k == "two_launch") g_tune.two_launch = value;
    else if (k == "spmm_rowmajor") g_tune.spmm_rowmajor = value;
    else if (k == "pad_rows") g_tune.pad_rows = value;
    else if (k == "spmv_nt") g_tune.spmv_nt = value;
    else if (k == "vec_nt") g_tune.vec_nt = value;
    else if (k == "spmv_cycle") g_tune.spmv_cycle = value;
    else if (k == "vec_grid") g_tune.vec_grid = value;
    // development hooks: tests, rehearsals, profiling (not part of the documented interface)
    else if (k == "dev.no_fold_alpha") g_tune.dev_no_fold_alpha = value;
    else if (k == "dev.x_lag") g_tune.dev_x_lag = value;
    else if (k == "dev.x_lag_dnt") g_tune.dev_x_lag_dnt = value;
    else if (k == "dev.generic_spmv") g_tune.dev_generic_spmv = value;
    else if (k == "dev.long_row_bytes") g_tune.dev_long_row_bytes = value;
    else if (k == "dev.long_row_segment") g_tune.dev_long_row_segment = value;
    else if (k == "dev.value_codes") g_tune.value_codes = value;
    else if (k == "dev.vc_pipe") g_tune.dev_vc_pipe = value;
    else if (k == "dev.joint_codes") g_tune.dev_joint_codes = value;
    else if (k == "dev.row_codes") g_tune.dev_row_codes = value;
    else if (k == "dev.row_codes_min_mb") g_tune.dev_row_codes_min_mb = value;
    else if (k == "dev.row_pipe") g_tune.dev_row_pipe = value;
    else if (k == "dev.row_pairs") g_tune.dev_row_pairs = value;
    else if (k == "dev.row_pairs_min_mb") g_tune.dev_row_pairs_min_mb = value;
    else if (k == "dev.spmv_plane") g_tune.dev_spmv_plane = value;
    else if (k == "dev.resident_lock") g_tune.resident_lock = value;
    else if (k == "dev.slab_cus") g_tune.slab_cus = value;
    else if (k == "dev.slab_trim") g_tune.slab_trim = value;
    else if (k == "dev.resident_test_short_grid") g_tune.resident_test_short_grid = value;
    else if (k == "dev.resident_wide_rpt") g_tune.resident_wide_rpt = value;
    else if (k == "dev.resident_window") g_tune.resident_window = value;
    else if (k == "dev.vec_ppt") g_tune.vec_ppt = value;
    else if (k == "dev.spmv_unroll") g_tune.spmv_unroll = value;
    else if (k == "dev.spmv_grid") g_tune.spmv_grid = value;
    else if (k == "dev.spmv_slice_kb") g_tune.spmv_slice_kb = value;
    else if (k == "dev.spmv_chunk_kb") g_tune.spmv_chunk_kb = value;
    else if (k == "dev.spmv_chunked") g_tune.spmv_chunked = value;
    else if (k == "dev.spmm_ynt") g_tune.spmm_ynt = value;
    else if (k == "dev.spmm_group") g_tune.spmm_group = value;
    else if (k == "dev.spmm_rb") g_tune.spmm_rb = value;
    else if (k == "dev.spmm_wgs") g_tune.spmm_wgs = value;
    else if (k == "dev.spmm_lead") g_tune.spmm_lead = value;
    else if (k == "dev.spmm_wide_max") g_tune.spmm_wide_max = value;
    else if (k == "dev.line_host_route") g_tune.dev_line_host_route = value;
    else known = false;
    });
    if (!known) return fail(CGAMD_ERR_INVALID, "tune: unknown key " + k);
    return CGAMD_OK;
}

int cgamd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        fail(CGAMD_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
        return -CGAMD_ERR_NO_DEVICE;
    }
    return n;
}

int cgamd_device_name(int device, char *buf, size_t buflen) {
    if (!buf || !buflen) return fail(CGAMD_ERR_INVALID, "device_name: null buffer");
    hipDeviceProp_t p;
    CG_HIP(hipGetDeviceProperties(&p, device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return CGAMD_OK;
}

int cgamd_ctx_create(int device, cgamd_ctx **out) {
    if (!out) return fail(CGAMD_ERR_INVALID, "ctx_create: out is NULL");
    *out = nullptr;
    int n = cgamd_device_count();
    if (n <= 0) return fail(CGAMD_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    thread_hip_setup();
    if (device < 0 || device >= n) return fail(CGAMD_ERR_INVALID, "ctx_create: device index out of range");
    CG_HIP(hipSetDevice(device));
    cgamd_ctx *c = new cgamd_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(CGAMD_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    c->own_stream = true;
    *out = c;
    return CGAMD_OK;
}

int cgamd_ctx_destroy(cgamd_ctx *c) {
    if (!c) return CGAMD_OK;
    (void)hipSetDevice(c->device);
    if (c->partials) (void)hipFree(c->partials);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return CGAMD_OK;
}

int cgamd_ctx_set_stream(cgamd_ctx *c, void *stream) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    if (c->own_stream && c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
    }
    c->own_stream = false;
    c->stream = static_cast<hipStream_t>(stream);
    return CGAMD_OK;
}
void *cgamd_ctx_stream(cgamd_ctx *c) { return c ? (void *)c->stream : nullptr; }
int cgamd_ctx_device(cgamd_ctx *c) { return c ? c->device : -1; }
int cgamd_ctx_synchronize(cgamd_ctx *c) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(c->device));
    CG_HIP(hipStreamSynchronize(c->stream));
    return CGAMD_OK;
}

int cgamd_malloc(cgamd_ctx *c, size_t bytes, void **dptr) {
    if (!c || !dptr) return fail(CGAMD_ERR_INVALID, "malloc: null argument");
    thread_hip_setup();
    CG_HIP(hipSetDevice(c->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    return CGAMD_OK;
}
int cgamd_free(cgamd_ctx *c, void *dptr) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(c->device));
    if (dptr) CG_HIP(hipFree(dptr));
    return CGAMD_OK;
}
int cgamd_memcpy_h2d(cgamd_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(c->device));
    CG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    CG_HIP(hipStreamSynchronize(c->stream));
    return CGAMD_OK;
}
int cgamd_memcpy_d2h(cgamd_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(c->device));
    CG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    CG_HIP(hipStreamSynchronize(c->stream));
    return CGAMD_OK;
}
int cgamd_memcpy_d2d(cgamd_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    CG_HIP(hipSetDevice(c->device));
    CG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return CGAMD_OK;
}
int cgamd_memset(cgamd_ctx *c, void *dst, int value, size_t bytes) {
    if (!c) return fail(CGAMD_ERR_INVALID, "ctx is NULL");
    CG_HIP(hipSetDevice(c->device));
    CG_HIP(hipMemsetAsync(dst, value, bytes, c->stream));
    return CGAMD_OK;
}

// ---- stand-alone ops ---------------------------------------------------------------------------
static int check_op(cgamd_ctx *c, int dtype, int size, int nRHS, const char *what) {
    if (!c) return fail(CGAMD_ERR_INVALID, std::string(what) + ": ctx is NULL");
    if (dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, std::string(what) + ": bad dtype");
    if (size < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, std::string(what) + ": bad size/nRHS");
    thread_hip_setup();
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(CGAMD_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return CGAMD_OK;
}

int cgamd_spmv(cgamd_ctx *c, int dtype, int size, long long nnz, const void *aValues, const int *aPointers,
               const int *aCols, const void *x, void *y, int nRHS) {
    if (int rc = check_op(c, dtype, size, nRHS, "spmv")) return rc;
    if (size == 0) return CGAMD_OK;
    if (!aPointers || !x || !y || (nnz > 0 && (!aValues || !aCols))) return fail(CGAMD_ERR_INVALID, "spmv: null pointer");
    const SpmvPlan plan = make_spmv_plan(size);
    return launch_spmv(dtype, plan, size, nnz, aValues, aPointers, aCols, x, size, y, size, nRHS, nullptr, nullptr, c->stream);
}

static int ensure_partials(cgamd_ctx *c, size_t bytes) {
    if (c->partials_bytes >= bytes) return CGAMD_OK;
    if (c->partials) {
        CG_HIP(hipStreamSynchronize(c->stream));
        CG_HIP(hipFree(c->partials));
        c->partials = nullptr;
        c->partials_bytes = 0;
    }
    hipError_t e = hipMalloc(&c->partials, bytes);
    if (e != hipSuccess) return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(partials): ") + hipGetErrorString(e));
    c->partials_bytes = bytes;
    return CGAMD_OK;
}

int cgamd_vdot(cgamd_ctx *c, int dtype, int size, const void *a, const void *b, void *result, int nRHS) {
    if (int rc = check_op(c, dtype, size, nRHS, "vdot")) return rc;
    if (!result || (size > 0 && (!a || !b))) return fail(CGAMD_ERR_INVALID, "vdot: null pointer");
    const int grid = vec_grid(size, dtype);
    if (int rc = ensure_partials(c, acc_size(dtype) * (size_t)grid * nRHS)) return rc;
    if (int rc = launch_dot_partials(dtype, size, a, b, size, nRHS, c->partials, grid, c->stream)) return rc;
    return launch_reduce_to_value(dtype, c->partials, grid, nRHS, result, c->stream);
}

int cgamd_axpy(cgamd_ctx *c, int dtype, int size, const void *x, void *y, const void *a, int aSign, int nRHS) {
    if (int rc = check_op(c, dtype, size, nRHS, "axpy")) return rc;
    if (size > 0 && (!x || !y || !a)) return fail(CGAMD_ERR_INVALID, "axpy: null pointer");
    return launch_axpy(dtype, size, x, y, size, a, aSign, nRHS, c->stream);
}
int cgamd_aypx(cgamd_ctx *c, int dtype, int size, const void *x, void *y, const void *a, int nRHS) {
    if (int rc = check_op(c, dtype, size, nRHS, "aypx")) return rc;
    if (size > 0 && (!x || !y || !a)) return fail(CGAMD_ERR_INVALID, "aypx: null pointer");
    return launch_aypx(dtype, size, x, y, size, a, nRHS, c->stream);
}
int cgamd_sub(cgamd_ctx *c, int dtype, int size, const void *a, const void *b, void *result, int nRHS) {
    if (int rc = check_op(c, dtype, size, nRHS, "sub")) return rc;
    if (size > 0 && (!a || !b || !result)) return fail(CGAMD_ERR_INVALID, "sub: null pointer");
    return launch_sub(dtype, size, a, b, result, size, nRHS, c->stream);
}

int cgamd_transpose(cgamd_ctx *c, int dtype, int rows, int cols, const void *in, void *out) {
    if (int rc = check_op(c, dtype, rows, 1, "transpose")) return rc;
    if (cols < 0 || ((long long)rows * cols > 0 && (!in || !out || in == out))) return fail(CGAMD_ERR_INVALID, "transpose: bad argument");
    return launch_transpose(dtype, rows, cols, in, out, c->stream);
}

// ---- generators --------------------------------------------------------------------------------
int cgamd_gen_laplace3d(cgamd_ctx *c, int dtype, int nx, int ny, int nz, long long row_begin, long long row_end,
                        void *aValues, int *aPointers, int *aCols, long long *nnz_out) {
    const long long n = (long long)nx * ny * nz;
    if (nx < 1 || ny < 1 || nz < 1 || row_begin < 0 || row_end > n || row_begin > row_end)
        return fail(CGAMD_ERR_INVALID, "gen_laplace3d: bad grid or row range");
    if (n > 2147483647LL) return fail(CGAMD_ERR_INVALID, "gen_laplace3d: more than 2^31-1 columns (int32 column indices)");
    const long long nnz = laplace3d_ptr(row_end, nx, ny, nz) - laplace3d_ptr(row_begin, nx, ny, nz);
    if (nnz_out) *nnz_out = nnz;
    if (!aPointers) return CGAMD_OK;  // size query
    if (nnz > 2147483647LL - 8192) return fail(CGAMD_ERR_INVALID, "gen_laplace3d: slab has more than 2^31 entries");
    if (int rc = check_op(c, dtype, 0, 1, "gen_laplace3d")) return rc;
    if (!aValues || !aCols) return fail(CGAMD_ERR_INVALID, "gen_laplace3d: null pointer");
    return launch_gen_laplace3d(dtype, nx, ny, nz, row_begin, row_end, aValues, aPointers, aCols, c->stream);
}

int cgamd_gen_poisson2d(cgamd_ctx *c, int dtype, int N, void *aValues, int *aPointers, int *aCols, long long *nnz_out) {
    if (N < 1 || (long long)N * N > 400000000LL) return fail(CGAMD_ERR_INVALID, "gen_poisson2d: bad N");
    const long long nnz = poisson2d_ptr((long long)N * N, N);
    if (nnz_out) *nnz_out = nnz;
    if (!aPointers) return CGAMD_OK;
    if (int rc = check_op(c, dtype, 0, 1, "gen_poisson2d")) return rc;
    if (!aValues || !aCols) return fail(CGAMD_ERR_INVALID, "gen_poisson2d: null pointer");
    return launch_gen_poisson2d(dtype, N, aValues, aPointers, aCols, c->stream);
}

static int gen_fe_common(cgamd_ctx *c, int dtype, int variable, int N, double p0, double p1, double p2, double L, const double *C_host, int Nh,
                         int Nv, void *aValues, int *aPointers, int *aCols, long long *nnz_out, const char *what) {
    if (N < 2 || Nh < 2 || Nv < 2 || (long long)Nh * Nv > 200000000LL) return fail(CGAMD_ERR_INVALID, std::string(what) + ": bad N / Nhoriz / Nvert");
    const long long nnz = helm_fe_nnz(Nh, Nv);
    if (nnz_out) *nnz_out = nnz;
    if (!aPointers) return CGAMD_OK;
    if (int rc = check_op(c, dtype, 0, 1, what)) return rc;
    if (!aValues || !aCols) return fail(CGAMD_ERR_INVALID, std::string(what) + ": null pointer");
    if (dtype != CGAMD_C64 && dtype != CGAMD_C128) return fail(CGAMD_ERR_INVALID, std::string(what) + ": the matrix is complex (dtype complex64 or complex128)");
    double *C_dev = nullptr;
    if (variable) {     // wave speed per square on the device (all ones when the caller passes none)
        const size_t count = (size_t)(Nh - 1) * (Nv - 1);
        std::vector<double> ones;
        if (!C_host) { ones.assign(count, 1.0); C_host = ones.data(); }
        for (size_t i = 0; i < count; ++i)
            if (!(C_host[i] != 0.0)) return fail(CGAMD_ERR_INVALID, std::string(what) + ": wave speed C must be non-zero");
        CG_HIP(hipMalloc(&C_dev, count * sizeof(double)));
        hipError_t e = hipMemcpyAsync(C_dev, C_host, count * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);     // `ones` / the caller's array may go away
        if (e != hipSuccess) { (void)hipFree(C_dev); return fail(CGAMD_ERR_HIP, std::string(what) + ": upload of C: " + hipGetErrorString(e)); }
    }
    int rc = launch_gen_helm_fe(dtype, variable, N, p0, p1, p2, L, C_dev, Nh, Nv, aValues, aPointers, aCols, c->stream);
    if (C_dev) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(C_dev);
    }
    return rc;
}

int cgamd_gen_helm_fe_var(cgamd_ctx *c, int dtype, int N, double omega, const double *C, double rho, int Nhoriz, int Nvert, void *aValues,
                          int *aPointers, int *aCols, long long *nnz_out) {
    return gen_fe_common(c, dtype, 1, N, omega, rho, 0.0, 1.0, C, Nhoriz, Nvert, aValues, aPointers, aCols, nnz_out, "gen_helm_fe_var");
}

int cgamd_gen_local_rect(cgamd_ctx *c, int dtype, int N, double k, double eps, double eta, double L, int Nhoriz, int Nvert, void *aValues,
                         int *aPointers, int *aCols, long long *nnz_out) {
    return gen_fe_common(c, dtype, 0, N, k, eps, eta, L, nullptr, Nhoriz, Nvert, aValues, aPointers, aCols, nnz_out, "gen_local_rect");
}

int cgamd_gen_rhs(cgamd_ctx *c, int dtype, int kind, int N, double k, void *b) {
    if (!c || !b) return fail(CGAMD_ERR_INVALID, "gen_rhs: null argument");
    if (dtype < 0 || dtype > 3 || kind < 0 || kind > 2 || N < 2) return fail(CGAMD_ERR_INVALID, "gen_rhs: bad dtype / kind / N");
    if (kind == 0 && dtype != CGAMD_C64 && dtype != CGAMD_C128) return fail(CGAMD_ERR_INVALID, "gen_rhs: rhs(N, k) is complex valued");
    CG_HIP(hipSetDevice(c->device));
    return launch_gen_rhs(dtype, kind, N, k, b, c->stream);
}

// ---- one-call typed solve on host arrays ----------------------------------------------------------
// Stateless towards the caller (matrix, b, x are host arrays alive for the call only; everything is uploaded every time,
// as in the reference clcg.c:202-211), but the DEVICE STATE -- context, stream, allocations, SpMV plan, captured graphs --
// is kept per calling thread and reused when the shape repeats: the reference's caller solves with the same sub-domain
// matrix once per outer GMRES iteration (p_h-PY_C-CL.py:1948-1950), and rebuilding that state costs as much as the 256
// iterations themselves (per-call split).
namespace {
struct CgCache {
    cgamd_ctx *ctx = nullptr;
    cgamd_solver *s = nullptr;
    int dtype = -1, size = 0, nrhs = 0, device = -1;
    long long nnz = -1;
    unsigned long long tune_gen = 0;      // generation of the tuning configuration the handle was created under
    unsigned long long last_use = 0;
    void release() {
        if (s) cgamd_solver_destroy(s);
        if (ctx) cgamd_ctx_destroy(ctx);
        s = nullptr; ctx = nullptr; dtype = -1;
    }
    void forget() { s = nullptr; ctx = nullptr; dtype = -1; }      // after fork(): the child must not touch the parent's HIP handles
};
// A small LRU per calling thread: the reference's as_prec cycles over sub-domains of a few different sizes (p_h-PY_C-CL.py:1918-1953),
// one entry would miss every time.  An entry is reused only under the tuning configuration it was created with.
constexpr int kCgCacheEntries = 4;
struct CgCacheSet {
    CgCache e[kCgCacheEntries];
    unsigned long long clock = 0;
    ~CgCacheSet() { for (auto &c : e) c.release(); }
};
thread_local CgCacheSet t_cg_cache;
std::atomic<unsigned long long> g_fork_generation{0};
thread_local unsigned long long t_fork_seen = 0;
void cg_atfork_child() { g_fork_generation.fetch_add(1, std::memory_order_relaxed); }
void cg_cache_check_fork() {
    static std::once_flag once;
    std::call_once(once, [] { pthread_atfork(nullptr, nullptr, cg_atfork_child); });
    const unsigned long long g = g_fork_generation.load(std::memory_order_relaxed);
    if (g != t_fork_seen) {                // this process is a fork()ed child: the cached device state belongs to the parent
        for (auto &c : t_cg_cache.e) c.forget();
        t_fork_seen = g;
    }
}
thread_local double t_cg_timing[6] = {0, 0, 0, 0, 0, 0};
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

int cgamd_cg_release_cache(void) {
    cg_cache_check_fork();
    for (auto &c : t_cg_cache.e) c.release();
    return CGAMD_OK;
}
int cgamd_cg_last_timing(double *ms6) {
    if (!ms6) return fail(CGAMD_ERR_INVALID, "cg_last_timing: null argument");
    for (int i = 0; i < 6; ++i) ms6[i] = t_cg_timing[i];
    return CGAMD_OK;
}

int cgamd_cg(int dtype, int size, long long nnz, const void *aValues, const void *b, const int *aPointers,
             const int *aCols, void *x, int nRHS, int nIterations, void *history, int device) {
    if (size < 0 || nnz < 0 || nRHS < 1 || nIterations < 0) return fail(CGAMD_ERR_INVALID, "cg: bad size argument");
    if (size == 0) return CGAMD_OK;
    if (!aPointers || !b || !x || (nnz > 0 && (!aValues || !aCols))) return fail(CGAMD_ERR_INVALID, "cg: null pointer");
    static const bool no_cache = [] { const char *e = getenv("CGAMD_CG_NO_CACHE"); return e && e[0] == '1'; }();
    cg_cache_check_fork();
    const unsigned long long tgen = g_tune_generation.load(std::memory_order_relaxed);
    CgCache local;
    CgCache *pick = &local;
    if (!no_cache) {        // the entry of this shape (under today's tuning), else the least recently used one
        CgCacheSet &set = t_cg_cache;
        pick = &set.e[0];
        for (auto &e : set.e)
            if (e.s && e.dtype == dtype && e.size == size && e.nnz == nnz && e.nrhs == nRHS && e.device == device && e.tune_gen == tgen) { pick = &e; break; }
            else if (e.last_use < pick->last_use) pick = &e;
        pick->last_use = ++set.clock;
    }
    CgCache &c = *pick;
    double t[6];
    t[0] = now_ms();
    const bool hit = c.s && c.dtype == dtype && c.size == size && c.nnz == nnz && c.nrhs == nRHS && c.device == device && c.tune_gen == tgen;
    int rc = CGAMD_OK;
    double t_upload = 0.0;
    if (hit) {
        const double u0 = now_ms();
        rc = cgamd_solver_reload_matrix(c.s, aValues, aPointers, aCols);
        t_upload = now_ms() - u0;
    } else {
        c.release();
        rc = cgamd_ctx_create(device, &c.ctx);
        // creation uploads the matrix as part of building the handle: not separable, all of it is counted as device state
        if (rc == CGAMD_OK) rc = cgamd_solver_create(c.ctx, dtype, size, nnz, aValues, aPointers, aCols, nRHS, 0, &c.s);
        if (rc == CGAMD_OK) { c.dtype = dtype; c.size = size; c.nnz = nnz; c.nrhs = nRHS; c.device = device; c.tune_gen = tgen; }
    }
    t[1] = now_ms();
    if (rc == CGAMD_OK) rc = cgamd_solver_set_rhs(c.s, b, x, 0);      // x is in/out: initial guess (clcg.c:210)
    t[2] = now_ms();
    if (rc == CGAMD_OK) rc = cgamd_solver_iterate(c.s, nIterations);
    if (rc == CGAMD_OK) rc = cgamd_ctx_synchronize(c.ctx);
    t[3] = now_ms();
    if (rc == CGAMD_OK) rc = cgamd_solver_get_x(c.s, x, 0);
    if (rc == CGAMD_OK && history) {
        const int got = cgamd_solver_history(c.s, history, nIterations + 1);
        if (got < 0) rc = -got;
    }
    t[4] = now_ms();
    t_cg_timing[0] = t[1] - t[0] - t_upload; t_cg_timing[1] = t_upload; t_cg_timing[2] = t[2] - t[1];
    t_cg_timing[3] = t[3] - t[2]; t_cg_timing[4] = t[4] - t[3]; t_cg_timing[5] = hit ? 1.0 : 0.0;
    if (rc != CGAMD_OK || no_cache) {       // never keep a handle in an unknown state (CGAMD_CG_NO_CACHE: never keep one at all)
        std::string keep = g_err;
        c.release();
        g_err = keep;
    }
    return rc;
}

// ---- legacy ABI (reference clcg.h:3-5) ------------------------------------------------------------
float *cg(int size, int nonZeros, const float *aValues, const float *b, const int *aPointers, const int *aCols,
          float *x, int nRHS, int nIterations, int isComplex) {
    const int rc = cgamd_cg(isComplex ? CGAMD_C64 : CGAMD_F32, size, nonZeros, aValues, b, aPointers, aCols, x, nRHS,
                            nIterations, nullptr, 0);
    if (rc != CGAMD_OK)  // the reference prints and carries on (clcg.c:52-56); x is left as passed in
        fprintf(stderr, "error -- cg (MI355X/HIP) failed with status %d: %s\n", rc, cgamd_last_error());
    return x;
}

}  // extern "C"
