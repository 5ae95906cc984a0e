// Setup of the preconditioners, shared by the single-GPU handle (solver.cpp) and the row-partitioned one (dist.cpp): factoring and
// planning a tridiagonal M on the host from its three arrays, and building the line / Jacobi preconditioners on the device from a
// CSR matrix (precond_build.hip).  Nothing here knows a handle: the callers pass the stream, the sizes and the matrix and get device
// allocations back (TriBuilt), which they install.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "cgamd_internal.h"

namespace cgamd {


void tri_built_free(TriBuilt *b) {
    if (b->coef) (void)hipFree(b->coef);
    if (b->plan) (void)hipFree(b->plan);
    *b = TriBuilt();
}

// The host side both tridiagonal forms share: M's three arrays to the host and the factorisation along every chain c, c + stride,
// c + 2 stride, ... (stride 1: the rows in order).  Rows are visited in order, so the first bad row is the one named.  Leaves the
// factors as the kernels read them (nl, ne, w: `pitch` values each) and, per row, whether the stored -l / -w c are 0.
struct TriFactors {
    std::vector<unsigned char> coef;
    std::vector<char> l_zero, e_zero;
    size_t pitch = 0;
};
static int tri_factor(hipStream_t st, int dt, int nu, int n, const std::string &who, int stride, const void *lower, const void *diag,
                      const void *upper, int on_device, TriFactors &out) {
    const size_t vs = dtype_size(dt);
    std::vector<unsigned char> h[3];
    const void *src[3] = {lower, diag, upper};
    for (int k = 0; k < 3; ++k) {
        h[k].resize((size_t)nu * vs);
        if (on_device) CG_HIP(hipMemcpyAsync(h[k].data(), src[k], h[k].size(), hipMemcpyDeviceToHost, st));
        else std::memcpy(h[k].data(), src[k], h[k].size());
    }
    if (on_device) CG_HIP(hipStreamSynchronize(st));
    using C = std::complex<double>;
    auto get = [&](int k, int i) -> C {
        const unsigned char *p = h[k].data() + (size_t)i * vs;
        switch (dt) {
        case CGAMD_F32: { float v; std::memcpy(&v, p, 4); return C(v, 0.); }
        case CGAMD_F64: { double v; std::memcpy(&v, p, 8); return C(v, 0.); }
        case CGAMD_C64: { float v[2]; std::memcpy(v, p, 8); return C(v[0], v[1]); }
        default: { double v[2]; std::memcpy(v, p, 16); return C(v[0], v[1]); }
        }
    };
    auto finite = [](C v) { return std::isfinite(v.real()) && std::isfinite(v.imag()); };
    const int E = (int)(16 / vs);
    const size_t pitch = ((size_t)n + 2 * E - 1) / (2 * E) * (2 * E);      // values per factor array: whole 32-byte rows of a thread
    out.pitch = pitch;
    out.coef.assign(3 * pitch * vs, 0);
    auto put = [&](int k, int i, C v) {
        unsigned char *p = out.coef.data() + ((size_t)k * pitch + i) * vs;
        switch (dt) {
        case CGAMD_F32: { const float f = (float)v.real(); std::memcpy(p, &f, 4); break; }
        case CGAMD_F64: { const double f = v.real(); std::memcpy(p, &f, 8); break; }
        case CGAMD_C64: { const float f[2] = {(float)v.real(), (float)v.imag()}; std::memcpy(p, f, 8); break; }
        default: { const double f[2] = {v.real(), v.imag()}; std::memcpy(p, f, 16); break; }
        }
    };
    const bool single = dt == CGAMD_F32 || dt == CGAMD_C64;
    auto rounds_to_zero = [&](C v) { return single ? ((float)v.real() == 0.f && (float)v.imag() == 0.f) : v == C(0., 0.); };
    out.l_zero.assign((size_t)n, 1);      // the stored -l / -w c are 0 (as the kernels see them)
    out.e_zero.assign((size_t)n, 1);
    std::vector<C> u_prev((size_t)stride, C(0., 0.)), c_prev((size_t)stride, C(0., 0.));      // of row i - stride, per chain
    for (int i = 0; i < nu; ++i) {
        const int ch = i % stride;
        const bool head = i < stride;
        const C a = head ? C(0., 0.) : get(0, i), b = get(1, i), c = i < nu - stride ? get(2, i) : C(0., 0.);
        if (!finite(a) || !finite(b) || !finite(c))
            return fail(CGAMD_ERR_INVALID, who + ": non-finite entry in row " + std::to_string(i));
        const C l = head ? C(0., 0.) : a / u_prev[ch];
        const C u = b - l * c_prev[ch];
        if (!finite(l) || !finite(u) || u == C(0., 0.))
            return fail(CGAMD_ERR_INVALID, who + ": zero or non-finite pivot in row " + std::to_string(i) +
                                               " (the factorisation does not pivot)");
        const C w = 1. / u;
        if (!finite(w)) return fail(CGAMD_ERR_INVALID, who + ": pivot too small in row " + std::to_string(i));
        put(0, i, -l);
        put(1, i, -(w * c));
        put(2, i, w);
        out.l_zero[i] = rounds_to_zero(l);
        out.e_zero[i] = rounds_to_zero(w * c);
        u_prev[ch] = u;
        c_prev[ch] = c;
    }
    // (the padding rows keep 0 everywhere: decoupled, z = 0 there)
    return CGAMD_OK;
}

// Chunk boundaries of the stride-1 sweep from the segment list (seg: the first rows in order, then n): O(segments).  Returns
// whether the sweep takes its long form (a segment does not fit one chunk: plain slices of Cmax rows).
static bool tri_plan_chunks(const std::vector<int> &seg, int n, int dt, std::vector<int> &starts) {
    const int Cmax = tri_chunk_rows(dt), R = Cmax / kBlock;
    starts.assign(1, 0);
    bool longform = false;
    for (size_t k = 1; k < seg.size() && !longform; ++k) {
        if (seg[k] - starts.back() / R * R <= Cmax) continue;        // segment k-1 still fits the current chunk
        if (seg[k - 1] == starts.back()) longform = true;            // it alone does not fit one
        else {
            starts.push_back(seg[k - 1]);
            if (seg[k] - seg[k - 1] / R * R > Cmax) longform = true;
        }
    }
    if (longform) {
        starts.clear();
        for (int i = 0; i < n; i += Cmax) starts.push_back(i);
    }
    starts.push_back(n);
    return longform;
}

// host factors and a host plan to the device
static int tri_upload(hipStream_t st, const std::string &who, const TriFactors &f, const std::vector<int> &plan, int stride, int count,
                      bool longform, TriBuilt *out) {
    void *coef = nullptr;
    int *dplan = nullptr;
    int rc = dmalloc(&coef, f.coef.size(), "tridiagonal factors");
    if (!rc) rc = dmalloc((void **)&dplan, plan.size() * 4, stride == 1 ? "tridiagonal chunk plan" : "tridiagonal segment plan");
    if (!rc) {
        hipError_t e = hipMemcpyAsync(coef, f.coef.data(), f.coef.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(dplan, plan.data(), plan.size() * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(CGAMD_ERR_HIP, who + " upload: " + hipGetErrorString(e));
    }
    if (rc) {
        if (coef) (void)hipFree(coef);
        if (dplan) (void)hipFree(dplan);
        return rc;
    }
    out->coef = coef; out->pitch = f.pitch; out->plan = dplan; out->stride = stride; out->count = count; out->longform = longform;
    return CGAMD_OK;
}

// Tridiagonal M: z solves M z = r (the reference PCG's spsolve branch, helmFE_var.py:561-562).  Factored here once, in double /
// complex double (Thomas LU, no pivoting: u_0 = b_0, l_i = a_i / u_{i-1}, u_i = b_i - l_i c_{i-1}); the kernels get -l, -w c and
// w = 1/u in the value type.  Rows where both couplings to the row before vanish start a segment; chunks of at most
// tri_chunk_rows() rows start at segment starts when every segment fits one (no carry between work-groups), else they are plain
// slices and the sweep takes its three-launch form.
// The same M at a distance (stride > 1): lower[i] = M[i][i-stride], upper[i] = M[i][i+stride].  The factorisation runs along every
// chain c, c + stride, ...; a chain is cut where both stored couplings round to zero in the value type (the rule of the stride-1
// form, at distance stride), and the plan is the list of those segments (first row, length) ordered by first row: one thread of
// pcg_tri_strided_kernel each, whatever their length.
int tri_build_host(hipStream_t st, int dt, int nu, int n, const std::string &who, int stride, const void *lower, const void *diag,
                   const void *upper, int on_device, TriBuilt *out) {
    TriFactors f;
    if (int rc = tri_factor(st, dt, nu, n, who, stride, lower, diag, upper, on_device, f)) return rc;
    if (stride == 1) {
        std::vector<int> seg;
        for (int i = 0; i < n; ++i)
            if (i == 0 || (f.l_zero[i] && f.e_zero[i - 1])) seg.push_back(i);
        seg.push_back(n);
        std::vector<int> starts;
        const bool longform = tri_plan_chunks(seg, n, dt, starts);
        return tri_upload(st, who, f, starts, 1, (int)starts.size() - 1, longform, out);
    }
    // row i starts a segment when it heads its chain or both couplings to row i - stride vanish; its length is known once the
    // chain's next start (or end) is: walk the rows backwards, carrying per chain the rows seen since the last start
    std::vector<int> segs;      // (first row, length) pairs, built last segment first
    {
        std::vector<int> run((size_t)stride, 0);
        for (int i = n - 1; i >= 0; --i) {
            int &len = run[i % stride];
            ++len;
            if (i < stride || (f.l_zero[i] && f.e_zero[i - stride])) {
                segs.push_back(len);
                segs.push_back(i);
                len = 0;
            }
        }
        std::reverse(segs.begin(), segs.end());
    }
    return tri_upload(st, who, f, segs, stride, (int)(segs.size() / 2), false, out);
}

// ---- preconditioners built from a CSR matrix, on the device (precond_build.hip) ---------------------------------------------------
namespace {
struct DevScratch {      // device allocations of one call, freed on return unless the caller took them
    std::vector<void *> ptrs;
    ~DevScratch() {
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
    int get(void **p, size_t bytes, const char *what) {
        const int rc = dmalloc(p, bytes, what);
        if (!rc) ptrs.push_back(*p);
        return rc;
    }
    void release(void *p) {
        for (void *&q : ptrs)
            if (q == p) q = nullptr;
    }
};
}  // namespace

// Longest pre-segment the device factorisation takes, one thread per pre-segment; beyond it the diagonals are extracted on the
// device and factored by the host route (source 3).  PROVISIONAL: the value is to be the largest segment length at
// which `scripts/line_setup_ab.py --groups chains` finds the device no slower than the host; that table
// (profiles/line_setup/long_segments.log) has not been measured yet.
constexpr int kLineHostRouteRows = 65536;

// The plan from the final segment flags: the flagged rows before every 256-row block, their number, then the ordered list -- with
// lengths for pcg_tri_strided_kernel (stride > 1), or through the host chunk planner (stride 1).  *plan is taken from tmp.
static int tri_plan_from_flags(hipStream_t st, int dt, int n, int stride, const unsigned char *flags, int *count, DevScratch &tmp,
                               int **plan_out, int *nplan_out, bool *longform_out) {
    int rc;
    if ((rc = launch_line_count(n, flags, count, st))) return rc;
    int nsegs = 0;
    CG_HIP(hipMemcpyAsync(&nsegs, count + line_count_ints(n) - 1, 4, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    int *plan = nullptr;
    int nplan = nsegs;
    bool longform = false;
    if (stride > 1) {       // the plan of pcg_tri_strided_kernel: (first row, length) ordered by first row
        if ((rc = tmp.get((void **)&plan, (size_t)nsegs * 8, "tridiagonal segment plan"))) return rc;
        if ((rc = launch_line_emit(n, stride, true, flags, count, plan, st))) return rc;
    } else {                // the segment starts go to the host chunk planner
        int *starts_dev = nullptr;
        if ((rc = tmp.get((void **)&starts_dev, (size_t)nsegs * 4, "tridiagonal segment starts"))) return rc;
        if ((rc = launch_line_emit(n, 1, false, flags, count, starts_dev, st))) return rc;
        std::vector<int> seg((size_t)nsegs + 1), starts;
        CG_HIP(hipMemcpyAsync(seg.data(), starts_dev, (size_t)nsegs * 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        seg[(size_t)nsegs] = n;
        longform = tri_plan_chunks(seg, n, dt, starts);
        nplan = (int)starts.size() - 1;
        if ((rc = tmp.get((void **)&plan, starts.size() * 4, "tridiagonal chunk plan"))) return rc;
        CG_HIP(hipMemcpyAsync(plan, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
        CG_HIP(hipStreamSynchronize(st));
    }
    *plan_out = plan; *nplan_out = nplan; *longform_out = longform;
    return CGAMD_OK;
}

// M = the matrix entries at column - row in {-stride, 0, +stride} among the columns below col_limit: extracted, factored and planned
// on the device.  The temporaries are three n-long value arrays, n flag bytes, one int per 256 rows and three words.
int tri_build_from_matrix(hipStream_t st, int dt, int nu, int n, int route, const std::string &who, int stride, const void *vals,
                          const int *ptr, const int *cols, int col_limit, TriBuilt *out) {
    const size_t vs = dtype_size(dt);
    DevScratch tmp;
    void *abc = nullptr, *words = nullptr;
    unsigned char *flags = nullptr;
    int *count = nullptr;
    int rc = tmp.get(&abc, 3 * (size_t)n * vs, "line preconditioner: diagonals");
    if (!rc) rc = tmp.get((void **)&flags, (size_t)n, "line preconditioner: flags");
    if (!rc) rc = tmp.get((void **)&count, (size_t)line_count_ints(n) * 4, "line preconditioner: block counts");
    if (!rc) rc = tmp.get(&words, 16, "line preconditioner: words");
    if (rc) return rc;
    char *lower = static_cast<char *>(abc), *diag = lower + (size_t)n * vs, *upper = diag + (size_t)n * vs;
    unsigned long long *err = static_cast<unsigned long long *>(words);
    int *longest = reinterpret_cast<int *>(err + 1);
    CG_HIP(hipMemsetAsync(abc, 0, 3 * (size_t)n * vs, st));      // (the padding rows: no couplings)
    CG_HIP(hipMemsetAsync(err, 0xff, 8, st));
    CG_HIP(hipMemsetAsync(longest, 0, 4, st));
    if ((rc = launch_line_extract(dt, nu, stride, vals, ptr, cols, col_limit, lower, diag, upper, st))) return rc;
    if ((rc = launch_line_flags(dt, n, stride, lower, upper, flags, st))) return rc;
    int longest_h = 0;      // route 1 / -1: forced, nothing to measure
    if (route == 0) {
        if ((rc = launch_line_longest(n, stride, flags, kLineHostRouteRows + 1, longest, st))) return rc;
        CG_HIP(hipMemcpyAsync(&longest_h, longest, 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
    }
    if (route > 0 || (route == 0 && longest_h > kLineHostRouteRows)) {
        // few long segments: one thread each is slower than the host's serial loop.  The extracted diagonals go the host route.
        CG_HIP(hipStreamSynchronize(st));
        rc = tri_build_host(st, dt, nu, n, who, stride, lower, diag, upper, 1, out);
        if (!rc) out->source = 3;
        return rc;
    }
    const int E = (int)(16 / vs);
    const size_t pitch = ((size_t)n + 2 * E - 1) / (2 * E) * (2 * E);      // as tri_factor lays the factors out
    void *coef = nullptr;
    if ((rc = tmp.get(&coef, 3 * pitch * vs, "tridiagonal factors"))) return rc;
    char *nl = static_cast<char *>(coef), *ne = nl + pitch * vs, *w = ne + pitch * vs;
    CG_HIP(hipMemsetAsync(coef, 0, 3 * pitch * vs, st));           // (the padding rows keep 0 everywhere: decoupled, z = 0 there)
    if ((rc = launch_line_factor(dt, nu, stride, flags, lower, diag, upper, nl, ne, w, err, st))) return rc;
    unsigned long long err_h = 0;
    CG_HIP(hipMemcpyAsync(&err_h, err, 8, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    if (err_h != ~0ull) {
        const std::string row = std::to_string(err_h >> 2);
        switch ((int)(err_h & 3)) {
        case 0: return fail(CGAMD_ERR_INVALID, who + ": non-finite entry in row " + row);
        case 1: return fail(CGAMD_ERR_INVALID, who + ": zero or non-finite pivot in row " + row + " (the factorisation does not pivot)");
        default: return fail(CGAMD_ERR_INVALID, who + ": pivot too small in row " + row);
        }
    }
    // the final segments, from the factors as stored
    if ((rc = launch_line_flags(dt, n, stride, nl, ne, flags, st))) return rc;
    int *plan = nullptr;
    int nplan = 0;
    bool longform = false;
    if ((rc = tri_plan_from_flags(st, dt, n, stride, flags, count, tmp, &plan, &nplan, &longform))) return rc;
    CG_HIP(hipStreamSynchronize(st));
    tmp.release(coef);
    tmp.release(plan);
    out->coef = coef; out->pitch = pitch; out->plan = plan; out->stride = stride; out->count = nplan; out->longform = longform;
    out->source = 2;
    return CGAMD_OK;
}

// m = 1 / diag(A) on the device (m: nu values, the caller's); names the smallest row with a zero, missing or non-finite diagonal
int jacobi_build_from_matrix(hipStream_t st, int dt, int nu, const std::string &who, const void *vals, const int *ptr, const int *cols,
                             void *m) {
    DevScratch tmp;
    void *err = nullptr;
    int rc = tmp.get(&err, 8, "Jacobi preconditioner: error word");
    if (rc) return rc;
    CG_HIP(hipMemsetAsync(err, 0xff, 8, st));
    if ((rc = launch_jacobi_extract(dt, nu, vals, ptr, cols, m, static_cast<unsigned long long *>(err), st))) return rc;
    unsigned long long err_h = 0;
    CG_HIP(hipMemcpyAsync(&err_h, err, 8, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    if (err_h != ~0ull)
        return fail(CGAMD_ERR_INVALID, who + ": zero, missing or non-finite diagonal in row " + std::to_string(err_h));
    return CGAMD_OK;
}

// ---- the same for nsys matrices on one pattern (a batched handle) -----------------------------------------------------------------
// Every system's lines are extracted and factored by ONE launch each (precond_build.hip, grid.y over the systems); the segment flags
// are AND-ed over the systems, so one plan serves all of them: a system whose own couplings vanish inside a shared segment has
// stored zeros there, which restart the sweeps' recurrences arithmetically.  Always on the device: long chains are factored serially.
static std::string system_row(unsigned long long sys, unsigned long long row) {
    return "system " + std::to_string(sys) + " row " + std::to_string(row);
}
int tri_build_from_matrix_batched(hipStream_t st, int dt, int nu, int n, int nsys, long long nnz, const std::string &who, int stride,
                                  const void *vals, const int *ptr, const int *cols, TriBuilt *out) {
    const size_t vs = dtype_size(dt);
    const int E = (int)(16 / vs);
    const size_t pitch = ((size_t)n + 2 * E - 1) / (2 * E) * (2 * E);      // per system, as tri_factor lays the factors out
    const size_t arr = pitch * (size_t)nsys * vs;                           // one array of all systems
    DevScratch tmp;
    void *abc = nullptr, *words = nullptr, *coef = nullptr;
    unsigned char *flags = nullptr;
    int *count = nullptr;
    int rc = tmp.get(&abc, 3 * arr, "batched line preconditioner: diagonals");
    if (!rc) rc = tmp.get(&coef, 3 * arr, "batched tridiagonal factors");
    if (!rc) rc = tmp.get((void **)&flags, (size_t)n, "batched line preconditioner: flags");
    if (!rc) rc = tmp.get((void **)&count, (size_t)line_count_ints(n) * 4, "batched line preconditioner: block counts");
    if (!rc) rc = tmp.get(&words, 16, "batched line preconditioner: words");
    if (rc) return rc;
    char *lower = static_cast<char *>(abc), *diag = lower + arr, *upper = diag + arr;
    char *nl = static_cast<char *>(coef), *ne = nl + arr, *w = ne + arr;
    unsigned long long *err = static_cast<unsigned long long *>(words);
    CG_HIP(hipMemsetAsync(abc, 0, 3 * arr, st));       // (the padding rows: no couplings)
    CG_HIP(hipMemsetAsync(coef, 0, 3 * arr, st));      // (... and 0 in every factor: decoupled, z = 0 there)
    CG_HIP(hipMemsetAsync(err, 0xff, 8, st));
    if ((rc = launch_batched_line_extract(dt, nu, stride, nsys, nnz, vals, ptr, cols, lower, diag, upper, (long long)pitch, st))) return rc;
    if ((rc = launch_batched_line_flags(dt, n, stride, nsys, lower, upper, (long long)pitch, flags, st))) return rc;
    if ((rc = launch_batched_line_factor(dt, nu, stride, nsys, flags, lower, diag, upper, nl, ne, w, (long long)pitch, err, st))) return rc;
    unsigned long long err_h = 0;
    CG_HIP(hipMemcpyAsync(&err_h, err, 8, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    if (err_h != ~0ull) {
        const std::string at = system_row(err_h >> kBatchedErrSystemShift, (err_h & ((1ull << kBatchedErrSystemShift) - 1)) >> 2);
        switch ((int)(err_h & 3)) {
        case 0: return fail(CGAMD_ERR_INVALID, who + ": non-finite entry in " + at);
        case 1: return fail(CGAMD_ERR_INVALID, who + ": zero or non-finite pivot in " + at + " (the factorisation does not pivot)");
        default: return fail(CGAMD_ERR_INVALID, who + ": pivot too small in " + at);
        }
    }
    if ((rc = launch_batched_line_flags(dt, n, stride, nsys, nl, ne, (long long)pitch, flags, st))) return rc;
    int *plan = nullptr;
    int nplan = 0;
    bool longform = false;
    if ((rc = tri_plan_from_flags(st, dt, n, stride, flags, count, tmp, &plan, &nplan, &longform))) return rc;
    CG_HIP(hipStreamSynchronize(st));
    tmp.release(coef);
    tmp.release(plan);
    out->coef = coef; out->pitch = pitch; out->plan = plan; out->stride = stride; out->count = nplan; out->longform = longform;
    out->source = 2; out->nsys = nsys;
    return CGAMD_OK;
}

int jacobi_build_from_matrix_batched(hipStream_t st, int dt, int nu, int nsys, long long nnz, const std::string &who, const void *vals,
                                     const int *ptr, const int *cols, void *m, long long pitch, int level) {
    DevScratch tmp;
    void *err = nullptr;
    int rc = tmp.get(&err, 8, "Jacobi preconditioner: error word");
    if (rc) return rc;
    CG_HIP(hipMemsetAsync(err, 0xff, 8, st));
    if ((rc = launch_batched_jacobi_extract(dt, nu, nsys, nnz, vals, ptr, cols, m, pitch, static_cast<unsigned long long *>(err), st))) return rc;
    unsigned long long err_h = 0;
    CG_HIP(hipMemcpyAsync(&err_h, err, 8, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    if (err_h != ~0ull)
        return fail(CGAMD_ERR_INVALID, who + ": zero, missing or non-finite diagonal in " +
                                           (level < 0 ? system_row(err_h >> 32, err_h & 0xffffffffull)
                                                      : "system " + std::to_string(err_h >> 32) + " level " + std::to_string(level) + " row " +
                                                            std::to_string(err_h & 0xffffffffull)));
    return CGAMD_OK;
}

}  // namespace cgamd
