// Mixed-precision CG (include/cgamd.h "Mixed precision"): the recurrence runs in fp32 / complex64 on the INNER handle, x and the true
// residual live in fp64 / complex128 on the OUTER handle, and whenever the inner residual has dropped by `delta` the inner x is added
// into the outer one, r = b - A x is recomputed there, rounded down and handed back WITH THE DIRECTION KEPT
// (cgamd_solver_replace_residual) -- residual replacement after van der Vorst and Ye ("reliable updates"), not a restarted iterative
// refinement, which throws the Krylov space away at every restart.  The kernels between the two sides are in mixed.hip.
#include <cfloat>
#include <cmath>
#include <vector>

#include "cgamd_internal.h"

using namespace cgamd;

struct cgamd_mixed {
    cgamd_ctx *ctx = nullptr;
    int dtype_hi = 0, size = 0, nrhs = 1;
    cgamd_solver *outer = nullptr, *inner = nullptr;
    void *vals_lo = nullptr;        // the rounded values the inner handle runs on (its own copy, made once at create)
    void *r_lo = nullptr;           // round_down(r_hi) at the inner handle's leading dimension
    double *partials = nullptr;     // mixed_norm2: nrhs * G
    double *dev = nullptr;          // device: [norm2 | scale | 1 / scale] of nrhs doubles each, then the nrhs mask ints
    double *pin = nullptr;          // pinned image of `dev`
    std::vector<double> scales;     // of the last solve
};

static int mixed_free(cgamd_mixed *m) {
    if (m->inner) cgamd_solver_destroy(m->inner);
    if (m->outer) cgamd_solver_destroy(m->outer);
    for (void *p : {m->vals_lo, m->r_lo, (void *)m->partials, (void *)m->dev})
        if (p) (void)hipFree(p);
    if (m->pin) (void)hipHostFree(m->pin);
    delete m;
    return CGAMD_OK;
}

static int mixed_alloc(void **p, size_t bytes, const char *what) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(mixed ") + what + "): " + hipGetErrorString(e));
    return CGAMD_OK;
}

extern "C" {

int cgamd_mixed_create(cgamd_ctx *ctx, int dtype_hi, int size, long long nnz, const void *aValues_hi, const int *aPointers, const int *aCols,
                       int nRHS, int flags, cgamd_mixed **out) {
    // (what can be judged without a device comes first)
    if (!out) return fail(CGAMD_ERR_INVALID, "mixed_create: out is NULL");
    *out = nullptr;
    if (dtype_hi != CGAMD_F64 && dtype_hi != CGAMD_C128)
        return fail(CGAMD_ERR_INVALID, "mixed_create: dtype_hi must be CGAMD_F64 or CGAMD_C128 (the loop runs in fp32 / complex64 under it)");
    if (flags & ~(CGAMD_NO_GRAPH | CGAMD_MATRIX_ON_DEVICE))
        return fail(CGAMD_ERR_INVALID, "mixed_create: flags other than CGAMD_NO_GRAPH and CGAMD_MATRIX_ON_DEVICE (CGAMD_UNFUSED and "
                                       "CGAMD_HERMITIAN handles have no residual replacement)");
    if (!ctx) return fail(CGAMD_ERR_INVALID, "mixed_create: ctx is NULL");
    if (size < 1 || nnz < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, "mixed_create: bad size/nnz/nRHS");
    if (!aPointers || (nnz > 0 && (!aValues_hi || !aCols))) return fail(CGAMD_ERR_INVALID, "mixed_create: null matrix pointer");
    const int dtype_lo = dtype_hi == CGAMD_F64 ? CGAMD_F32 : CGAMD_C64;
    cgamd_mixed *m = new cgamd_mixed();
    m->ctx = ctx; m->dtype_hi = dtype_hi; m->size = size; m->nrhs = nRHS;
    m->scales.assign((size_t)nRHS, 1.);
    int rc = cgamd_solver_create(ctx, dtype_hi, size, nnz, aValues_hi, aPointers, aCols, nRHS, flags, &m->outer);
    if (!rc) rc = mixed_alloc(&m->vals_lo, (size_t)nnz * dtype_size(dtype_lo) + 64, "values");
    if (!rc) {      // the lo copy is taken here, once, from the values the outer handle's SpMV reads (its own copy or the borrowed array)
        const int *ptr = nullptr, *cols = nullptr;
        const void *vals_hi = solver_matrix(m->outer, &ptr, &cols);
        rc = launch_mixed_round_values(dtype_hi, nnz, vals_hi, m->vals_lo, ctx->stream);
        if (!rc) rc = cgamd_solver_create(ctx, dtype_lo, size, nnz, m->vals_lo, ptr, cols, nRHS, (flags & CGAMD_NO_GRAPH) | CGAMD_MATRIX_ON_DEVICE,
                                          &m->inner);
    }
    if (!rc) rc = mixed_alloc(&m->r_lo, (size_t)cgamd_solver_ld(m->inner) * nRHS * dtype_size(dtype_lo), "residual");
    if (!rc) rc = mixed_alloc((void **)&m->partials, sizeof(double) * (size_t)mixed_norm2_grid(dtype_hi, size) * nRHS, "norm partials");
    if (!rc) rc = mixed_alloc((void **)&m->dev, (size_t)nRHS * 32, "scalars");
    if (!rc && hipHostMalloc((void **)&m->pin, (size_t)nRHS * 32, hipHostMallocDefault) != hipSuccess)
        rc = fail(CGAMD_ERR_ALLOC, "mixed_create: hipHostMalloc");
    if (rc) {
        const std::string keep = cgamd_last_error();
        mixed_free(m);
        set_error(keep);
        return rc;
    }
    *out = m;
    return CGAMD_OK;
}

int cgamd_mixed_destroy(cgamd_mixed *m) {
    if (!m) return CGAMD_OK;
    if (m->ctx) {
        (void)hipSetDevice(m->ctx->device);
        (void)hipStreamSynchronize(m->ctx->stream);
    }
    return mixed_free(m);
}

cgamd_solver *cgamd_mixed_outer(cgamd_mixed *m) { return m ? m->outer : nullptr; }
cgamd_solver *cgamd_mixed_inner(cgamd_mixed *m) { return m ? m->inner : nullptr; }

int cgamd_mixed_scales(cgamd_mixed *m, double *scales) {
    if (!m || !scales) return fail(CGAMD_ERR_INVALID, "mixed_scales: null argument");
    for (int r = 0; r < m->nrhs; ++r) scales[r] = m->scales[(size_t)r];
    return CGAMD_OK;
}

// ---- the four streaming kernels as stateless entries (include/cgamd.h "Mixed precision: the kernels"): thin wrappers over the
// launch_mixed_* the solve calls, with leading dimensions and pointers left to the caller.  What can be judged without a device is
// judged first, the context last.
static int mixed_op(cgamd_ctx *ctx, int dtype_hi, long long size, int nRHS, const char *what) {
    if (dtype_hi != CGAMD_F64 && dtype_hi != CGAMD_C128) return fail(CGAMD_ERR_INVALID, std::string(what) + ": dtype_hi must be CGAMD_F64 or CGAMD_C128");
    if (size < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, std::string(what) + ": bad size/nRHS");
    if (!ctx) return fail(CGAMD_ERR_INVALID, std::string(what) + ": ctx is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(ctx->device));
    return CGAMD_OK;
}

int cgamd_mixed_accumulate(cgamd_ctx *ctx, int dtype_hi, int size, void *x_hi, long long ld_hi, const void *x_lo, long long ld_lo,
                           const double *scale, const int *mask, int nRHS) {
    if (!x_hi || !x_lo || !scale || !mask) return fail(CGAMD_ERR_INVALID, "mixed_accumulate: null pointer");
    if (ld_hi < size || ld_lo < size) return fail(CGAMD_ERR_INVALID, "mixed_accumulate: leading dimension below size");
    if (int rc = mixed_op(ctx, dtype_hi, size, nRHS, "mixed_accumulate")) return rc;
    return launch_mixed_accumulate(dtype_hi, size, x_hi, ld_hi, x_lo, ld_lo, scale, mask, nRHS, ctx->stream);
}

int cgamd_mixed_round_down(cgamd_ctx *ctx, int dtype_hi, int size, const void *r_hi, long long ld_hi, void *r_lo, long long ld_lo,
                           const double *inv_scale, int nRHS) {
    if (!r_hi || !r_lo || !inv_scale) return fail(CGAMD_ERR_INVALID, "mixed_round_down: null pointer");
    if (ld_hi < size || ld_lo < size) return fail(CGAMD_ERR_INVALID, "mixed_round_down: leading dimension below size");
    if (int rc = mixed_op(ctx, dtype_hi, size, nRHS, "mixed_round_down")) return rc;
    return launch_mixed_round_down(dtype_hi, size, r_hi, ld_hi, r_lo, ld_lo, inv_scale, nRHS, ctx->stream);
}

int cgamd_mixed_norm2_grid(int dtype_hi, int size) {
    if ((dtype_hi != CGAMD_F64 && dtype_hi != CGAMD_C128) || size < 1) return 0;
    return mixed_norm2_grid(dtype_hi, size);
}

int cgamd_mixed_norm2(cgamd_ctx *ctx, int dtype_hi, int size, const void *v, long long ld, int nRHS, double *partials, double *out) {
    if (!v || !partials || !out) return fail(CGAMD_ERR_INVALID, "mixed_norm2: null pointer");
    if (ld < size) return fail(CGAMD_ERR_INVALID, "mixed_norm2: leading dimension below size");
    if (int rc = mixed_op(ctx, dtype_hi, size, nRHS, "mixed_norm2")) return rc;
    return launch_mixed_norm2(dtype_hi, size, v, ld, nRHS, partials, out, ctx->stream);
}

int cgamd_mixed_round_values(cgamd_ctx *ctx, int dtype_hi, long long count, const void *hi, void *lo) {
    if (!hi || !lo) return fail(CGAMD_ERR_INVALID, "mixed_round_values: null pointer");
    if (int rc = mixed_op(ctx, dtype_hi, count, 1, "mixed_round_values")) return rc;
    return launch_mixed_round_values(dtype_hi, count, hi, lo, ctx->stream);
}

int cgamd_mixed_solve(cgamd_mixed *m, const void *b, void *x, int on_device, const double *tol, int nTol, int maxIterations, double delta,
                      int maxSegment, int checkEvery, int *iterations, double *resnorm, int *status, int *replacements) {
    if (!m || !b || !x || !tol || !iterations || !resnorm || !status || !replacements)
        return fail(CGAMD_ERR_INVALID, "mixed_solve: null argument");
    const int nr = m->nrhs;
    if (nTol != 1 && nTol != nr) return fail(CGAMD_ERR_INVALID, "mixed_solve: nTol must be 1 or nRHS");
    for (int i = 0; i < nTol; ++i)
        if (!(tol[i] > 0.)) return fail(CGAMD_ERR_INVALID, "mixed_solve: every tolerance must be positive");
    if (maxIterations < 0 || maxSegment < 0 || checkEvery < 0) return fail(CGAMD_ERR_INVALID, "mixed_solve: negative maxIterations, maxSegment or checkEvery");
    if (!(delta >= 0.) || !(delta < 1.)) return fail(CGAMD_ERR_INVALID, "mixed_solve: delta must be in [0, 1) (0 = 0.1)");
    if (delta == 0.) delta = 0.1;
    // what the inner handle cannot do (a line preconditioner, a row-major width) is its own refusal, before anything is touched
    if (solver_block_on(m->outer) || solver_block_on(m->inner))
        return fail(CGAMD_ERR_STATE, "mixed_solve: block CG is on (cgamd_solver_set_block) on one of the two handles, which this entry does not serve; turn it off first");
    if (int rc = solver_replace_planned(m->inner)) return rc;
    CG_HIP(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    const bool cplx = m->dtype_hi == CGAMD_C128;
    const int n = m->size;
    double *pn2 = m->pin, *pscale = m->pin + nr, *pinv = m->pin + 2 * nr;
    int *pmask = reinterpret_cast<int *>(m->pin + 3 * nr);
    double *dn2 = m->dev, *dscale = m->dev + nr, *dinv = m->dev + 2 * nr;
    int *dmask = reinterpret_cast<int *>(m->dev + 3 * nr);
    std::vector<double> dl((size_t)nr * 2), tseg((size_t)nr);
    std::vector<float> dl_lo((size_t)nr * 2);
    std::vector<int> its((size_t)nr);
    std::vector<char> done((size_t)nr, 0);
    for (int r = 0; r < nr; ++r) { iterations[r] = 0; status[r] = 1; resnorm[r] = 0.; }
    *replacements = 0;

    // 1. r_hi = b - A x_hi, delta = r_hi . r_hi: the outer handle's set_rhs
    if (int rc = cgamd_solver_set_rhs(m->outer, b, x, on_device)) return rc;
    if (cgamd_solver_layout(m->outer) != 0)
        return fail(CGAMD_ERR_STATE, "mixed_solve: the outer handle keeps its right-hand sides interleaved (row-major layout)");
    const long long ld_hi = cgamd_solver_ld(m->outer), ld_lo = cgamd_solver_ld(m->inner);
    int used = 0, open = nr;
    for (bool first = true;; first = false) {
        const int got = cgamd_solver_history(m->outer, dl.data(), 1);        // synchronises: once per segment
        if (got < 1) return got < 0 ? -got : fail(CGAMD_ERR_STATE, "mixed_solve: the outer handle has no residual");
        for (int r = 0; r < nr; ++r) {
            const double res = std::sqrt(cplx ? std::hypot(dl[2 * (size_t)r], dl[2 * (size_t)r + 1]) : std::fabs(dl[(size_t)r]));
            if (done[r]) continue;
            resnorm[r] = res;
            const double t = tol[nTol == 1 ? 0 : r];
            if (!(res >= t)) { done[r] = 1; status[r] = std::isnan(res) ? 2 : 0; --open; }
            else if (!std::isfinite(res)) { done[r] = 1; status[r] = 2; --open; }
        }
        if (open == 0 || used >= maxIterations) break;
        if (first) {    // the scale of every right-hand side, fixed for the whole solve: the power of two below its residual's 2-norm
            if (int rc = launch_mixed_norm2(m->dtype_hi, n, cgamd_solver_vector(m->outer, 1), ld_hi, nr, m->partials, dn2, st)) return rc;
            CG_HIP(hipMemcpyAsync(pn2, dn2, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
            CG_HIP(hipStreamSynchronize(st));
            for (int r = 0; r < nr; ++r) {
                const double nrm = std::sqrt(pn2[r]);
                const double s = (std::isfinite(nrm) && nrm > 0.) ? std::ldexp(1., std::ilogb(nrm)) : 1.;
                m->scales[(size_t)r] = pscale[r] = s;
                pinv[r] = 1. / s;
            }
            CG_HIP(hipMemcpyAsync(dscale, pscale, sizeof(double) * 2 * nr, hipMemcpyHostToDevice, st));
        }
        // 2. / 3. the residual goes down to the inner handle: a fresh start the first time, then replaced with the direction kept
        if (int rc = launch_mixed_round_down(m->dtype_hi, n, cgamd_solver_vector(m->outer, 1), ld_hi, m->r_lo, ld_lo, dinv, nr, st)) return rc;
        if (int rc = first ? solver_set_rhs_ld(m->inner, m->r_lo, ld_lo) : solver_replace_residual_ld(m->inner, m->r_lo, ld_lo)) return rc;
        // 4. advance until the inner residual has dropped by delta, or to the tolerance in the inner handle's scale
        if (cgamd_solver_history(m->inner, dl_lo.data(), 1) < 1) return fail(CGAMD_ERR_STATE, "mixed_solve: the inner handle has no residual");
        for (int r = 0; r < nr; ++r) {
            const double start = std::sqrt(cplx ? std::hypot((double)dl_lo[2 * (size_t)r], (double)dl_lo[2 * (size_t)r + 1]) : std::fabs((double)dl_lo[(size_t)r]));
            const double t = tol[nTol == 1 ? 0 : r] / m->scales[(size_t)r];
            tseg[(size_t)r] = done[r] ? DBL_MAX : (delta * start > t ? delta * start : t);
            pmask[r] = done[r] ? 0 : 1;
        }
        const int left = maxIterations - used, seg = (maxSegment > 0 && maxSegment < left) ? maxSegment : left;
        if (int rc = cgamd_solver_iterate_until(m->inner, seg, tseg.data(), nr, checkEvery, its.data())) return rc;
        used += cgamd_solver_iterations_done(m->inner);
        for (int r = 0; r < nr; ++r)
            if (!done[r]) iterations[r] += its[(size_t)r];
        // 5. x_hi += s x_lo for the open right-hand sides, and the true residual of the new x_hi
        CG_HIP(hipMemcpyAsync(dmask, pmask, sizeof(int) * nr, hipMemcpyHostToDevice, st));
        if (int rc = launch_mixed_accumulate(m->dtype_hi, n, cgamd_solver_vector(m->outer, 0), ld_hi, cgamd_solver_vector(m->inner, 0), ld_lo, dscale,
                                             dmask, nr, st)) return rc;
        if (int rc = solver_restart(m->outer)) return rc;
        ++*replacements;
    }
    if (int rc = cgamd_solver_get_x(m->outer, x, on_device)) return rc;
    CG_HIP(hipStreamSynchronize(st));
    return CGAMD_OK;
}

}  // extern "C"
