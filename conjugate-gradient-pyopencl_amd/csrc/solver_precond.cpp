// The preconditioner entries of the single-GPU handle, single and batched: what installs, replaces, rebuilds and removes M
// (precond_state.h owns M itself), and the accessors of the multigrid hierarchy.  Every installer has the same shape: build the new M
// aside (nothing on the handle changes while that can fail), hand it to the handle's Precond, then pre_replaced.
#include <string>

#include "cgamd_internal.h"
#include "launch_util.h"
#include "solver_handle.h"

using namespace cgamd;

constexpr const char *kHermNoLines = "whose preconditioner is diagonal: the line sweeps form the unconjugated r.z and r.r";
constexpr const char *kHermNoCycle = "which the V-cycle does not serve";

// What an entry refuses for the state of the handle, in the order the entries have always checked, before anything changes.
// shared: NULL for an entry of the plain handle (one M for all right-hand sides), else the entry is a batched handle's (one M per
// system) and `shared` names its plain counterpart; herm_why: why a CGAMD_HERMITIAN handle is not served (NULL: it is); mg: a V-cycle
static int entry_refuses(const cgamd_solver *s, const char *who, const char *shared, const char *herm_why, bool mg) {
    if (!s) return fail(CGAMD_ERR_INVALID, std::string(who) + ": solver is NULL");
    if (shared && !s->nsys)
        return fail(CGAMD_ERR_STATE, std::string(who) + ": the handle is not batched (one matrix for all right-hand sides); use " + shared);
    if (!shared && s->nsys) return batched_refuses(who);
    if (herm_why && s->herm) return herm_refuses(who, herm_why);
    if (!shared)
        if (int rc = shifts_refuse(s, who)) return rc;
    if (mg && (s->flags & CGAMD_UNFUSED)) return fail(CGAMD_ERR_STATE, std::string(who) + ": CGAMD_UNFUSED replays the reference's kernel sequence");
    if (mg && !shared && s->rm_ok) return fail(CGAMD_ERR_STATE, std::string(who) + ": the handle keeps its right-hand sides interleaved (row-major layout)");
    return CGAMD_OK;
}

// M has just been replaced or removed: the captured graphs replay the old loop, the recurrence starts again at the next set_rhs, and
// the loop family -- so the order of the partial sums (apply_wide_order) -- may have changed.  A diagonal M runs in the chip-wide
// resident loop, whose plan creation skipped where the one-XCD loop runs the plain recurrence
static int pre_replaced(cgamd_solver *s) {
    destroy_graphs(s);
    s->rhs_set = false;
    if (s->pre.kind == Precond::kDiag && !s->resw.ok && !s->nsys && !s->herm)
        if (int rc = setup_resident_wide_plan(s)) return rc;
    apply_wide_order(s);
    return CGAMD_OK;
}
static int pre_begin(cgamd_solver *s) {
    CG_HIP(hipSetDevice(s->ctx->device));
    CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}
// the r.z partials and rho of the diagonal and multigrid loops, allocated at the first such M and kept
static int ensure_rz_rho(cgamd_solver *s) {
    if (!s->part_rz)
        if (int rc = dmalloc(&s->part_rz, acc_size(s->dtype) * s->part_rr_cap * s->nrhs, "partials_rz")) return rc;
    return precond_ensure_rho(&s->pre, s->dtype, s->nrhs);
}

// z = m .* r between residual and search direction: the reference's PCG with a diagonal CSR M (helmFE_var.py:546-586;
// pass 1/diag(A) for Jacobi).  m: `size` values of the solver's type shared by all right-hand sides -- on a batched handle one
// diagonal per system, at the caller's stride `size`.  The next cgamd_solver_set_rhs starts the preconditioned recurrence; history
// then holds r.r as before.  The handle's copy carries the padding rows (zero).
static int diag_install(cgamd_solver *s, const void *m, int on_device, Precond::Built built) {
    if (int rc = pre_begin(s)) return rc;
    if (!m) {       // removal
        precond_drop(&s->pre);
        return pre_replaced(s);
    }
    const size_t vs = dtype_size(s->dtype);
    const size_t nm = s->nsys ? (size_t)s->nsys : 1;
    hipStream_t st = s->ctx->stream;
    void *md = nullptr;
    if (int rc = dmalloc(&md, (size_t)s->n * nm * vs, "preconditioner")) return rc;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipError_t e = hipSuccess;
    if (s->n != s->n_user) e = hipMemsetAsync(md, 0, (size_t)s->n * nm * vs, st);
    if (e == hipSuccess) {
        if (nm == 1 || s->n == s->n_user) e = hipMemcpyAsync(md, m, (size_t)s->n_user * nm * vs, kind, st);
        else e = hipMemcpy2DAsync(md, (size_t)s->n * vs, m, (size_t)s->n_user * vs, (size_t)s->n_user * vs, nm, kind, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    int rc = e == hipSuccess ? ensure_rz_rho(s) : fail(CGAMD_ERR_HIP, std::string("set_preconditioner: ") + hipGetErrorString(e));
    if (rc) { (void)hipFree(md); return rc; }
    precond_take_diag(&s->pre, md, built);
    return pre_replaced(s);
}
int cgamd_solver_set_preconditioner(cgamd_solver *s, const void *m, int on_device) {
    if (!s) return fail(CGAMD_ERR_INVALID, "set_preconditioner: solver is NULL");
    if (s->nsys && m) return batched_refuses("set_preconditioner");
    if (m)      // (removal stays served)
        if (int rc = shifts_refuse(s, "set_preconditioner")) return rc;
    if (s->blk_pcg) return block_refuses(s, "set_preconditioner");       // (removal too: M is part of the preconditioned block's state)
    if (s->nsys && !precond_set(s)) return CGAMD_OK;      // there is none to remove
    TuneScope ts(&s->tune);       // (m == NULL also removes the per-system preconditioner of a batched handle)
    return diag_install(s, m, on_device, Precond::kCaller);
}

// Tridiagonal M from its three arrays (factored on the host, planned, uploaded), at stride 1 or at a distance:
// lower[i] = M[i][i-stride], upper[i] = M[i][i+stride].  Everything is checked before the handle changes.
static int tridiag_entry(cgamd_solver *s, const char *who, bool strided, int stride, const void *lower, const void *diag, const void *upper,
                         int on_device) {
    if (!s || !lower || !diag || !upper) return fail(CGAMD_ERR_INVALID, std::string(who) + ": null argument");
    if (s->nsys) return batched_refuses(who);
    if (s->herm) return herm_refuses(who, kHermNoLines);
    if (int rc = shifts_refuse(s, who)) return rc;
    if (strided && (stride < 1 || stride >= s->n_user)) return fail(CGAMD_ERR_INVALID, std::string(who) + ": stride must be in [1, size - 1]");
    TuneScope ts(&s->tune);
    if (int rc = pre_begin(s)) return rc;
    TriBuilt b;
    if (int rc = tri_build_host(s->ctx->stream, s->dtype, s->n_user, s->n, stride == 1 ? "set_preconditioner_tridiag" : who, stride, lower, diag,
                                upper, on_device, &b)) return rc;
    if (int rc = precond_take_tri(&s->pre, &b, s->dtype, s->nrhs, 0, 0)) return rc;
    return pre_replaced(s);
}
int cgamd_solver_set_preconditioner_tridiag(cgamd_solver *s, const void *lower, const void *diag, const void *upper, int on_device) {
    return tridiag_entry(s, "set_preconditioner_tridiag", false, 1, lower, diag, upper, on_device);
}
int cgamd_solver_set_preconditioner_tridiag_strided(cgamd_solver *s, int stride, const void *lower, const void *diag, const void *upper,
                                                    int on_device) {
    return tridiag_entry(s, "set_preconditioner_tridiag_strided", true, stride, lower, diag, upper, on_device);
}

// ---- preconditioners built from the handle's own matrix, on the device (precond_setup.cpp, precond_build.hip).  A batched handle:
// one M per system (M_r for right-hand side r), never one shared by all ----------------------------------------------------------
// M = the matrix entries at column - row in {-stride, 0, +stride}: extracted, factored and planned on the device; every system of a
// batched handle on one segment plan
static int line_from_matrix(cgamd_solver *s, const std::string &who, int stride) {
    if (int rc = pre_begin(s)) return rc;
    hipStream_t st = s->ctx->stream;
    TriBuilt b;
    int rc;
    if (s->nsys) rc = tri_build_from_matrix_batched(st, s->dtype, s->n_user, s->n, s->nsys, s->nnz, who, stride, s->vals, s->ptr, s->cols, &b);
    else rc = tri_build_from_matrix(st, s->dtype, s->n_user, s->n, s->tune.dev_line_host_route, who, stride, s->vals, s->ptr, s->cols, s->n_user, &b);
    if (rc) return rc;
    if (s->nsys) b.source = 2;      // (the batched build has the device route only)
    if ((rc = precond_take_tri(&s->pre, &b, s->dtype, s->nrhs, s->nsys, stride))) return rc;
    return pre_replaced(s);
}
int cgamd_solver_set_preconditioner_line(cgamd_solver *s, int stride) {
    if (int rc = entry_refuses(s, "set_preconditioner_line", nullptr, kHermNoLines, false)) return rc;
    if (stride < 1 || stride >= s->n_user) return fail(CGAMD_ERR_INVALID, "set_preconditioner_line: stride must be in [1, size - 1]");
    TuneScope ts(&s->tune);
    return line_from_matrix(s, "set_preconditioner_line", stride);
}

// m = 1 / diag(A) (m_r = 1 / diag(A_r) of every system) on the device, then the diagonal form itself
static int jacobi_from_matrix(cgamd_solver *s, const std::string &who) {
    if (int rc = pre_begin(s)) return rc;
    hipStream_t st = s->ctx->stream;
    void *m = nullptr;
    int rc = dmalloc(&m, (size_t)s->n_user * (s->nsys ? (size_t)s->nsys : 1) * dtype_size(s->dtype), "Jacobi preconditioner");
    if (rc) return rc;
    if (s->nsys) rc = jacobi_build_from_matrix_batched(st, s->dtype, s->n_user, s->nsys, s->nnz, who, s->vals, s->ptr, s->cols, m, s->n_user);
    else rc = jacobi_build_from_matrix(st, s->dtype, s->n_user, who, s->vals, s->ptr, s->cols, m);
    if (!rc) rc = diag_install(s, m, 1, Precond::kJacobi);
    (void)hipFree(m);
    return rc;
}
int cgamd_solver_set_preconditioner_jacobi(cgamd_solver *s) {
    if (int rc = entry_refuses(s, "set_preconditioner_jacobi", nullptr, nullptr, false)) return rc;
    TuneScope ts(&s->tune);
    return jacobi_from_matrix(s, "set_preconditioner_jacobi");
}

// ---- aggregation multigrid (multigrid_setup.cpp): the hierarchy is built from the matrix as it is now, on the device -- on a batched
// handle one hierarchy per system inside the same MgHierarchy, on shared aggregates and patterns
static int multigrid_from_matrix(cgamd_solver *s, const std::string &who, const MgParams &p) {
    if (int rc = pre_begin(s)) return rc;
    MgHierarchy *h = nullptr;
    int rc = mg_build(s->ctx->stream, s->dtype, s->n_user, s->n, s->nrhs, s->nsys, s->plan, s->nnz, s->vals, s->ptr, s->cols, p, who, &h);
    if (rc) return rc;
    if ((rc = ensure_rz_rho(s))) { mg_free(h); return rc; }
    precond_take_mg(&s->pre, h, p);
    return pre_replaced(s);
}
int cgamd_solver_set_preconditioner_multigrid(cgamd_solver *s, int nx, int ny, int nz, int smooth_steps, double over_correction, int min_rows) {
    const std::string who = "set_preconditioner_multigrid";
    if (int rc = entry_refuses(s, who.c_str(), nullptr, kHermNoCycle, true)) return rc;
    MgParams p;
    if (int rc = mg_params_grid(who, s->n_user, nullptr, nx, ny, nz, smooth_steps, over_correction, min_rows, &p)) return rc;
    TuneScope ts(&s->tune);
    return multigrid_from_matrix(s, who, p);
}
// the same hierarchy with aggregates matched from the matrix (amg.hip): everything downstream of mg_build is the grid entry's
int cgamd_solver_set_preconditioner_amg(cgamd_solver *s, int passes, double strength, int smooth_steps, double over_correction, int min_rows) {
    const std::string who = "set_preconditioner_amg";
    if (int rc = entry_refuses(s, who.c_str(), nullptr, kHermNoCycle, true)) return rc;
    MgParams p;
    if (int rc = mg_params_amg(who, passes, strength, smooth_steps, over_correction, min_rows, &p)) return rc;
    TuneScope ts(&s->tune);
    return multigrid_from_matrix(s, who, p);
}

int cgamd::remove_and_fail(cgamd_solver *s, int rc) {
    if (s->pre.built == Precond::kCaller) return rc;        // (one from the caller's arrays does not depend on the matrix: kept)
    const std::string why = cgamd_last_error();
    if (s->blk_pcg) {       // preconditioned block CG goes with its M, whatever the wait returns: the mode never outlives M
        (void)pre_begin(s);
        block_drop(s);
    }
    (void)diag_install(s, nullptr, 0, Precond::kCaller);
    return fail(rc, why);
}

// the preconditioner the handle built from its matrix (matrices), built again from the values as they are now
int cgamd::rebuild_or_remove(cgamd_solver *s, const char *who) {
    int rc = CGAMD_OK;
    switch (s->pre.built) {
    case Precond::kCaller: return CGAMD_OK;         // (one from the caller's arrays is kept)
    case Precond::kJacobi: rc = jacobi_from_matrix(s, who); break;
    case Precond::kLine: rc = line_from_matrix(s, who, s->pre.stride); break;
    case Precond::kGridMg:
    case Precond::kAmg: rc = multigrid_from_matrix(s, who, MgParams(s->pre.mg_params)); break;
    }
    return rc ? remove_and_fail(s, rc) : CGAMD_OK;
}

int cgamd_solver_mg_levels(cgamd_solver *s) {
    if (!s) return -CGAMD_ERR_INVALID;
    return s->pre.mg ? mg_levels(s->pre.mg) : 0;
}
static int mg_wanted(cgamd_solver *s, const char *who) {
    if (!s) return fail(CGAMD_ERR_INVALID, std::string(who) + ": solver is NULL");
    if (!s->pre.mg) return fail(CGAMD_ERR_STATE, std::string(who) + ": no multigrid preconditioner is set");
    return CGAMD_OK;
}
int cgamd_solver_mg_level(cgamd_solver *s, int level, long long info[6]) {
    if (int rc = mg_wanted(s, "mg_level")) return rc;
    if (!info) return fail(CGAMD_ERR_INVALID, "mg_level: info is NULL");
    return mg_level_info(s->pre.mg, level, info);
}
int cgamd_solver_mg_level_bounds(cgamd_solver *s, int level, double *lmax, int count) {
    if (int rc = mg_wanted(s, "mg_level_bounds")) return rc;
    return mg_level_bounds(s->pre.mg, level, lmax, count);
}
int cgamd_solver_mg_level_matrix(cgamd_solver *s, int level, int *ptr, int *cols, void *vals) {
    if (int rc = mg_wanted(s, "mg_level_matrix")) return rc;
    CG_HIP(hipSetDevice(s->ctx->device));
    return mg_level_matrix(s->pre.mg, level, ptr, cols, vals, s->ctx->stream);
}
int cgamd_solver_mg_aggregates(cgamd_solver *s, int level, int *agg_host, int *n_coarse) {
    if (int rc = mg_wanted(s, "mg_aggregates")) return rc;
    CG_HIP(hipSetDevice(s->ctx->device));
    return mg_aggregates(s->pre.mg, level, agg_host, n_coarse, s->ctx->stream);
}
// one V-cycle on caller vectors (nRHS * size values each, device memory, stride `size`)
int cgamd_solver_mg_apply(cgamd_solver *s, const void *r_dev, void *z_dev) {
    if (int rc = mg_wanted(s, "mg_apply")) return rc;
    if (!r_dev || !z_dev) return fail(CGAMD_ERR_INVALID, "mg_apply: null argument");
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = stream_not_capturing(s->ctx->stream, "mg_apply")) return rc;
    return mg_apply_padded(s->pre.mg, s->ctx->stream, s->dtype, s->n, s->n_user, s->nrhs, r_dev, z_dev, "mg_apply");
}
int cgamd_solver_mg_level_state(cgamd_solver *s, int level, int which, void *out_host, long long cap_values, long long *count) {
    if (!s || !out_host || !count) return fail(CGAMD_ERR_INVALID, "mg_level_state: null argument");
    if (int rc = mg_wanted(s, "mg_level_state")) return rc;
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = stream_not_capturing(s->ctx->stream, "mg_level_state")) return rc;
    return mg_level_state(s->pre.mg, level, which, out_host, cap_values, count, s->ctx->stream);
}
int cgamd_solver_mg_level_spmv(cgamd_solver *s, int level, const void *x_dev, void *w_dev) {
    if (!s || !x_dev || !w_dev) return fail(CGAMD_ERR_INVALID, "mg_level_spmv: null argument");
    if (int rc = mg_wanted(s, "mg_level_spmv")) return rc;
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = stream_not_capturing(s->ctx->stream, "mg_level_spmv")) return rc;
    return mg_level_spmv(s->pre.mg, level, x_dev, w_dev, s->ctx->stream);
}

// ---- the entries of a batched handle --------------------------------------------------------------------------------------------
// m: nSystems * size values, the diagonal of system r at m + r * size; NULL removes any preconditioner
int cgamd_solver_set_preconditioner_batched(cgamd_solver *s, const void *m, int on_device) {
    if (int rc = entry_refuses(s, "set_preconditioner_batched", "cgamd_solver_set_preconditioner", nullptr, false)) return rc;
    if (!m && !precond_set(s)) return CGAMD_OK;
    TuneScope ts(&s->tune);
    return diag_install(s, m, on_device, Precond::kCaller);
}
int cgamd_solver_set_preconditioner_batched_jacobi(cgamd_solver *s) {
    if (int rc = entry_refuses(s, "set_preconditioner_batched_jacobi", "cgamd_solver_set_preconditioner_jacobi", nullptr, false)) return rc;
    TuneScope ts(&s->tune);
    return jacobi_from_matrix(s, "set_preconditioner_batched_jacobi");
}
int cgamd_solver_set_preconditioner_batched_line(cgamd_solver *s, int stride) {
    if (int rc = entry_refuses(s, "set_preconditioner_batched_line", "cgamd_solver_set_preconditioner_line", kHermNoLines, false)) return rc;
    if (stride < 1 || stride >= s->n_user) return fail(CGAMD_ERR_INVALID, "set_preconditioner_batched_line: stride must be in [1, size - 1]");
    TuneScope ts(&s->tune);
    return line_from_matrix(s, "set_preconditioner_batched_line", stride);
}
int cgamd_solver_set_preconditioner_batched_multigrid(cgamd_solver *s, int nx, int ny, int nz, int smooth_steps, double over_correction,
                                                      int min_rows) {
    const std::string who = "set_preconditioner_batched_multigrid";
    if (int rc = entry_refuses(s, who.c_str(), "cgamd_solver_set_preconditioner_multigrid", kHermNoCycle, true)) return rc;
    MgParams p;
    if (int rc = mg_params_grid(who, s->n_user, nullptr, nx, ny, nz, smooth_steps, over_correction, min_rows, &p)) return rc;
    TuneScope ts(&s->tune);
    return multigrid_from_matrix(s, who, p);
}

// 0 none, 1 the caller's arrays, 2 built from the matrix on the device, 3 lines extracted on the device and factored by the host route
int cgamd_solver_preconditioner_source(cgamd_solver *s) {
    if (!s || !precond_set(s)) return 0;
    if (s->pre.built == Precond::kCaller) return 1;
    return s->pre.built == Precond::kLine ? s->pre.route : 2;
}
