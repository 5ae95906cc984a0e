// Persistent single-GPU CG solver: the recurrence of reference clcg.c:250-430 (== cl.py:96-200 ==
// helmFE_var.py:507-544) with every scalar kept on the device, no host synchronisation inside the
// loop, and the per-iteration kernel sequence replayed from a hipGraph.
//
// Per iteration (fused, default) -- 4 launches instead of the reference's 6 kernels + 4 blocking copies:
//   spmv+dot   q = A d, partials of d.q                     (clcg.c:299-315)
//   cg_alpha   alpha = delta / (d.q)                          (clcg.c:317-334, done on the host there)
//   axpy2_dot  x += alpha d ; r -= alpha q ; partials of r.r (clcg.c:338-374)
//   aypx_beta  beta = delta_new/delta_old ; history ; d = beta d + r   (clcg.c:376-415; beta in the prologue)
// CGAMD_UNFUSED replays the reference's own op structure (spmv, vdot, axpy, axpy, vdot, aypx).
// CGAMD_HERMITIAN (complex types): the conjugated recurrence on four launches of its own (hermitian.hip), the SpMV unchanged.
// 16 / 32 right-hand sides (f64, complex64; f32 also 64): the block is kept ROW-MAJOR inside the handle and the
// product runs on the matrix cores (rowmajor.hip); the reference's RHS-major layout is converted in set_rhs / get_x.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "cgamd_internal.h"
#include "launch_util.h"
#include "solver_handle.h"
#include "spmv_device.h"
#include "xcd_schedule.h"

using namespace cgamd;

static int nshifts(const cgamd_solver *s) { return s->sh.view.S; }
static void *shift_xs(const cgamd_solver *s) { return s->sh.vec; }
static void *shift_ds(const cgamd_solver *s) { return static_cast<char *>(s->sh.vec) + dtype_size(s->dtype) * (size_t)nshifts(s) * s->nrhs * s->n; }
static void shifts_free(cgamd_solver *s) {
    for (void *p : {s->sh.vec, s->sh.scal, s->sh.view.history})
        if (p) (void)hipFree(p);
    s->sh = cgamd_solver::Shifts();
}

void cgamd::destroy_graphs(cgamd_solver *s) {
    for (int p = 0; p < 2; ++p) {
        if (s->g1[p]) (void)hipGraphExecDestroy(s->g1[p]);
        if (s->gU[p]) (void)hipGraphExecDestroy(s->gU[p]);
        if (s->g1g[p]) (void)hipGraphDestroy(s->g1g[p]);
        if (s->gUg[p]) (void)hipGraphDestroy(s->gUg[p]);
        s->g1[p] = s->gU[p] = nullptr;
        s->g1g[p] = s->gUg[p] = nullptr;
    }
    if (s->gT) (void)hipGraphExecDestroy(s->gT);
    if (s->gTg) (void)hipGraphDestroy(s->gTg);
    s->gT = nullptr; s->gTg = nullptr; s->gT_len = 0;
}

static void proj_free(cgamd_solver *s) {
    for (void *p : {s->proj.W, s->proj.x0, s->proj.scal, s->proj.partials})
        if (p) (void)hipFree(p);
    s->proj = cgamd_solver::Projection();
}
// the vectors held were A-orthonormal for the matrix that has just been replaced
static void proj_clear(cgamd_solver *s) { s->proj.m = s->proj.head = 0; s->proj.projected = s->proj.spent = false; }
static const char *kProjSpent = ": cgamd_solver_projection_update has used the handle's q and d storage: call set_rhs (of either kind) first";

static int validate_csr_host(int n, long long nnz, const int *ptr, const int *cols) {
    if (ptr[0] != 0) return fail(CGAMD_ERR_INVALID, "CSR: aPointers[0] != 0");
    for (int i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i]) return fail(CGAMD_ERR_INVALID, "CSR: aPointers not monotone at row " + std::to_string(i));
    if (ptr[n] != nnz) return fail(CGAMD_ERR_INVALID, "CSR: aPointers[size] != nonZeros");
    for (long long j = 0; j < nnz; ++j)
        if (cols[j] < 0 || cols[j] >= n) return fail(CGAMD_ERR_INVALID, "CSR: column index out of range at entry " + std::to_string(j));
    return CGAMD_OK;
}

// the SpMV (SpMM) launch of the iteration, bracketed by the caller's event pair when one is installed
static void *dbuf(cgamd_solver *s, int k) { return (s->fused2 && !s->until_mode && (k & 1)) ? s->d2 : s->d; }
// values between the diagonals of consecutive right-hand sides in s->pre.mdiag: a batched handle keeps one per system, else one for all
static long long m_pitch(const cgamd_solver *s) { return s->nsys ? s->n : 0; }
static bool fused2_now(const cgamd_solver *s) { return s->fused2 && !s->rm && !precond_set(s) && !(s->flags & CGAMD_UNFUSED) && !s->until_mode; }

// the handle's SpMV on n rows of RHS-major vectors: the batched kernel where every right-hand side has a matrix of its own
static int handle_spmv(cgamd_solver *s, int n, const void *x, long long ldx, void *y, long long ldy, const void *dvec, void *partials,
                       hipStream_t st) {
    if (s->nsys)
        return launch_spmv_batched(s->dtype, s->plan, n, s->nnz, s->nsys, s->vals, s->ptr, s->cols, x, ldx, y, ldy, dvec, partials, st);
    return launch_spmv(s->dtype, s->plan, n, s->nnz, s->vals, s->ptr, s->cols, x, ldx, y, ldy, s->nrhs, dvec, partials, st);
}

// k = iterations already enqueued since set_rhs (the iteration being enqueued is number k + 1)
// dvec: the direction the product is taken of where it is not s->d (a group iteration of the deferred x update)
static int enqueue_spmv(cgamd_solver *s, int k, hipStream_t st, void *dvec = nullptr) {
    const int dt = s->dtype, n = s->n, nr = s->nrhs;
    // timed pass: the row-block kernel of a single right-hand side takes the event pair on its dispatch (kernel duration);
    // every other SpMV form is bracketed by hipEventRecord (duration + launch gaps)
    const bool fused2 = fused2_now(s);
    const bool ext = s->ev_pair && !fused2 && !s->rm && nr == 1 && s->plan.kind == 5 && !s->nsys;
    if (s->ev_pair && !ext) CG_HIP(hipEventRecord(s->ev_pair[0], st));
    if (ext) set_kernel_event_pair(s->ev_pair);
    int rc;
    if (fused2)
        rc = launch_spmv_fused(dt, s->plan, n, s->nnz, s->vals, s->ptr, s->cols, dbuf(s, k), dbuf(s, k + 1), s->r, s->q, nr, s->part_dq,
                               s->part_rr, s->vgrid, s->sc, st);
    else if (s->rm) rc = launch_spmm_rm(dt, n, s->nnz, s->vals, s->ptr, s->cols, s->d, s->q, nr, s->part_dq, s->plan.max_quad, s->rm_pace, st);
    // (the preconditioned loops of a batched handle take alpha from the d.q partials whatever the flags)
    else if ((s->flags & CGAMD_UNFUSED) && !tri_on(s) && !(s->nsys && s->pre.mdiag)) rc = handle_spmv(s, n, s->d, n, s->q, n, nullptr, nullptr, st);
    else if (s->herm) rc = handle_spmv(s, n, s->d, n, s->q, n, s->d2, s->part_dq, st);       // the dot against dc = conj(d): d^H q
    else rc = handle_spmv(s, n, dvec ? dvec : s->d, n, s->q, n, dvec ? dvec : s->d, s->part_dq, st);
    set_kernel_event_pair(nullptr);
    if (rc) return rc;
    if (s->ev_pair && !ext) CG_HIP(hipEventRecord(s->ev_pair[1], st));
    return CGAMD_OK;
}

// r -= alpha q (update) and z = M^-1 r of a tridiagonal M, by the kernel of its form: the scan sweep of rows i +- 1 (precond.hip) or
// one thread per segment of rows i +- stride (precond_strided.hip)
// the r.z and r.r partials of the sweeps: the two halves of s->pre.tri_part, [nrhs][grid] each
static PcgPartials tri_partials(const cgamd_solver *s) { return pcg_partials(s->pre.tri_part, s->dtype, s->pre.tri.grid, s->nrhs); }
static int enqueue_tri_sweep(cgamd_solver *s, bool update, const void *q, void *z, hipStream_t st, const CgStop *g = nullptr) {
    const void *alpha = update ? s->sc.alpha : nullptr;
    const PcgPartials p = tri_partials(s);
    if (s->pre.tri.stride > 1) return launch_pcg_tri_strided(s->dtype, s->pre.tri, update, q, s->r, z, s->n, alpha, s->nrhs, p.rz, p.rr, st, g);
    return launch_pcg_tri(s->dtype, s->pre.tri, update, q, s->r, z, s->n, alpha, s->nrhs, p.rz, p.rr, st, g);
}

// Deferred x update: the lag the captured U-iteration graphs of this handle run with NOW (1 = none).  s->x_lag is what creation
// decided and allocated for; the loop family may have changed since (a preconditioner, the row-major layout)
static int x_lag_now(const cgamd_solver *s) {
    if (s->x_lag < 2 || s->nsys || s->rm || precond_set(s) || (s->flags & (CGAMD_UNFUSED | CGAMD_NO_GRAPH)) || fused2_now(s) || nshifts(s) || s->blk_on) return 1;
    return s->U % s->x_lag == 0 ? s->x_lag : 1;
}
static void *lag_dir(const cgamd_solver *s, int j) {
    return j == 0 ? s->d : j == 1 ? s->d2 : static_cast<char *>(s->dlag) + (size_t)(j - 2) * s->dlag_pitch;
}

// iteration j of a group of `lag` inside a captured graph: the SpMV on direction buffer j, alpha in its slot of the ring, the r
// update, and the d step into buffer j + 1 -- or, last of the group, the step that brings x up to date and writes buffer 0 = s->d
static int enqueue_lag_iteration(cgamd_solver *s, int k, int lag, int j, hipStream_t st) {
    const int dt = s->dtype, n = s->n, nr = s->nrhs;
    int rc;
    CgScalars sc = s->sc;
    sc.alpha = static_cast<char *>(s->sc.alpha) + dtype_size(dt) * (size_t)nr * lag_alpha_slot(j, lag);
    if ((rc = enqueue_spmv(s, k, st, lag_dir(s, j)))) return rc;
    const bool fold = fold_alpha_ok(s->plan.n_partials, s->plan.fold_max);
    if (!fold && (rc = launch_cg_alpha(dt, s->part_dq, s->plan.n_partials, nr, sc, st))) return rc;
    if (fold) rc = launch_axpy_dot_alpha(dt, n, s->q, s->r, n, s->part_dq, s->plan.n_partials, sc, nr, s->part_rr, s->vgrid, st);
    else rc = launch_axpy_dot(dt, n, s->q, s->r, n, sc.alpha, nr, s->part_rr, s->vgrid, st, s->plan.vec_nt);
    if (rc) return rc;
    if (j + 1 < lag)
        return launch_aypx_beta_out(dt, n, s->r, lag_dir(s, j), lag_dir(s, j + 1), n, s->part_rr, s->vgrid, nr, s->sc, st, s->plan.vec_nt);
    void *dirs[kLagMax];
    for (int i = 0; i < lag; ++i) dirs[i] = lag_dir(s, i);
    return launch_aypx_beta_xlag(dt, n, lag, s->r, dirs, s->x, n, s->part_rr, s->vgrid, nr, s->sc, st, s->plan.vec_nt);
}

// One block CG iteration (include/cgamd.h "Block CG"): the handle's SpMV as it is, without its dot, and the five launches of
// block_cg.hip -- a linear chain.  Every launch behind a breakdown or the stop leaves on the record's frozen word, under
// cgamd_solver_iterate as under cgamd_solver_iterate_until (g: the tolerances and the host's word); the SpMV is the unguarded one,
// its q is read by nothing that writes then
static int enqueue_block_pcg_iteration(cgamd_solver *s, int k, hipStream_t st, const CgStop *g);
static int enqueue_block_iteration(cgamd_solver *s, int k, hipStream_t st, const CgStop *g) {
    const int dt = s->dtype, n = s->n, S = s->nrhs;
    const BlockState &b = s->blk;
    const int *frozen = b.dev.rec + 2;
    int rc;
    if (s->blk_pcg) return enqueue_block_pcg_iteration(s, k, st, g);
    if (b.S != S || precond_set(s) || nshifts(s) || s->rm || s->herm || s->nsys || (s->flags & CGAMD_UNFUSED))
        return fail(CGAMD_ERR_STATE, "iterate: the handle is not in the state block CG was set up for");
    if (s->ev_pair) CG_HIP(hipEventRecord(s->ev_pair[0], st));
    if ((rc = handle_spmv(s, n, s->d, n, s->q, n, nullptr, nullptr, st))) return rc;
    if (s->ev_pair) CG_HIP(hipEventRecord(s->ev_pair[1], st));
    if ((rc = launch_block_gram(dt, n, n, S, s->d, s->q, b.dev.partials, b.grid, frozen, st))) return rc;
    if ((rc = launch_block_small(dt, 1, b, s->sc, g, st))) return rc;
    if ((rc = launch_block_xw(dt, n, n, S, s->d, s->q, s->x, s->r, b.dev.M_T, b.dev.alpha_T, b.dev.partials, b.grid, frozen, st))) return rc;
    if ((rc = launch_block_small(dt, 2, b, s->sc, g, st))) return rc;
    return launch_block_qp(dt, n, n, S, s->r, s->d, b.dev.tinv_T, b.dev.tau_T, false, frozen, st);
}

// The M^-1 side of preconditioned block CG (include/cgamd.h "Preconditioned block CG"; block_pcg.hip), shared by set_rhs and the
// iteration: Z = M^-1 W from r into q -- the V-cycle or the line sweeps, unguarded like the scalar multigrid loop's (what they write is
// read by nothing that writes once the loop is frozen), and nothing at all for a diagonal M -- then the partials of W^T Z beside those
// of W^T W: the Gram launch on (W, Z), or for a diagonal M the weighted one, which reads W and m and no Z
static int enqueue_block_pcg_wz(cgamd_solver *s, const int *frozen, hipStream_t st) {
    const int dt = s->dtype, n = s->n, S = s->nrhs;
    const BlockState &b = s->blk;
    int rc;
    if (s->pre.mdiag) return launch_block_gram_weighted(dt, n, n, S, s->r, s->pre.mdiag, b.dev.partials_z, b.grid, frozen, st);
    if (s->pre.mg) rc = mg_vcycle(s->pre.mg, s->r, s->q, st);
    else rc = enqueue_tri_sweep(s, false, nullptr, s->q, st);
    if (rc) return rc;
    return launch_block_gram(dt, n, n, S, s->r, s->q, b.dev.partials_z, b.grid, frozen, st);
}
// Q <- W tau^-1 ; P <- Z tau^-1 + P tau^T with Z in q, or z = m w formed in the launch
static int enqueue_block_pcg_qp(cgamd_solver *s, bool init, const int *frozen, hipStream_t st) {
    const BlockState &b = s->blk;
    return launch_block_qp_z(s->dtype, s->n, s->n, s->nrhs, s->r, s->d, s->pre.mdiag ? nullptr : s->q, s->pre.mdiag, b.dev.tinv_T, b.dev.tau_T, init,
                             frozen, st);
}
static bool block_pcg_state_ok(const cgamd_solver *s) {
    return s->blk.S == s->nrhs && s->blk.dev.CZ && precond_set(s) && (s->pre.mdiag || s->pre.mg || tri_on(s)) && !nshifts(s) && !s->rm && !s->herm &&
           !s->nsys && !(s->flags & CGAMD_UNFUSED);
}
// One preconditioned block iteration: the SpMV, the Gram launch and the G step and the x / w update of block CG as they are, then
// z = M^-1 w, the partials of W^T Z, the W step of block_pcg.hip and the q / p update with Z -- a linear chain, frozen like the
// unpreconditioned one
static int enqueue_block_pcg_iteration(cgamd_solver *s, int k, hipStream_t st, const CgStop *g) {
    const int dt = s->dtype, n = s->n, S = s->nrhs;
    const BlockState &b = s->blk;
    const int *frozen = b.dev.rec + 2;
    int rc;
    if (!block_pcg_state_ok(s)) return fail(CGAMD_ERR_STATE, "iterate: the handle is not in the state preconditioned block CG was set up for");
    if (s->ev_pair) CG_HIP(hipEventRecord(s->ev_pair[0], st));
    if ((rc = handle_spmv(s, n, s->d, n, s->q, n, nullptr, nullptr, st))) return rc;
    if (s->ev_pair) CG_HIP(hipEventRecord(s->ev_pair[1], st));
    if ((rc = launch_block_gram(dt, n, n, S, s->d, s->q, b.dev.partials, b.grid, frozen, st))) return rc;
    if ((rc = launch_block_small(dt, 1, b, s->sc, g, st))) return rc;
    if ((rc = launch_block_xw(dt, n, n, S, s->d, s->q, s->x, s->r, b.dev.M_T, b.dev.alpha_T, b.dev.partials, b.grid, frozen, st))) return rc;
    if ((rc = enqueue_block_pcg_wz(s, frozen, st))) return rc;
    if ((rc = launch_block_pcg_small(dt, 2, b, s->sc, g, st))) return rc;
    return enqueue_block_pcg_qp(s, false, frozen, st);
}

// lag >= 2 (capture of a U-iteration graph only): this is iteration k % lag of a group of the deferred x update
// g (cgamd_solver_iterate_until): the same launches with the guarded instantiation of every kernel that writes x, r, d, a scalar, the
// history or the counter (stop_device.h).  The SpMV is the unguarded one: q of a frozen right-hand side is recomputed from its frozen
// d and read by nothing.  Only the loops of a handle in until_mode have a guarded form -- the tridiagonal, the diagonal and the three /
// four-launch one; any other loop with a stop record is an error, never a silent unguarded run.
static int enqueue_iteration(cgamd_solver *s, int k, hipStream_t st, int lag = 1, const CgStop *g = nullptr) {
    const int dt = s->dtype, n = s->n, nr = s->nrhs;
    int rc;
    if (s->blk_on) return lag >= 2 ? fail(CGAMD_ERR_STATE, "iterate: block CG has no deferred x update") : enqueue_block_iteration(s, k, st, g);
    if (g && (lag >= 2 || fused2_now(s) || s->rm || (s->flags & CGAMD_UNFUSED)))
        return fail(CGAMD_ERR_STATE, "iterate_until: the loop this handle runs now has no guarded form");
    // (cgamd_solver_set_shifts and set_rhs see to it; any other loop with shifts in force is an error, never a run without them)
    if (nshifts(s) && (lag >= 2 || fused2_now(s) || s->rm || s->herm || precond_set(s) || (s->flags & CGAMD_UNFUSED)))
        return fail(CGAMD_ERR_STATE, "iterate: the loop this handle runs now does not carry the shifted systems");
    if (lag >= 2) return enqueue_lag_iteration(s, k, lag, k % lag, st);
    if (fused2_now(s)) {   // two launches: [beta, d = beta d + r, q = A d, d.q] and [alpha, x += alpha d, r -= alpha q, r.r]
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        return launch_axpy2_dot_alpha(dt, n, dbuf(s, k + 1), s->x, s->q, s->r, n, s->part_dq, s->plan.n_partials, s->sc, nr, s->part_rr, s->vgrid, st);
    }
    if (s->rm) {      // row-major block: SpMM on the matrix cores (+ d.q partials), alpha, r update (+ r.r), beta, x and d updates
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        if ((rc = launch_cg_alpha(dt, s->part_dq, s->rm_nwg, nr, s->sc, st))) return rc;
        if ((rc = launch_rm_axpy_dot(dt, n, nr, s->q, s->r, s->sc.alpha, s->part_rr, s->rm_vgrid, st))) return rc;
        if ((rc = launch_cg_beta(dt, s->part_rr, s->rm_vgrid, nr, s->sc, st))) return rc;
        return launch_rm_aypx_x(dt, n, nr, s->r, s->d, s->x, s->sc.alpha, s->sc.beta, s->rm_vgrid, st);
    }
    if (s->herm) {    // conjugated recurrence (hermitian.hip), with or without a diagonal M; delta holds rho
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        if ((rc = launch_herm_alpha(dt, s->part_dq, s->plan.n_partials, nr, s->sc, st, g))) return rc;
        if ((rc = launch_herm_axpy_dot(dt, n, s->q, s->r, s->pre.mdiag, m_pitch(s), n, s->sc.alpha, nr, s->part_rz, s->part_rr, s->vgrid, st, g))) return rc;
        return launch_herm_aypx_beta_x(dt, n, s->r, s->d, s->d2, s->x, s->pre.mdiag, m_pitch(s), n, s->part_rz, s->part_rr, s->vgrid, nr, s->sc,
                                       s->pre.rho2, st, g);
    }
    if (s->pre.mg) {      // multigrid M: r -= alpha q (+ r.r), z = V-cycle(r) in q's storage, r.z, then the tridiagonal loop's last launch
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        if ((rc = launch_cg_alpha(dt, s->part_dq, s->plan.n_partials, nr, s->sc, st, g))) return rc;
        if ((rc = launch_axpy_dot(dt, n, s->q, s->r, n, s->sc.alpha, nr, s->part_rr, s->vgrid, st, s->plan.vec_nt, g))) return rc;
        // (unguarded under iterate_until: z of a frozen right-hand side is read by nothing that writes)
        if ((rc = mg_vcycle(s->pre.mg, s->r, s->q, st))) return rc;
        if ((rc = launch_dot_partials(dt, n, s->r, s->q, n, nr, s->part_rz, s->vgrid, st))) return rc;
        return launch_pcg_aypx_beta_z(dt, n, s->d, s->q, n, s->part_rz, s->part_rr, s->vgrid, nr, s->sc, s->pre.rho2, s->x, st, g);
    }
    if (tri_on(s)) {  // tridiagonal M (helmFE_var.py:561-562): z = M^-1 r by the line sweeps, in q's storage
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        if ((rc = launch_cg_alpha(dt, s->part_dq, s->plan.n_partials, nr, s->sc, st, g))) return rc;
        if ((rc = enqueue_tri_sweep(s, true, s->q, s->q, st, g))) return rc;
        const PcgPartials p = tri_partials(s);
        return launch_pcg_aypx_beta_z(dt, n, s->d, s->q, n, p.rz, p.rr, s->pre.tri.grid, nr, s->sc, s->pre.rho2, s->x, st, g);
    }
    if (s->pre.mdiag) {   // preconditioned recurrence (helmFE_var.py:560-585); delta holds rho = r.z
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        if ((rc = launch_cg_alpha(dt, s->part_dq, s->plan.n_partials, nr, s->sc, st, g))) return rc;
        if ((rc = launch_pcg_axpy2_dot2(dt, false, n, s->d, s->x, s->q, s->r, s->pre.mdiag, n, s->sc.alpha, nr, s->part_rz, s->part_rr,
                                        s->vgrid, st, m_pitch(s), g))) return rc;
        return launch_pcg_aypx_beta(dt, n, s->r, s->d, s->pre.mdiag, n, s->part_rz, s->part_rr, s->vgrid, nr, s->sc, s->pre.rho2, s->x, st, m_pitch(s), g);
    }
    if (!(s->flags & CGAMD_UNFUSED)) {
        if ((rc = enqueue_spmv(s, k, st))) return rc;
        const bool fold = fold_alpha_ok(s->plan.n_partials, s->plan.fold_max);      // small system: alpha in the next launch's prologue
        if (!fold && (rc = launch_cg_alpha(dt, s->part_dq, s->plan.n_partials, nr, s->sc, st, g))) return rc;
        // r -= alpha q (+ r.r) ; then beta, x += alpha d, d = beta d + r : 3 + 5 vector passes (x is read by nothing inside the loop, so
        // its update rides in the aypx launch, which reads d anyway)
        if (fold) rc = launch_axpy_dot_alpha(dt, n, s->q, s->r, n, s->part_dq, s->plan.n_partials, s->sc, nr, s->part_rr, s->vgrid, st, g);
        else rc = launch_axpy_dot(dt, n, s->q, s->r, n, s->sc.alpha, nr, s->part_rr, s->vgrid, st, s->plan.vec_nt, g);
        if (rc) return rc;
        if ((rc = launch_aypx_beta_x(dt, n, s->r, s->d, s->x, n, s->part_rr, s->vgrid, nr, s->sc, st, s->plan.vec_nt, g))) return rc;
        if (!nshifts(s)) return CGAMD_OK;
        // the shifted systems, from alpha, beta and r_{k+1} as the seed's launches left them: the scalar step, then ONE vector launch
        const ShiftScalars &sh = s->sh.view;
        if ((rc = launch_shift_scalars(dt, nr, sh, s->sc, st, g))) return rc;
        return launch_shift_update(dt, n, n, nr, sh.S, s->r, shift_xs(s), shift_ds(s), sh.alpha_s, sh.beta_s, sh.zeta_s, st, s->plan.vec_nt, g);
    }
    if ((rc = enqueue_spmv(s, k, st))) return rc;
    if ((rc = launch_dot_partials(dt, n, s->d, s->q, n, nr, s->part_rr, s->vgrid, st))) return rc;
    if ((rc = launch_cg_alpha(dt, s->part_rr, s->vgrid, nr, s->sc, st))) return rc;
    if ((rc = launch_axpy(dt, n, s->d, s->x, n, s->sc.alpha, 1, nr, st))) return rc;
    if ((rc = launch_axpy(dt, n, s->q, s->r, n, s->sc.alpha, 0, nr, st))) return rc;
    if ((rc = launch_dot_partials(dt, n, s->r, s->r, n, nr, s->part_rr, s->vgrid, st))) return rc;
    if ((rc = launch_cg_beta(dt, s->part_rr, s->vgrid, nr, s->sc, st))) return rc;
    return launch_aypx(dt, n, s->r, s->d, n, s->sc.beta, nr, st);
}

// the resident loop applies where the two-launch loop does and the matrix slices fit LDS (needs the row pointers on the host)
// The launched loops of a handle the chip-wide resident loop can take over produce ITS bits (and the other way round): one
// 16-byte pack per thread in the vector launches (the r.r partial of a work-group = 256 consecutive packs), alpha folded whatever
// the size, and every prologue sum in the member-blocked order (reduce_device.h thread_partials; K = the blocks of one member).
// So iterate(15) twice and iterate(30) return the same bits although the first takes the launched loop and the second the
// resident one.  Called whenever the wide plan may have changed; captured graphs hold grids and orders, so they go when it did.
void cgamd::apply_wide_order(cgamd_solver *s) {
    if (s->nsys) return;        // a batched handle has no resident loop to match
    const int E = (int)(16 / dtype_size(s->dtype));
    // (where the one-XCD resident loop applies it runs, with the strided order -- unless a preconditioner is set: that recurrence only
    // has the chip-wide form; the tridiagonal one has none)
    const bool wide = s->resw.ok && !tri_on(s) && !s->pre.mg && (!s->res_ok || precond_set(s));
    const int kdq = wide ? kResWideBlocksPerRpt * s->resw.rpt : 0, krr = wide ? kdq / E : 0;
    const int vgrid = wide ? (s->n / E + kBlock - 1) / kBlock : vec_grid(s->n, s->dtype, s->nrhs);
    const int fold_max = 0;      // (alpha folded beyond 2048 partials was tried for these handles: every work-group summing 3907 partials, 1M rows 30 -> 52 us)
    if (kdq == s->sc.kdq && krr == s->sc.krr && vgrid == s->vgrid && fold_max == s->plan.fold_max) return;
    destroy_graphs(s);
    s->sc.kdq = kdq; s->sc.krr = krr; s->vgrid = vgrid; s->plan.fold_max = fold_max;
    s->fused2 = !s->herm && fused2_ok(s->plan, s->dtype, s->nrhs, s->vals, s->cols);
}

// the resident loop applies where the two-launch loop does and the matrix slices fit LDS (needs the row pointers on the host)
int cgamd::setup_resident_wide_plan(cgamd_solver *s) {
    s->resw.ok = false;
    if (tune().resident_wide == 0 || tune().resident == 0 || (s->flags & CGAMD_UNFUSED)) return CGAMD_OK;
    if (s->rm_ok && tune().spmm_rowmajor >= 2) return CGAMD_OK;      // the row-major loop was asked for
    if (!aligned16(s->x) || !aligned16(s->r) || !aligned16(s->d) || !aligned16(s->d2)) return CGAMD_OK;
    if (s->plan.kind != 5 && s->plan.kind != 6) return CGAMD_OK;    // the launched loops' 256-row d.q partials are what the members reproduce
    if (s->n % (int)(16 / dtype_size(s->dtype)) != 0) return CGAMD_OK;
    if (!s->n_cus) CG_HIP(hipDeviceGetAttribute(&s->n_cus, hipDeviceAttributeMultiprocessorCount, s->ctx->device));
    ResidentWidePlan wp;
    // (systems of up to 32768 rows only where the two-launch loop is the handle's launched loop and the one-XCD loop cannot hold them:
    // complex128 with 7-entry rows, 1024 rows x 20 bytes per entry do not fit LDS)
    if (int rc = resident_wide_plan(s->dtype, s->n, s->nnz, s->nrhs, s->n_cus, s->ptr, s->cols, s->sc.iter, s->ctx->stream, &wp, s->fused2)) return rc;
    if (!wp.ok) return CGAMD_OK;
    if ((size_t)((s->n / (int)(16 / dtype_size(s->dtype)) + kBlock - 1) / kBlock) > s->part_rr_cap) return CGAMD_OK;     // (cannot happen: sized at creation)
    if (s->resw_sync && wp.sync_bytes > s->resw.sync_bytes) { (void)hipFree(s->resw_sync); s->resw_sync = nullptr; }
    if (!s->resw_sync)
        if (int rc = dmalloc(&s->resw_sync, wp.sync_bytes, "wide resident sync words")) return rc;
    s->resw = wp;
    s->rm_ok = false;       // the chip-wide resident groups keep the caller's RHS-major layout (and beat the row-major loop: 1M x 32 fp64)
    return CGAMD_OK;
}

// the codes made from the VALUES (value, joint and row-pattern codes): freed, the plan reads aValues again
static void drop_value_codes(cgamd_solver *s) {
    if (s->vcodes) { (void)hipFree(s->vcodes); s->vcodes = nullptr; }
    if (s->vdict) { (void)hipFree(s->vdict); s->vdict = nullptr; }
    s->plan.vcodes = nullptr; s->plan.vdict = nullptr; s->plan.vcodes_for = nullptr;
    s->n_values = 0;
    if (s->jcodes) { (void)hipFree(s->jcodes); s->jcodes = nullptr; }
    if (s->jdict_off) { (void)hipFree(s->jdict_off); s->jdict_off = nullptr; }
    if (s->jdict_val) { (void)hipFree(s->jdict_val); s->jdict_val = nullptr; }
    s->plan.jcodes = nullptr; s->plan.jdict_off = nullptr; s->plan.jdict_val = nullptr;
    s->n_pairs = 0;
    if (s->rcodes) { (void)hipFree(s->rcodes); s->rcodes = nullptr; }
    if (s->rdict) { (void)hipFree(s->rdict); s->rdict = nullptr; }
    s->plan.rcodes = nullptr; s->plan.rdict_len = nullptr; s->plan.rdict_off = nullptr; s->plan.rdict_val = nullptr; s->plan.n_patterns = 0;
    s->plan.rcodes_for = nullptr;
    s->n_patterns = 0; s->n_user_patterns = 0;
    if (s->pcodes) { (void)hipFree(s->pcodes); s->pcodes = nullptr; }
    if (s->pdict) { (void)hipFree(s->pdict); s->pdict = nullptr; }
    s->plan.pcodes = nullptr; s->plan.pdict = nullptr; s->plan.n_pair_patterns = 0; s->plan.pair_slots = 0;
    s->n_pair_patterns = 0;
    if (s->sched) { (void)hipFree(s->sched); s->sched = nullptr; }
    s->plan.sched = nullptr; s->plan.sched_grid = 0;
    s->sched_unit = 0;
}
// The plane-matched XCD schedule of a handle that has just got its row codes.  The unit is the handle's largest
// stride, read from the row dictionary (9 KB to the host, once per pattern); where spmv_plane_wanted, the table of build_xcd_schedule
// goes to the device and the row- and pair-coded launches take it and its grid.  Built and dropped with the row codes, so captured
// graphs are destroyed wherever its pointer changes.
static int setup_xcd_schedule(cgamd_solver *s) {
    const size_t vsz = dtype_size(s->dtype);
    hipStream_t st = s->ctx->stream;
    std::vector<int> off(256 * 8), len(256);
    const char *rd = static_cast<const char *>(s->rdict);
    CG_HIP(hipMemcpyAsync(off.data(), rd + row_dict_off_at(vsz), off.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    CG_HIP(hipMemcpyAsync(len.data(), rd + row_dict_len_at(vsz), len.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    long long unit = 0;
    for (int c = 0; c < s->n_patterns && c < 256; ++c)
        for (int j = 0; j < len[c] && j < 8; ++j) unit = std::max(unit, std::llabs((long long)off[c * 8 + j]) / (long long)vsz);
    s->sched_unit = unit;
    if (!spmv_plane_wanted(s->tune.dev_spmv_plane, unit, kSuperRows, (size_t)s->nnz * (vsz + 4))) return CGAMD_OK;
    std::vector<int> table;
    const int supers = (s->plan.row_blocks + kSuperRows / kBlock - 1) / (kSuperRows / kBlock);
    const int grid = build_xcd_schedule(supers, kSuperRows, unit, table);
    if (grid <= 0) return CGAMD_OK;
    // the default rule takes only a table that loads the XCDs evenly (the launch lasts as long as the longest list); asked for by
    // name (dev.spmv_plane = 1) any table runs
    if (s->tune.dev_spmv_plane != 1 && !xcd_schedule_balanced(supers, grid)) return CGAMD_OK;
    CG_HIP(hipMalloc(&s->sched, table.size() * sizeof(int)));
    CG_HIP(hipMemcpyAsync(s->sched, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, st));
    CG_HIP(hipStreamSynchronize(st));       // (the host table goes away)
    s->plan.sched = s->sched; s->plan.sched_grid = grid;
    return CGAMD_OK;
}
// a handle whose SpMV reads one-byte column codes may carry codes of its values on top
static bool value_codes_apply(const cgamd_solver *s) {
    return s->codes && !s->plan.codes16 && !s->nsys && s->tune.value_codes && s->plan.kind == 5 && s->dtype != CGAMD_C128;
}
// the ladder on top of the one-byte column codes, for the values now in s->vals (create, reload_matrix, refresh_values); the handle
// has none of these codes when this is called (drop_value_codes)
static int setup_value_codes(cgamd_solver *s) {
    if (!value_codes_apply(s)) return CGAMD_OK;
    const size_t matrix_bytes = (size_t)s->nnz * (dtype_size(s->dtype) + 4);
    // matrices of at most 256 distinct entries (constant-coefficient stencils): one-byte value codes as well, 2 bytes per non-zero
    if (int rc = build_value_codes(s->dtype, s->nnz, s->vals, s->ctx->stream, &s->vcodes, &s->vdict, &s->n_values)) return rc;
    if (s->vcodes) { s->plan.vcodes = s->vcodes; s->plan.vdict = s->vdict; s->plan.vcodes_for = s->vals; }
    if (!s->vcodes || !s->tune.dev_joint_codes) return CGAMD_OK;
    if (int rc = build_joint_codes(s->dtype, s->nnz, s->codes, s->vcodes, s->dict, s->vdict, s->ctx->stream, &s->jcodes, &s->jdict_off,
                                   &s->jdict_val, &s->n_pairs)) return rc;
    if (s->jcodes) { s->plan.jcodes = s->jcodes; s->plan.jdict_off = s->jdict_off; s->plan.jdict_val = s->jdict_val; }
    // ... and one byte per ROW where the rows fit a 64-bit pattern key and few patterns occur (stencils: 9, 27); a threshold
    // of its own, so that index_codes_min_mb = 0 alone keeps the joint form on a small matrix
    const size_t vsz = dtype_size(s->dtype);
    if (s->jcodes && s->nrhs == 1 && s->plan.kind == 5 && s->plan.max_row > 0 && s->plan.max_row <= 7 && s->tune.dev_row_codes &&
        s->tune.dev_row_codes_min_mb >= 0 && matrix_bytes > ((size_t)s->tune.dev_row_codes_min_mb << 20) &&
        (unsigned long long)s->n * vsz < (1ULL << 30)) {
        if (int rc = build_row_codes(s->dtype, s->n, s->n_user, s->ptr, s->jcodes, s->jdict_off, s->jdict_val, s->ctx->stream, &s->rcodes,
                                     &s->rdict, &s->n_patterns, &s->n_user_patterns)) return rc;
        if (s->rcodes) {
            const char *rd = static_cast<const char *>(s->rdict);
            s->plan.rcodes = s->rcodes; s->plan.rdict_val = rd; s->plan.n_patterns = s->n_patterns;
            s->plan.rdict_off = reinterpret_cast<const int *>(rd + row_dict_off_at(vsz));
            s->plan.rdict_len = reinterpret_cast<const int *>(rd + row_dict_len_at(vsz));
            s->plan.rcodes_for = s->ptr;
            // ... and one byte per PAIR of rows (two rows per lane, one 16-byte gather per slot) above a threshold of its own
            if (row_pairs_wanted(s->tune.dev_row_pairs, vsz) && s->tune.dev_row_pairs_min_mb >= 0 &&
                matrix_bytes > ((size_t)s->tune.dev_row_pairs_min_mb << 20)) {
                if (int rc = build_row_pairs(s->dtype, s->n, s->rcodes, s->rdict, s->n_patterns, s->ctx->stream, &s->pcodes, &s->pdict,
                                             &s->n_pair_patterns, &s->plan.pair_slots)) return rc;
                if (s->pcodes) { s->plan.pcodes = s->pcodes; s->plan.pdict = s->pdict; s->plan.n_pair_patterns = s->n_pair_patterns; }
            }
            // ... and both forms' super blocks dealt to the XCDs by their place inside the largest stride
            if (int rc = setup_xcd_schedule(s)) return rc;
        }
    }
    return CGAMD_OK;
}

// (re)build the one-byte column codes for the matrix now in s->cols, and the value codes on top; dropped when they do not apply
static int setup_index_codes(cgamd_solver *s) {
    if (s->codes) { (void)hipFree(s->codes); s->codes = nullptr; }
    if (s->dict) { (void)hipFree(s->dict); s->dict = nullptr; }
    s->plan.codes = nullptr; s->plan.dict = nullptr; s->plan.codes_for = nullptr; s->plan.codes16 = false;
    s->n_offsets = 0;
    drop_value_codes(s);
    const size_t matrix_bytes = (size_t)s->nnz * (dtype_size(s->dtype) + 4);
    // a handle whose iterations run in the chip-wide resident loop (matrix in registers) would pay the two coding passes at every
    // create / reload (the stateless cg() reloads per call) for the few launched SpMVs around it
    if (s->resw.ok && !(s->flags & CGAMD_NO_GRAPH) && s->tune.index_codes < 2) return CGAMD_OK;
    if (!s->tune.index_codes || s->nrhs != 1 || (s->plan.kind != 5 && s->plan.kind != 7) || s->tune.index_codes_min_mb < 0 ||
        matrix_bytes <= ((size_t)s->tune.index_codes_min_mb << 20))
        return CGAMD_OK;
    if (int rc = build_index_codes(s->n, s->nnz, s->ptr, s->cols, s->ctx->stream, &s->codes, &s->dict, &s->n_offsets)) return rc;
    if (s->codes) {
        s->plan.codes = s->codes; s->plan.dict = s->dict; s->plan.codes_for = s->cols; s->plan.codes16 = false;
        return setup_value_codes(s);
    }
    // more than 256 distinct offsets (unstructured patterns, Matrix-Market inputs): 16-bit columns relative to the row block's first
    if (s->tune.index_codes16 == 0) return CGAMD_OK;
    if (int rc = build_index_codes16(s->n, s->nnz, s->ptr, s->cols, s->ctx->stream, &s->codes, &s->dict)) return rc;
    if (s->codes) { s->plan.codes = s->codes; s->plan.dict = s->dict; s->plan.codes_for = s->cols; s->plan.codes16 = true; s->n_offsets = 65536; }
    return CGAMD_OK;
}

static int setup_resident_local(cgamd_solver *s);
static int setup_resident(cgamd_solver *s) {
    const int rc = setup_resident_local(s);
    apply_wide_order(s);
    return rc;
}
// the one-XCD loop where it applies (bit-identical to the two-launch loop as it is); else the chip-wide groups
static int setup_resident_one_xcd(cgamd_solver *s);
static int setup_resident_local(cgamd_solver *s) {
    s->res_ok = false;
    s->resw.ok = false;
    if (s->herm) return CGAMD_OK;       // the conjugated recurrence has no resident form
    if (int rc = setup_resident_one_xcd(s)) return rc;
    // where the one-XCD loop applies the chip-wide plan is only needed once a preconditioner is set (that recurrence has no one-XCD
    // form): cgamd_solver_set_preconditioner asks for it then -- the stateless cg() entry reloads per call and would pay the scan
    if (s->res_ok && !s->pre.mdiag) return CGAMD_OK;
    return setup_resident_wide_plan(s);
}
static int setup_resident_one_xcd(cgamd_solver *s) {
    if (!s->fused2 || tune().resident == 0 || s->n > 65536) return CGAMD_OK;
    std::vector<int> tmp;
    const int *ph = s->ptr_host.size() == (size_t)s->n + 1 ? s->ptr_host.data() : nullptr;
    if (!ph) {          // borrowed device matrix
        tmp.resize((size_t)s->n + 1);
        CG_HIP(hipMemcpyAsync(tmp.data(), s->ptr, tmp.size() * 4, hipMemcpyDeviceToHost, s->ctx->stream));
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        ph = tmp.data();
    }
    if (!s->n_cus) CG_HIP(hipDeviceGetAttribute(&s->n_cus, hipDeviceAttributeMultiprocessorCount, s->ctx->device));
    ResidentPlan rp;
    if (!aligned16(s->x) || !aligned16(s->r) || !aligned16(s->d) || !aligned16(s->d2)) return CGAMD_OK;
    int max_window = 0;
    if (s->n % (int)(16 / dtype_size(s->dtype)) == 0)
        if (int rc = resident_max_window(s->dtype, s->n, s->ptr, s->cols, s->sc.iter, s->ctx->stream, &max_window)) return rc;
    // (checked against the plain launched configuration: the vector grid of a handle no chip-wide loop takes over)
    if (!resident_plan(s->dtype, s->n, vec_grid(s->n, s->dtype, s->nrhs), s->plan.n_partials, s->n_cus, ph, max_window, &rp)) return CGAMD_OK;
    if (s->res_sync && rp.sync_bytes > s->res.sync_bytes) { (void)hipFree(s->res_sync); s->res_sync = nullptr; }
    if (!s->res_sync)
        if (int rc = dmalloc(&s->res_sync, rp.sync_bytes, "resident sync words")) return rc;
    s->res = rp;
    s->res_ok = true;
    return CGAMD_OK;
}

// The lag of the deferred x update this handle is to run with, and its direction buffers beyond d and d2 (allocated here, never
// inside a capture).  dev.x_lag forces 2 / 4 / 8 (0, 1: off); the default rule (-1) turns it on where the loop is the four-launch
// form (alpha not folded: more than 2048 d.q partials, vectors far beyond the caches) with the lag the three legs of
// profiles/x_lag/ab.log speak for: 10M rows fp64 5784 it/s without, 6059 with 4, 6094 with 8; fp32 10252 / 10892 / 10872; 100M rows
// fp64 521.3 / 573.4 / 558.7.  8 wins the first by 0.6 %, 4 the other two (by 2.6 % at 100M rows) with two extra vectors instead of six.
// A handle whose buffers cannot be allocated runs without: cgamd_solver_x_lag says 1.
constexpr int kXLagDefault = 4;
static void setup_x_lag(cgamd_solver *s) {
    const int knob = s->tune.dev_x_lag;
    // (a handle the chip-wide resident loop takes over launches a graph for the few calls too short for that loop only)
    int lag = knob >= 0 ? std::max(knob, 1) : (fold_alpha_ok(s->plan.n_partials, s->plan.fold_max) || s->resw.ok ? 1 : kXLagDefault);
    if (s->nsys || s->herm || (s->flags & (CGAMD_UNFUSED | CGAMD_NO_GRAPH)) || lag > kLagMax || s->U % lag != 0) lag = 1;
    if (lag - 2 > s->dlag_bufs) {
        if (s->dlag) { (void)hipStreamSynchronize(s->ctx->stream); (void)hipFree(s->dlag); s->dlag = nullptr; s->dlag_bufs = 0; }
        s->dlag_pitch = ((size_t)s->n * s->nrhs * dtype_size(s->dtype) + 4095) & ~(size_t)4095;      // as in the handle's slab
        if (hipMalloc(&s->dlag, s->dlag_pitch * (size_t)(lag - 2)) == hipSuccess) s->dlag_bufs = lag - 2;
        else { (void)hipGetLastError(); s->dlag = nullptr; lag = 1; }
    }
    if (lag != s->x_lag) destroy_graphs(s);
    s->x_lag = lag;
}

// CGAMD_SPLIT_LONG_ROWS (include/cgamd.h, long_rows.hip): after finalize_spmv_plan.  The flag applies where the plan ended at kind 0
// on a single system with one right-hand side and 16-byte-aligned aValues / aCols for no other reason than its spans; everywhere else
// it changes nothing.  The lists live in s->plan.lr (copies of the plan, the multigrid's finest level among them, borrow them)
static int setup_long_rows(cgamd_solver *s) {
    const bool had = s->plan.lr.on != 0;
    free_long_rows(&s->plan.lr);
    if (had) destroy_graphs(s);
    if (!(s->flags & CGAMD_SPLIT_LONG_ROWS) || s->nsys || s->nrhs != 1 || s->plan.max_span <= 0) return CGAMD_OK;
    if (!aligned16(s->vals) || !aligned16(s->cols) || tune().dev_generic_spmv) return CGAMD_OK;
    const size_t ebytes = dtype_size(s->dtype) + 4;
    const int knob = tune().dev_long_row_bytes;
    // dev.long_row_bytes below the chunked form's cap: the handle is planned as if that cap were the knob -- a block form that could
    // stage the heavy blocks is set aside, so that small test matrices reach the split
    const bool lowered = knob > 0 && knob < kMaxChunkBytes;
    if (s->plan.kind != 0 && !(lowered && (s->plan.kind == 5 || s->plan.kind == 7))) return CGAMD_OK;
    const int heavy_entries = (int)((size_t)(lowered ? knob : kMaxChunkBytes) / ebytes);
    int seg = tune().dev_long_row_segment > 0 ? tune().dev_long_row_segment : kLongRowSegment;
    seg = std::min(seg, (int)(kLongRowMaxLds / ebytes));
    seg = std::max(seg & ~3, 4);
    LongRows lr;
    int spans[8];
    const int cycle = spmv_cycle_now(tune());
    if (int rc = build_long_rows(s->n, s->ptr, s->plan.row_blocks, heavy_entries, seg, dtype_size(s->dtype), cycle, s->ctx->stream, &lr, spans)) return rc;
    if (lr.n_heavy == 0) return CGAMD_OK;
    // the body's kernel, chosen from the regular blocks' spans by the rules of every other handle
    SpmvPlan body = s->plan;
    body.max_span = spans[0]; body.max_row = spans[7];
    for (int lv = 0; lv < 5; ++lv) body.chunk_span[lv] = spans[lv + 1];
    finalize_spmv_plan(&body, s->dtype, 1, s->n, s->nnz, s->vals, s->cols);
    if (lr.n_regular > 0 && body.kind != 5 && body.kind != 7) { free_long_rows(&lr); return CGAMD_OK; }      // (dev.spmv_chunked = 0: no form for the body)
    lr.body_kind = lr.n_regular > 0 ? body.kind : 0; lr.body_lpr = body.lpr; lr.body_max_span = body.max_span; lr.body_max_row = body.max_row;
    for (int lv = 0; lv < 5; ++lv) lr.body_chunk_span[lv] = body.chunk_span[lv];
    lr.on = 1;
    s->plan.lr = lr;
    s->plan.kind = 0; s->plan.lpr = 1; s->plan.wide = false;      // (already so unless dev.long_row_bytes lowered the threshold)
    s->plan.n_partials = s->plan.row_blocks;      // one d.q partial per 256-row block, from the body and from the combine launch alike
    return CGAMD_OK;
}

static int capture(cgamd_solver *s, int k0, int iters, hipGraph_t *g, hipGraphExec_t *ge, bool guarded = false) {
    hipStream_t st = s->ctx->stream;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
    ++s->captures;
    int rc = CGAMD_OK;
    // whole groups of the deferred x update, so that nothing is pending when the graph ends (k0 = 0 there: no parity)
    const int lag = (!guarded && iters == s->U && k0 == 0) ? x_lag_now(s) : 1;
    for (int i = 0; i < iters && rc == CGAMD_OK; ++i) rc = enqueue_iteration(s, k0 + i, st, lag, guarded ? &s->stop.view : nullptr);
    e = hipStreamEndCapture(st, g);
    if (rc != CGAMD_OK) return rc;
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(ge, *g, nullptr, nullptr, 0);
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    return CGAMD_OK;
}

// the shift history (zeta_k per shift and right-hand side) holds as many rows as the seed's history
static int ensure_shift_history(cgamd_solver *s, int cap) {
    ShiftScalars &sh = s->sh.view;
    if (!sh.S || cap <= sh.history_cap) return CGAMD_OK;
    const size_t row = dtype_size(s->dtype) * (size_t)sh.S * s->nrhs;
    void *nh = nullptr;
    if (int rc = dmalloc(&nh, (size_t)cap * row, "shift history")) return rc;
    if (sh.history) {
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        CG_HIP(hipMemcpyAsync(nh, sh.history, (size_t)sh.history_cap * row, hipMemcpyDeviceToDevice, s->ctx->stream));
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        CG_HIP(hipFree(sh.history));
    }
    sh.history = nh;
    sh.history_cap = cap;
    destroy_graphs(s);  // (as below)
    return CGAMD_OK;
}

static int ensure_history(cgamd_solver *s, int entries) {
    if (entries <= s->sc.history_cap) return ensure_shift_history(s, s->sc.history_cap);
    int cap = std::max(entries, std::max(1024, s->sc.history_cap * 2));
    const size_t vs = dtype_size(s->dtype);
    void *nh = nullptr;
    if (int rc = dmalloc(&nh, (size_t)cap * s->nrhs * vs, "history")) return rc;
    if (s->sc.history) {
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        // on the context's stream, never the legacy NULL stream: work on the NULL stream while ANOTHER thread's stream is
        // being captured is an error in that thread too ("implicit dependency on the legacy stream")
        CG_HIP(hipMemcpyAsync(nh, s->sc.history, (size_t)s->sc.history_cap * s->nrhs * vs, hipMemcpyDeviceToDevice, s->ctx->stream));
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        CG_HIP(hipFree(s->sc.history));
    }
    s->sc.history = nh;
    s->sc.history_cap = cap;
    destroy_graphs(s);  // history pointer / capacity are baked into captured kernel arguments
    return ensure_shift_history(s, cap);
}

// What a batched handle's plan holds once the pattern is known: one d.q partial per 256-row block whichever kernel of batched.hip
// runs (the vector kernels sum plan.n_partials of them per right-hand side), the cache policy priced on ALL value arrays, and none of
// the loops or codes that assume one matrix.
static void finalize_batched_plan(cgamd_solver *s) {
    s->plan.n_partials = s->plan.row_blocks;
    const size_t V = dtype_size(s->dtype), MB = (size_t)1 << 20;
    const size_t matrix_bytes = (size_t)s->nnz * (V * (size_t)s->nsys + 4) + ((size_t)s->n + 1) * 4;
    const size_t vector_bytes = (size_t)s->n * V * (size_t)s->nrhs;
    s->plan.nt = tune().spmv_nt >= 0 ? (tune().spmv_nt != 0) : (matrix_bytes > 256 * MB);      // as finalize_spmv_plan decides
    if (tune().vec_nt >= 0) s->plan.vec_nt = tune().vec_nt;
    else if (!s->plan.nt) s->plan.vec_nt = (matrix_bytes + 5 * vector_bytes <= 200 * MB) ? 0 : 3;
    else s->plan.vec_nt = (matrix_bytes <= 512 * MB) ? 0 : 3;
    s->fused2 = false;
    s->res_ok = false;
    s->resw.ok = false;
}

// nsys == 0: cgamd_solver_create; nsys >= 1: cgamd_solver_create_batched (nRHS == nsys, aValues holds nsys * nnz values)
static int create_impl(const std::string &who, cgamd_ctx *ctx, int dtype, int size, long long nnz, const void *aValues,
                       const int *aPointers, const int *aCols, int nRHS, int nsys, int flags, cgamd_solver **out) {
    if (!out) return fail(CGAMD_ERR_INVALID, who + ": out is NULL");
    *out = nullptr;
    if (!ctx) return fail(CGAMD_ERR_INVALID, who + ": ctx is NULL");
    if (dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, who + ": bad dtype");
    if (size < 1 || nnz < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, who + (nsys ? ": bad size/nnz/nSystems" : ": bad size/nnz/nRHS"));
    if (nnz > 2147483647LL - 8192) return fail(CGAMD_ERR_INVALID, who + ": nnz exceeds int32 row pointers");
    if (!aPointers || (nnz > 0 && (!aValues || !aCols))) return fail(CGAMD_ERR_INVALID, who + ": null matrix pointer");
    const size_t nmat = nsys ? (size_t)nsys : 1;      // value arrays of nnz entries behind aValues
    const bool herm = (flags & CGAMD_HERMITIAN) && (dtype == CGAMD_C64 || dtype == CGAMD_C128);     // real types: Hermitian is symmetric
    if (herm && (flags & CGAMD_UNFUSED))
        return fail(CGAMD_ERR_INVALID, who + ": CGAMD_UNFUSED replays the reference's unconjugated kernel sequence; it has no CGAMD_HERMITIAN form");
    CG_HIP(hipSetDevice(ctx->device));
    const size_t vs = dtype_size(dtype);
    cgamd_solver *s = new cgamd_solver();
    s->herm = herm;
    s->tune = tune_snapshot();
    TuneScope ts(&s->tune);
    s->ctx = ctx; s->dtype = dtype; s->n = size; s->n_user = size; s->nnz = nnz; s->nrhs = nRHS; s->nsys = nsys; s->flags = flags;
    // Row-major block + matrix-core SpMM inside the loop: by default only where the whole iteration is faster than the RHS-major
    // one (measured in one process at N = 1M, profiles/r2_experiments/spmm_ab12.log: f64 x 32 +8 %; f64 x 16, f32 x 32 equal within
    // 1 %, complex64 x 16 slower).  spmm_rowmajor = 2 takes it for every supported type, 0 never.
    const int rm_knob = tune().spmm_rowmajor;
    // (up to 32768 rows the resident loop is several times faster than any launched loop; between that and ~1M rows the chip-wide
    // resident groups take over when they apply, setup_resident_wide_plan)
    const bool rm_wins = dtype == CGAMD_F64 && nRHS == 32 && size > 32768;
    s->rm_ok = !nsys && !herm && nRHS > 1 && (rm_knob >= 2 || (rm_knob == 1 && rm_wins)) && !(flags & CGAMD_UNFUSED) && spmm_rm_supported(dtype, nRHS, size);
    if (s->rm_ok) s->rm_vgrid = rm_vec_grid((long long)size * nRHS, dtype);
    {
        const int E = (int)(16 / vs);      // values per 16-byte pack
        if (size % E != 0 && !s->rm_ok && tune().pad_rows != 0 && size < 2147483647 - 8) s->n = (size + E - 1) / E * E;
    }
    const int n_int = s->n;
    s->plan = make_spmv_plan(n_int);
    s->vgrid = vec_grid(n_int, dtype, nRHS);
    int rc = CGAMD_OK;
    std::vector<int> pad_ptr((size_t)(n_int - size), (int)nnz);      // row pointers of the appended empty rows
    if (flags & CGAMD_MATRIX_ON_DEVICE) {
        s->vals = const_cast<void *>(aValues);
        s->ptr = const_cast<int *>(aPointers);
        s->cols = const_cast<int *>(aCols);
        if (n_int != size) {
            s->ptr = nullptr;
            rc = dmalloc((void **)&s->ptr, (size_t)(n_int + 1) * 4, "aPointers (padded copy)");
            if (!rc) {
                s->own_ptr = true;
                hipError_t e = hipMemcpyAsync(s->ptr, aPointers, (size_t)(size + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(s->ptr + size + 1, pad_ptr.data(), pad_ptr.size() * 4, hipMemcpyHostToDevice, ctx->stream);
                if (e != hipSuccess) rc = fail(CGAMD_ERR_HIP, std::string("copy aPointers: ") + hipGetErrorString(e));
            }
        }
    } else {
        rc = validate_csr_host(size, nnz, aPointers, aCols);
        s->own_matrix = true;
        if (!rc) rc = dmalloc(&s->vals, (size_t)nnz * nmat * vs + 64, "aValues");
        if (!rc) rc = dmalloc((void **)&s->ptr, (size_t)(n_int + 1) * 4, "aPointers");
        if (!rc) rc = dmalloc((void **)&s->cols, (size_t)nnz * 4 + 64, "aCols");
        if (!rc && nnz) {
            hipError_t e = hipMemcpyAsync(s->vals, aValues, (size_t)nnz * nmat * vs, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(s->cols, aCols, (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) rc = fail(CGAMD_ERR_HIP, std::string("upload matrix: ") + hipGetErrorString(e));
        }
        if (!rc) {
            hipError_t e = hipMemcpyAsync(s->ptr, aPointers, (size_t)(size + 1) * 4, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess && n_int != size)
                e = hipMemcpyAsync(s->ptr + size + 1, pad_ptr.data(), pad_ptr.size() * 4, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) rc = fail(CGAMD_ERR_HIP, std::string("upload aPointers: ") + hipGetErrorString(e));
            else {
                s->ptr_host.assign(aPointers, aPointers + size + 1);
                s->ptr_host.insert(s->ptr_host.end(), pad_ptr.begin(), pad_ptr.end());
            }
        }
    }
    const size_t vbytes = (size_t)n_int * nRHS * vs;
    {
        // the five vectors live in one slab, each at a 4 KiB-aligned offset plus a per-vector skew: the update kernels
        // stream up to four of them in lock-step, and equal strides between them alias onto the same HBM channels
        const size_t pitch = (vbytes + 4095) & ~(size_t)4095;
        if (!rc) rc = dmalloc(&s->slab, pitch * 6 + 4096, "vectors");
        if (!rc && n_int != size && hipMemsetAsync(s->slab, 0, pitch * 6 + 4096, ctx->stream) != hipSuccess)     // the padding rows of b
            rc = fail(CGAMD_ERR_HIP, "hipMemsetAsync(vectors)");
        if (!rc) {
            char *base = static_cast<char *>(s->slab);
            s->x = base; s->r = base + pitch; s->d = base + 2 * pitch; s->q = base + 3 * pitch; s->b = base + 4 * pitch;
            s->d2 = base + 5 * pitch;
        }
    }
    // the row-major SpMM writes one d.q partial per work-group of its sweep: at most 8 XCDs x 32 CUs x 8 work-groups
    s->part_dq_cap = (size_t)std::max(std::max(s->plan.grid, s->plan.row_blocks), s->rm_ok ? 2048 : 0);
    if (!rc) rc = dmalloc(&s->part_dq, acc_size(dtype) * s->part_dq_cap * nRHS, "partials_dq");
    // (handles the chip-wide resident loop may take over size their vector launches one pack per thread: apply_wide_order)
    s->part_rr_cap = (size_t)std::max(std::max(s->vgrid, s->rm_vgrid), n_int <= (1 << 20) + 4096 ? (int)((n_int / (16 / vs) + kBlock - 1) / kBlock) : 0);
    if (!rc) rc = dmalloc(&s->part_rr, acc_size(dtype) * s->part_rr_cap * nRHS, "partials_rr");
    if (!rc) rc = dmalloc(&s->sc.alpha, vs * nRHS * kLagMax, "alpha");      // slot 0 is alpha; the rest: the ring of the deferred x update
    if (!rc) rc = dmalloc(&s->sc.beta, vs * nRHS, "beta");
    if (!rc) rc = dmalloc(&s->sc.delta, vs * nRHS, "delta");
    if (!rc) rc = dmalloc((void **)&s->sc.iter, 64, "iter");
    if (!rc) rc = dmalloc(&s->sc.stage, acc_size(dtype) * 32 * (size_t)nRHS, "alpha stage");
    if (!rc) rc = dmalloc((void **)&s->sc.ticket, sizeof(unsigned) * (size_t)nRHS, "alpha tickets");
    if (!rc && hipMemsetAsync(s->sc.ticket, 0, sizeof(unsigned) * (size_t)nRHS, ctx->stream) != hipSuccess) rc = fail(CGAMD_ERR_HIP, "hipMemsetAsync(alpha tickets)");
    if (!rc) rc = ensure_history(s, 1024);
    if (!rc && (flags & CGAMD_MATRIX_ON_DEVICE))      // host matrices were checked before the upload
        rc = validate_csr_device(size, nnz, size, aPointers, s->cols, nullptr, 0, 0, s->sc.iter, ctx->stream);     // the caller's arrays, as passed
    if (!rc) rc = compute_spmv_plan(s->ptr, s->cols, n_int, s->sc.iter, ctx->stream, &s->plan);
    if (!rc) finalize_spmv_plan(&s->plan, dtype, nRHS, n_int, nnz, s->vals, s->cols);
    if (!rc && (flags & CGAMD_SPLIT_LONG_ROWS)) rc = setup_long_rows(s);
    if (!rc && s->rm_ok) s->rm_nwg = spmm_rm_grid(dtype, nRHS, size, s->plan.max_quad, true);
    if (!rc && s->rm_ok) rc = dmalloc((void **)&s->rm_pace, sizeof(int) * kSpmmPaceInts, "spmm pace counters");
    if (!rc && s->rm_ok && hipMemsetAsync(s->rm_pace, 0, sizeof(int) * kSpmmPaceInts, ctx->stream) != hipSuccess) rc = fail(CGAMD_ERR_HIP, "hipMemsetAsync(spmm pace counters)");
    if (!rc && nsys) finalize_batched_plan(s);
    if (!rc && !nsys) s->fused2 = !s->herm && fused2_ok(s->plan, dtype, nRHS, s->vals, s->cols);
    if (!rc && !nsys) rc = setup_resident(s);
    if (!rc && !nsys) rc = setup_index_codes(s);
    if (!rc) setup_x_lag(s);
    if (!rc) {
        hipError_t e = hipStreamSynchronize(ctx->stream);  // host matrix arrays may go away after return
        if (e != hipSuccess) rc = fail(CGAMD_ERR_HIP, who + " sync: " + hipGetErrorString(e));
    }
    if (rc) {
        std::string keep = cgamd_last_error();
        cgamd_solver_destroy(s);
        set_error(keep);
        return rc;
    }
    *out = s;
    return CGAMD_OK;
}

// a batched handle (cgamd_solver_create_batched) has a matrix per right-hand side: one M shared by all of them preconditions none
int cgamd::batched_refuses(const char *who) {
    return fail(CGAMD_ERR_STATE, std::string(who) + ": the handle is batched (a matrix of its own per right-hand side); a preconditioner "
                                                    "shared by all right-hand sides has no meaning for different systems");
}
// what a CGAMD_HERMITIAN handle does not serve: refused before anything on the handle changes
int cgamd::herm_refuses(const char *who, const char *why) {
    return fail(CGAMD_ERR_STATE, std::string(who) + ": the handle runs the conjugated recurrence (CGAMD_HERMITIAN), " + why);
}
// with shifts in force (cgamd_solver_set_shifts) the handle serves the unpreconditioned recurrence from x0 = 0 alone: a preconditioned
// operator is not a shift of anything.  Refused before anything on the handle changes
int cgamd::block_refuses(const cgamd_solver *s, const char *who) {
    if (!s->blk_want) return CGAMD_OK;
    if (s->blk_pcg)
        return fail(CGAMD_ERR_STATE, std::string(who) + ": preconditioned block CG is on (cgamd_solver_set_block_pcg), which this entry does not serve -- M is part of its state; turn it off first");
    return fail(CGAMD_ERR_STATE, std::string(who) + ": block CG is on (cgamd_solver_set_block), which this entry does not serve; turn it off first");
}
// block CG goes, in either mode: the next set_rhs starts a handle that never had it.  The caller has waited for the stream
void cgamd::block_drop(cgamd_solver *s) {
    block_free(&s->blk);
    destroy_graphs(s);
    s->blk_want = s->blk_on = s->blk_pcg = false;
    s->rhs_set = false;     // (r and d hold Q and P)
    s->until_mode = s->until_stopped = false;
}
int cgamd::shifts_refuse(const cgamd_solver *s, const char *who, bool block_too) {
    if (!s->sh.view.S) return block_too ? block_refuses(s, who) : CGAMD_OK;
    return fail(CGAMD_ERR_STATE, std::string(who) + ": shifts are in force (cgamd_solver_set_shifts), which this entry does not serve; remove them first");
}
extern "C" {

int cgamd_solver_create(cgamd_ctx *ctx, int dtype, int size, long long nnz, const void *aValues, const int *aPointers,
                        const int *aCols, int nRHS, int flags, cgamd_solver **out) {
    return create_impl("solver_create", ctx, dtype, size, nnz, aValues, aPointers, aCols, nRHS, 0, flags, out);
}

int cgamd_solver_create_batched(cgamd_ctx *ctx, int dtype, int size, long long nnz, const void *aValues, const int *aPointers,
                                const int *aCols, int nSystems, int flags, cgamd_solver **out) {
    if (out) *out = nullptr;
    if (nSystems < 1) return fail(CGAMD_ERR_INVALID, "solver_create_batched: nSystems must be at least 1");
    return create_impl("solver_create_batched", ctx, dtype, size, nnz, aValues, aPointers, aCols, nSystems, nSystems, flags, out);
}

int cgamd_solver_systems(cgamd_solver *s) { return s ? s->nsys : -CGAMD_ERR_INVALID; }
int cgamd_solver_hermitian(cgamd_solver *s) { return s ? (s->herm ? 1 : 0) : -CGAMD_ERR_INVALID; }

static int step_not_capturing(cgamd_solver *s, const char *who) { return stream_not_capturing(s->ctx->stream, who); }

// New matrix VALUES / PATTERN of the same size into an existing handle (host arrays; the handle must own its matrix):
// what the stateless cg() needs to reuse its cached device state -- allocations, stream, captured graphs -- from one call
// to the next.  The pattern-dependent plan is recomputed only when the row pointers differ from the ones uploaded before.
int cgamd_solver_reload_matrix(cgamd_solver *s, const void *aValues, const int *aPointers, const int *aCols) {
    if (!s || !aPointers || (s->nnz > 0 && (!aValues || !aCols))) return fail(CGAMD_ERR_INVALID, "reload_matrix: null argument");
    if (!s->own_matrix) return fail(CGAMD_ERR_STATE, "reload_matrix: the handle borrows a device matrix");
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = validate_csr_host(s->n_user, s->nnz, aPointers, aCols)) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t vs = dtype_size(s->dtype);
    s->rhs_set = false;
    proj_clear(s);
    if (s->nnz) {
        CG_HIP(hipMemcpyAsync(s->vals, aValues, (size_t)s->nnz * (s->nsys ? (size_t)s->nsys : 1) * vs, hipMemcpyHostToDevice, st));
        CG_HIP(hipMemcpyAsync(s->cols, aCols, (size_t)s->nnz * 4, hipMemcpyHostToDevice, st));
    }
    const bool same_ptr = s->ptr_host.size() == (size_t)s->n + 1 && memcmp(s->ptr_host.data(), aPointers, ((size_t)s->n_user + 1) * 4) == 0;
    if (!same_ptr) {
        // (the row pointers of the appended empty rows all equal nnz, which does not change: they stay as uploaded at creation)
        CG_HIP(hipMemcpyAsync(s->ptr, aPointers, ((size_t)s->n_user + 1) * 4, hipMemcpyHostToDevice, st));
        std::copy(aPointers, aPointers + s->n_user + 1, s->ptr_host.begin());
        destroy_graphs(s);          // kernel choice, LDS size and partial counts are baked into the captured launches
        const LongRows old_lists = s->plan.lr;      // (the handle's: setup_long_rows frees them and builds the new pattern's)
        s->plan = make_spmv_plan(s->n);
        s->plan.lr = old_lists;
        if (int rc = compute_spmv_plan(s->ptr, s->cols, s->n, s->sc.iter, st, &s->plan)) return rc;
        finalize_spmv_plan(&s->plan, s->dtype, s->nrhs, s->n, s->nnz, s->vals, s->cols);
        if (s->flags & CGAMD_SPLIT_LONG_ROWS)
            if (int rc = setup_long_rows(s)) return rc;
        if ((size_t)std::max(s->plan.grid, s->plan.row_blocks) > s->part_dq_cap) return fail(CGAMD_ERR_STATE, "reload_matrix: partial buffer too small");
        if (s->rm_ok) s->rm_nwg = spmm_rm_grid(s->dtype, s->nrhs, s->n, s->plan.max_quad, true);
        s->fused2 = !s->herm && fused2_ok(s->plan, s->dtype, s->nrhs, s->vals, s->cols);
        if (s->nsys) finalize_batched_plan(s);
    }
    if (s->nsys) {                                  // no resident loop, no codes; a per-system preconditioner built from the matrices follows them
        CG_HIP(hipStreamSynchronize(st));
        return rebuild_or_remove(s, "reload_matrix");
    }
    if (int rc = setup_resident(s)) return rc;      // also with unchanged row pointers: the column range of a row slice may have moved
    {                                               // the columns were replaced: their codes go with them
        const bool had = s->codes != nullptr;
        if (had) destroy_graphs(s);                 // captured launches hold the old code array
        if (int rc = setup_index_codes(s)) return rc;
        if (!had && s->codes) destroy_graphs(s);
    }
    setup_x_lag(s);                     // (the default rule follows the number of d.q partials and the resident plan)
    CG_HIP(hipStreamSynchronize(st));   // the host arrays may go away after return
    return rebuild_or_remove(s, "reload_matrix");       // a preconditioner built from the matrix follows it
}

// New VALUES on the SAME pattern (include/cgamd.h): everything made from the values follows them -- the value, joint and row-pattern
// codes and a preconditioner built from the matrix -- and nothing made from the pattern alone is touched (no validation, no plan, no
// resident scan, no x lag, the column codes stay).  Returns the outcome through s->last_refresh.
static int refresh_codes(cgamd_solver *s) {
    s->last_refresh = 0;
    if (!value_codes_apply(s) || s->nnz <= 0) return CGAMD_OK;
    if (s->vcodes) {        // classes intact: the dictionaries are rewritten in place, arrays, pointers and captured graphs stay
        bool kept = false;
        if (int rc = refresh_value_dicts(s->dtype, s->nnz, s->vals, s->vcodes, s->vdict, s->n_pairs, s->jcodes ? s->jdict_off : nullptr,
                                         s->jcodes ? s->jdict_val : nullptr, s->n_patterns, s->rcodes ? s->rdict : nullptr, s->ctx->stream, &kept)) {
            destroy_graphs(s);      // (what the dictionaries hold is unknown: the SpMV reads aValues)
            drop_value_codes(s);
            return rc;
        }
        if (kept && s->pdict) {     // the pair dictionary's values follow rdict's, in place too
            if (int rc = refresh_pair_dict(s->dtype, s->n_pair_patterns, s->rdict, s->pdict, s->ctx->stream)) {
                destroy_graphs(s);
                drop_value_codes(s);
                return rc;
            }
        }
        if (kept) { s->last_refresh = 1; return CGAMD_OK; }
    }
    const bool had = s->vcodes != nullptr;
    if (had) destroy_graphs(s);     // captured launches hold the old code arrays
    drop_value_codes(s);
    const int rc = setup_value_codes(s);
    if (!had && s->vcodes) destroy_graphs(s);
    if (rc) { drop_value_codes(s); return rc; }
    s->last_refresh = s->vcodes ? 2 : 3;
    return CGAMD_OK;
}
int cgamd_solver_refresh_values(cgamd_solver *s, const void *aValues, int on_device) {
    if (!s) return fail(CGAMD_ERR_INVALID, "refresh_values: solver is NULL");
    if (s->own_matrix && !aValues) return fail(CGAMD_ERR_INVALID, "refresh_values: the handle owns its matrix: aValues is NULL");
    if (!s->own_matrix && aValues && (aValues != s->vals || !on_device))
        return fail(CGAMD_ERR_INVALID, "refresh_values: the handle borrows its value array (CGAMD_MATRIX_ON_DEVICE): copy the new values into "
                                       "that array and pass NULL (or the array itself, on_device = 1); borrowing another array needs a new handle");
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (int rc = stream_not_capturing(st, "refresh_values")) return rc;
    s->rhs_set = false;
    s->last_refresh = 0;
    proj_clear(s);
    CG_HIP(hipStreamSynchronize(st));       // nothing of the handle's still reads the old values
    if (s->own_matrix && s->nnz) {
        const size_t bytes = (size_t)s->nnz * (s->nsys ? (size_t)s->nsys : 1) * dtype_size(s->dtype);
        CG_HIP(hipMemcpyAsync(s->vals, aValues, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        CG_HIP(hipStreamSynchronize(st));   // the caller's array may go away (or change) after return
    }
    if (int rc = refresh_codes(s)) {        // the values are in force, read as they are; factors of the old ones must not stay
        s->last_refresh = -rc;
        return remove_and_fail(s, rc);
    }
    return rebuild_or_remove(s, "refresh_values");      // a preconditioner built from the matrix follows it
}
int cgamd_solver_last_refresh(cgamd_solver *s) { return s ? s->last_refresh : -CGAMD_ERR_INVALID; }
int cgamd_solver_graph_captures(cgamd_solver *s) { return s ? s->captures : -CGAMD_ERR_INVALID; }

int cgamd_solver_destroy(cgamd_solver *s) {
    if (!s) return CGAMD_OK;
    thread_hip_setup();
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    destroy_graphs(s);
    precond_drop(&s->pre);
    proj_free(s);
    shifts_free(s);
    block_free(&s->blk);
    free_long_rows(&s->plan.lr);
    if (s->own_ptr && s->ptr) (void)hipFree(s->ptr);
    if (s->own_matrix) {
        if (s->vals) (void)hipFree(s->vals);
        if (s->ptr) (void)hipFree(s->ptr);
        if (s->cols) (void)hipFree(s->cols);
    }
    void *bufs[] = {s->slab, s->part_dq, s->part_rr, s->sc.alpha, s->sc.beta, s->sc.delta,
                    s->sc.history, s->sc.iter, s->part_rz, s->pre.rho2, s->sc.stage, s->sc.ticket, s->res_sync, s->resw_sync, s->dlag, s->codes, s->dict, s->rm_pace, s->vcodes, s->vdict, s->jcodes, s->jdict_off, s->jdict_val, s->rcodes, s->rdict, s->pcodes, s->pdict, s->sched};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    stop_run_free(s->stop);
    delete s;
    return CGAMD_OK;
}

// set_rhs with the caller's blocks at leading dimension ldb (the public entry: `size`).  b == NULL (the mixed solve's outer handle,
// mixed.cpp): b and x stay what the handle holds -- x as a caller of cgamd_solver_vector left it -- and the recurrence starts from
// them with the same launches, so the bits are those of set_rhs(b, x)
static int set_rhs_impl(cgamd_solver *s, const void *b, const void *x0, int on_device, long long ldb) {
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const size_t vbytes = (size_t)s->n * s->nrhs * dtype_size(s->dtype);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const bool rm = s->rm_ok && !precond_set(s);      // the preconditioned recurrence keeps the RHS-major kernels
    if (rm && (!b || ldb != s->n_user)) return fail(CGAMD_ERR_STATE, "the handle keeps its right-hand sides interleaved (row-major layout)");
    if (rm != s->rm) destroy_graphs(s);         // captured launch sequences belong to one layout
    const bool blk = s->blk_want;               // block CG takes effect here, and goes here
    if (blk && rm) return fail(CGAMD_ERR_STATE, "set_rhs: block CG is on (cgamd_solver_set_block), which the row-major layout does not serve");
    if (blk != s->blk_on) destroy_graphs(s);
    s->blk_on = blk;
    // (captured while the two-launch loop was set aside: iterate_until; with shifts in force or block CG on it stays set aside)
    if (s->until_mode && s->fused2 && !nshifts(s) && !blk) destroy_graphs(s);
    s->until_mode = nshifts(s) > 0 || blk;
    s->until_stopped = s->stop.armed = false;
    s->proj.projected = s->proj.spent = false;      // (cgamd_solver_set_rhs_projected sets its mark after this call)
    s->rm = rm;
    int rc;
    if (rm) {
        // caller's blocks are RHS-major [nrhs][n] (reference spmv.cl:25,48); the handle keeps [n][nrhs]: q is the staging area
        CG_HIP(hipMemcpyAsync(s->q, b, vbytes, kind, st));
        if ((rc = launch_transpose(s->dtype, s->nrhs, s->n, s->q, s->b, st))) return rc;
        if (x0) {
            CG_HIP(hipMemcpyAsync(s->q, x0, vbytes, kind, st));
            if ((rc = launch_transpose(s->dtype, s->nrhs, s->n, s->q, s->x, st))) return rc;
        } else {
            CG_HIP(hipMemsetAsync(s->x, 0, vbytes, st));
        }
        // r = b - A x0 ; d = r ; delta0 = r.r   (clcg.c:255-292)
        if ((rc = launch_spmm_rm(s->dtype, s->n, s->nnz, s->vals, s->ptr, s->cols, s->x, s->q, s->nrhs, nullptr, s->plan.max_quad, s->rm_pace, st))) return rc;
        if ((rc = launch_sub(s->dtype, s->n * s->nrhs, s->b, s->q, s->r, (long long)s->n * s->nrhs, 1, st))) return rc;
        CG_HIP(hipMemcpyAsync(s->d, s->r, vbytes, hipMemcpyDeviceToDevice, st));
        if ((rc = launch_rm_dot(s->dtype, s->n, s->nrhs, s->r, s->r, s->part_rr, s->rm_vgrid, st))) return rc;
        if ((rc = launch_cg_delta0(s->dtype, s->part_rr, s->rm_vgrid, s->nrhs, s->sc, st))) return rc;
        if (!on_device) CG_HIP(hipStreamSynchronize(st));
        s->rhs_set = true;
        s->iters = 0;
        return CGAMD_OK;
    }
    if (!b) {                    // (restart: b and x are in place)
    } else if (s->n != ldb) {    // caller's blocks are [nrhs][size]; the handle's carry the padding rows (b and x stay 0 there)
        const size_t vs = dtype_size(s->dtype);
        CG_HIP(hipMemcpy2DAsync(s->b, (size_t)s->n * vs, b, (size_t)ldb * vs, (size_t)s->n_user * vs, (size_t)s->nrhs, kind, st));
        CG_HIP(hipMemsetAsync(s->x, 0, vbytes, st));
        if (x0) CG_HIP(hipMemcpy2DAsync(s->x, (size_t)s->n * vs, x0, (size_t)ldb * vs, (size_t)s->n_user * vs, (size_t)s->nrhs, kind, st));
    } else {
        CG_HIP(hipMemcpyAsync(s->b, b, vbytes, kind, st));
        if (x0) CG_HIP(hipMemcpyAsync(s->x, x0, vbytes, kind, st));
        else CG_HIP(hipMemsetAsync(s->x, 0, vbytes, st));
    }
    // r = b - A x0 ; d = r ; delta0 = r.r   (clcg.c:255-292)
    if ((rc = handle_spmv(s, s->n, s->x, s->n, s->q, s->n, nullptr, nullptr, st))) return rc;
    if ((rc = launch_sub(s->dtype, s->n, s->b, s->q, s->r, s->n, s->nrhs, st))) return rc;
    if (s->blk_on && s->blk_pcg) {     // Z0 = M^-1 R0 into q; C = R0^T Z0 = L L^T, xi = L^T, Q = R0 xi^-1 over r, P = Z0 xi^-1, delta_0[j] = (R0^T R0)_jj
        const BlockState &bk = s->blk;
        if (!block_pcg_state_ok(s)) return fail(CGAMD_ERR_STATE, "set_rhs: the handle is not in the state preconditioned block CG was set up for");
        if ((rc = launch_block_gram(s->dtype, s->n, s->n, s->nrhs, s->r, s->r, bk.dev.partials, bk.grid, nullptr, st))) return rc;
        if ((rc = enqueue_block_pcg_wz(s, nullptr, st))) return rc;
        if ((rc = launch_block_pcg_small(s->dtype, 0, bk, s->sc, nullptr, st))) return rc;
        if ((rc = enqueue_block_pcg_qp(s, true, bk.dev.rec + 2, st))) return rc;
    } else if (s->blk_on) {   // C = R0^T R0 = L L^T, xi = L^T, Q = R0 xi^-1 over r, P = Q, delta_0[j] = |xi e_j|^2; a dependent block freezes here
        const BlockState &bk = s->blk;
        if ((rc = launch_block_gram(s->dtype, s->n, s->n, s->nrhs, s->r, s->r, bk.dev.partials, bk.grid, nullptr, st))) return rc;
        if ((rc = launch_block_small(s->dtype, 0, bk, s->sc, nullptr, st))) return rc;
        if ((rc = launch_block_qp(s->dtype, s->n, s->n, s->nrhs, s->r, s->d, bk.dev.tinv_T, bk.dev.tau_T, true, bk.dev.rec + 2, st))) return rc;
    } else if (s->herm) {    // d0 = r0 (d0 = m .* r0), dc = conj(d0), delta0 = r0^H r0, rho0 (hermitian.hip)
        if ((rc = launch_herm_init(s->dtype, s->n, s->r, s->d, s->d2, s->pre.mdiag, m_pitch(s), s->n, s->nrhs, s->part_rz, s->part_rr, s->vgrid, st))) return rc;
        if ((rc = launch_herm_delta0(s->dtype, s->pre.mdiag != nullptr, s->part_rz, s->part_rr, s->vgrid, s->nrhs, s->sc, s->pre.rho2, st))) return rc;
    } else if (s->pre.mg) {      // z0 = V-cycle(r0), p0 = z0, rho0 = r0.z0; the partials by the launches of an iteration
        if ((rc = mg_vcycle(s->pre.mg, s->r, s->d, st))) return rc;
        if ((rc = launch_dot_partials(s->dtype, s->n, s->r, s->r, s->n, s->nrhs, s->part_rr, s->vgrid, st))) return rc;
        if ((rc = launch_dot_partials(s->dtype, s->n, s->r, s->d, s->n, s->nrhs, s->part_rz, s->vgrid, st))) return rc;
        if ((rc = launch_pcg_delta0(s->dtype, s->part_rz, s->part_rr, s->vgrid, s->nrhs, s->sc, s->pre.rho2, st))) return rc;
    } else if (tri_on(s)) {  // z0 = M^-1 r0 (the line sweeps), p0 = z0, rho0 = r0.z0
        if ((rc = enqueue_tri_sweep(s, false, nullptr, s->d, st))) return rc;
        const PcgPartials p = tri_partials(s);
        if ((rc = launch_pcg_delta0(s->dtype, p.rz, p.rr, s->pre.tri.grid, s->nrhs, s->sc, s->pre.rho2, st))) return rc;
    } else if (s->pre.mdiag) {   // z0 = M r0, p0 = z0, rho0 = r0.z0 (helmFE_var.py:562-573)
        if ((rc = launch_pcg_axpy2_dot2(s->dtype, true, s->n, s->d, s->x, s->q, s->r, s->pre.mdiag, s->n, nullptr, s->nrhs, s->part_rz,
                                        s->part_rr, s->vgrid, st, m_pitch(s)))) return rc;
        if ((rc = launch_pcg_delta0(s->dtype, s->part_rz, s->part_rr, s->vgrid, s->nrhs, s->sc, s->pre.rho2, st))) return rc;
    } else {
        CG_HIP(hipMemcpyAsync(s->d, s->r, vbytes, hipMemcpyDeviceToDevice, st));
        if ((rc = launch_dot_partials(s->dtype, s->n, s->r, s->r, s->n, s->nrhs, s->part_rr, s->vgrid, st))) return rc;
        if ((rc = launch_cg_delta0(s->dtype, s->part_rr, s->vgrid, s->nrhs, s->sc, st))) return rc;
        if (nshifts(s)) {   // x_j = 0, d_j = r_0 = b (x0 = 0), theta = zeta = 1: every shifted system starts where the seed does
            const size_t sbytes = vbytes * (size_t)nshifts(s);
            CG_HIP(hipMemsetAsync(shift_xs(s), 0, sbytes, st));
            for (int j = 0; j < nshifts(s); ++j)
                CG_HIP(hipMemcpyAsync(static_cast<char *>(shift_ds(s)) + (size_t)j * vbytes, s->r, vbytes, hipMemcpyDeviceToDevice, st));
            if ((rc = launch_shift_init(s->dtype, s->nrhs, s->sh.view, st))) return rc;
        }
    }
    if (!on_device) CG_HIP(hipStreamSynchronize(st));  // host buffers may be released by the caller
    s->rhs_set = true;
    s->iters = 0;
    return CGAMD_OK;
}
int cgamd_solver_set_rhs(cgamd_solver *s, const void *b, const void *x0, int on_device) {
    if (!s || !b) return fail(CGAMD_ERR_INVALID, "set_rhs: null argument");
    if (nshifts(s) && x0) return fail(CGAMD_ERR_INVALID, "set_rhs: shifts are in force (cgamd_solver_set_shifts), and the shifted systems share a Krylov space with the seed only from x0 = 0: pass x0 = NULL");
    return set_rhs_impl(s, b, x0, on_device, s->n_user);
}


int cgamd_solver_iterate(cgamd_solver *s, int nIterations) {
    if (!s) return fail(CGAMD_ERR_INVALID, "iterate: solver is NULL");
    TuneScope ts(&s->tune);
    if (!s->rhs_set) return fail(CGAMD_ERR_STATE, "iterate: call set_rhs first");
    if (nIterations < 0) return fail(CGAMD_ERR_INVALID, "iterate: negative iteration count");
    if (s->until_stopped) return fail(CGAMD_ERR_STATE, "iterate: iterate_until has stopped a right-hand side (the columns are at different iterations): go on with iterate_until, or call set_rhs");
    if (s->proj.spent) return fail(CGAMD_ERR_STATE, std::string("iterate") + kProjSpent);
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = ensure_history(s, s->iters + nIterations + 1)) return rc;
    hipStream_t st = s->ctx->stream;
    int left = nIterations, k = s->iters;
    const bool use_graph = !(s->flags & CGAMD_NO_GRAPH) && !s->graph_failed;
    const bool two = fused2_now(s);
    if (s->resw.ok && !s->until_mode && !tri_on(s) && !s->pre.mg && !(two && s->res_ok) && !s->rm && !(s->flags & (CGAMD_NO_GRAPH | CGAMD_UNFUSED)) &&
        (nIterations >= std::max(1, tune().resident_wide_min) || s->tol_req > 0.)) {
        // one chip-wide resident group (single right-hand side, matrix rows in registers).  d ping-pongs inside the launch; handles
        // of the launched loops that keep d in one buffer get it back there, and the launched loops' r.r partials are rebuilt.
        const bool keeps_new_d = !two;       // three / four-launch loops: between iterations d already is beta d + r
        // a launch stays around a second at most (groups solve their right-hand sides in turn, ~10 us per iteration)
        const int rounds_w = (s->nrhs + s->resw.NG - 1) / s->resw.NG, kmax_w = std::min(1 << 15, std::max(64, 100000 / rounds_w));
        for (int left = nIterations; left > 0;) {
            const int K = std::min(left, kmax_w);
            void *cur = dbuf(s, s->iters), *other = cur == s->d ? s->d2 : s->d;
            void *d0 = (s->iters & 1) ? other : cur, *d1 = (s->iters & 1) ? cur : other;
            bool untouched = false;
            int stop = -1;
            s->tol_served = s->tol_req > 0.;
            CgScalars scw = s->sc;           // the Jacobi-preconditioned recurrence runs in the same loop (rho for delta, z = m r)
            if (s->pre.mdiag) { scw.pcg_m = s->pre.mdiag; scw.pcg_rho2 = s->pre.rho2; }
            if (int rc = run_cg_resident_wide(s->dtype, s->resw, s->n, s->nrhs, s->vals, s->ptr, s->cols, s->x, s->r, d0, d1,
                                              keeps_new_d && s->iters > 0, scw, s->iters, K, s->resw_sync, s->n_cus, st, &untouched, s->tol_req,
                                              &stop)) {
                if (!untouched) {            // x / r / d / delta may be partly advanced: the handle demands a fresh set_rhs
                    s->rhs_set = false;
                    s->resw.ok = false;
                    return rc;
                }
                s->resw.ok = false;          // the chip is shared with something that does not yield: this handle keeps the launched loops
                if (int rc2 = launch_dot_partials(s->dtype, s->n, s->r, s->r, s->n, s->nrhs, s->part_rr, s->vgrid, st)) return rc2;
                if (s->tol_req > 0.) { s->tol_served = false; return rc; }      // (the launched loops have no device-side stop: the caller checks from the host)
                return cgamd_solver_iterate(s, left);
            }
            const int done = stop >= 0 ? stop - s->iters : K;      // the tolerance may end the solve before K iterations
            void *fin = ((s->iters + done) & 1) ? d1 : d0;
            s->iters += done;
            left = stop >= 0 ? 0 : left - K;
            s->tol_stopped = stop >= 0;
            if (done > 0) {                  // (a stop before the first iteration leaves d as the caller had it)
                if (fin != dbuf(s, s->iters))
                    CG_HIP(hipMemcpyAsync(dbuf(s, s->iters), fin, (size_t)s->n * s->nrhs * dtype_size(s->dtype), hipMemcpyDeviceToDevice, st));
                if (s->pre.mdiag) {              // p = beta p + m r (helmFE_var.py:583-585)
                    if (int rc = launch_pcg_p_update(s->dtype, s->n, s->r, dbuf(s, s->iters), s->pre.mdiag, s->n, s->sc.beta, s->nrhs, st)) return rc;
                } else if (keeps_new_d)      // d = beta d + r with the beta the launch recorded last (clcg.c:415)
                    if (int rc = launch_aypx(s->dtype, s->n, s->r, dbuf(s, s->iters), s->n, s->sc.beta, s->nrhs, st)) return rc;
            }
        }
        return launch_dot_partials(s->dtype, s->n, s->r, s->r, s->n, s->nrhs, s->part_rr, s->vgrid, st);
    }
    if (two && s->res_ok && !(s->flags & CGAMD_NO_GRAPH) && (nIterations >= std::max(1, tune().resident_min) || s->tol_req > 0.)) {
        // small system: the whole call in one launch per 2^15 iterations (resident.hip; a launch stays well below the bound of its
        // waits); same state, same bits as the loop below
        const int groups_r = std::max(1, 8 * s->res.lg), rounds_r = (s->nrhs + groups_r - 1) / groups_r;
        const int kmax_r = std::min(1 << 15, std::max(64, 200000 / rounds_r));      // a launch stays around a second at most
        for (int left = nIterations; left > 0;) {
            const int K = std::min(left, kmax_r);
            bool untouched = false;
            int stop = -1;
            s->tol_served = s->tol_req > 0.;
            if (int rc = run_cg_resident(s->dtype, s->res, s->n, s->nrhs, s->vals, s->ptr, s->cols, s->x, s->r, s->d, s->d2, s->part_rr,
                                         s->vgrid, s->plan.n_partials, s->sc, s->iters, K, s->res_sync, s->n_cus, st, &untouched, s->tol_req, &stop)) {
                if (!untouched) {            // (see above)
                    s->rhs_set = false;
                    s->res_ok = false;
                    return rc;
                }
                s->res_ok = false;           // no group could form (CUs held by other work): this handle keeps the launched loops
                if (s->tol_req > 0.) { s->tol_served = false; return rc; }
                return cgamd_solver_iterate(s, left);
            }
            if (stop >= 0) {             // the tolerance ended the solve: the launched loops' r.r partials of that state are rebuilt
                s->iters = stop;
                s->tol_stopped = true;
                return launch_dot_partials(s->dtype, s->n, s->r, s->r, s->n, s->nrhs, s->part_rr, s->vgrid, st);
            }
            s->iters += K;
            left -= K;
        }
        return CGAMD_OK;
    }
    // graphs start at a fixed parity of the iteration count (d ping-pongs in the two-launch loop; U is even)
    while (use_graph && !s->graph_failed && left > 0) {
        const int par = two ? (k & 1) : 0;
        const bool big = left >= s->U;
        hipGraphExec_t &ge = big ? s->gU[par] : s->g1[par];
        if (!ge && capture(s, par, big ? s->U : 1, big ? &s->gUg[par] : &s->g1g[par], &ge) != CGAMD_OK) {
            s->graph_failed = true;
            destroy_graphs(s);
            break;
        }
        CG_HIP(hipGraphLaunch(ge, st));
        left -= big ? s->U : 1;
        k += big ? s->U : 1;
    }
    for (; left > 0; --left, ++k)
        if (int rc = enqueue_iteration(s, k, st)) {
            s->iters = k + 1;      // the device counter may have advanced for the broken iteration too
            return rc;
        }
    s->iters = k;
    if (two && nIterations > 0) return launch_cg_tail(s->dtype, s->part_rr, s->vgrid, s->nrhs, s->sc, st);
    return CGAMD_OK;
}

// Tolerance-stopping run ON THE DEVICE (one right-hand side, handles that take a resident loop): iterations until
// sqrt|r.r| < tol (or NaN), at most maxIterations -- the reference's NumPy sub-solver with `tol` (p_h-PY_C-CL.py:1338-1369) and
// PCG's stopping rule without preconditioner (helmFE_var.py:575-577).  Every member of the resident group sees the same delta and
// leaves the loop in the same iteration, so x is the iterate of exactly *iterations_run iterations; no read-back per check, no
// re-run.  CGAMD_ERR_STATE when the handle has no resident loop (the caller then checks the history from the host).
int cgamd_solver_iterate_tol(cgamd_solver *s, int maxIterations, double tol, int *iterations_run) {
    if (!s || !iterations_run) return fail(CGAMD_ERR_INVALID, "iterate_tol: null argument");
    if (!(tol > 0.) || maxIterations < 0) return fail(CGAMD_ERR_INVALID, "iterate_tol: tol must be positive, maxIterations >= 0");
    if (s->nsys) return fail(CGAMD_ERR_STATE, "iterate_tol: a batched handle runs a launched loop (check the history from the host)");
    if (s->herm) return herm_refuses("iterate_tol", "which has no resident loop: use cgamd_solver_iterate_until");
    if (int rc = shifts_refuse(s, "iterate_tol")) return rc;
    if (!s->rhs_set) return fail(CGAMD_ERR_STATE, "iterate_tol: call set_rhs first");
    if (s->nrhs != 1) return fail(CGAMD_ERR_STATE, "iterate_tol: one right-hand side");
    if (s->until_mode) return fail(CGAMD_ERR_STATE, "iterate_tol: iterate_until runs this right-hand side on the launched loop until the next set_rhs");
    if (s->proj.spent) return fail(CGAMD_ERR_STATE, std::string("iterate_tol") + kProjSpent);
    {
        TuneScope ts(&s->tune);
        const bool local = fused2_now(s) && s->res_ok, wide = s->resw.ok && !tri_on(s) && !s->pre.mg && !s->rm && !(s->res_ok && !precond_set(s));
        if ((!local && !wide) || (s->flags & (CGAMD_NO_GRAPH | CGAMD_UNFUSED)))
            return fail(CGAMD_ERR_STATE, "iterate_tol: this handle runs a launched loop (check the history from the host)");
    }
    const int start = s->iters;
    s->tol_req = tol;
    s->tol_served = s->tol_stopped = false;
    int rc = maxIterations > 0 ? cgamd_solver_iterate(s, maxIterations) : CGAMD_OK;
    const bool served = s->tol_served || maxIterations == 0;
    s->tol_req = 0.;
    if (rc) return rc;
    if (!served) return fail(CGAMD_ERR_STATE, "iterate_tol: the resident loop was not available for this call");
    *iterations_run = s->iters - start;
    return CGAMD_OK;
}


// From here to the next set_rhs the handle runs its three / four-launch loop only, d in ONE buffer and final in memory (what
// cgamd_solver_iterate_until and cgamd_solver_replace_residual share)
static int enter_until_mode(cgamd_solver *s, hipStream_t st) {
    if (s->until_mode) return CGAMD_OK;
    if (fused2_now(s) && s->iters > 0) {
        // the two-launch loop (and the resident loops that stand in for it) leave d = beta d + r of the last iteration to the
        // next SpMV launch: done here with the beta that iteration recorded, the very expression (vaypx), into the one buffer
        void *cur = dbuf(s, s->iters);
        if (int rc = launch_aypx(s->dtype, s->n, s->r, cur, s->n, s->sc.beta, s->nrhs, st)) return rc;
        if (cur != s->d) CG_HIP(hipMemcpyAsync(s->d, cur, (size_t)s->n * s->nrhs * dtype_size(s->dtype), hipMemcpyDeviceToDevice, st));
    }
    if (s->fused2) destroy_graphs(s);       // captured per parity of the two-launch loop
    s->until_mode = true;
    return CGAMD_OK;
}

// Residual replacement (include/cgamd.h; the "reliable updates" of van der Vorst and Ye): the recurrence goes on from (0, r_new, d).
// What the entry does not serve is refused before anything on the handle changes.  planned: the question is asked BEFORE the set_rhs
// that will precede the call (the mixed solve, mixed.cpp), so the layout is the one that set_rhs will decide
static int replace_refuses(const cgamd_solver *s, bool planned) {
    const std::string who = "replace_residual: ";
    if (!planned && !s->rhs_set) return fail(CGAMD_ERR_STATE, who + "call set_rhs first");
    if (planned ? (s->rm_ok && !precond_set(s)) : s->rm)
        return fail(CGAMD_ERR_STATE, who + "the handle keeps its right-hand sides interleaved (row-major layout)");
    if (tri_on(s)) return fail(CGAMD_ERR_STATE, who + "a tridiagonal / line preconditioner is set; the entry serves no preconditioner or a diagonal one");
    if (s->pre.mg) return fail(CGAMD_ERR_STATE, who + "a multigrid preconditioner is set; the entry serves no preconditioner or a diagonal one");
    if (s->herm) return herm_refuses("replace_residual", "which the entry does not serve");
    if (int rc = block_refuses(s, "replace_residual")) return rc;
    if (s->nsys) return fail(CGAMD_ERR_STATE, who + "the handle is batched");
    if (s->flags & CGAMD_UNFUSED) return fail(CGAMD_ERR_STATE, who + "CGAMD_UNFUSED replays the reference's kernel sequence");
    return CGAMD_OK;
}
// r_new at leading dimension ldr: `size` (the public entry), or the handle's own with zero padding rows (mixed.cpp)
static int replace_residual_impl(cgamd_solver *s, const void *r_new, long long ldr) {
    TuneScope ts(&s->tune);
    if (int rc = replace_refuses(s, false)) return rc;
    if (int rc = shifts_refuse(s, "replace_residual")) return rc;
    if (s->proj.spent) return fail(CGAMD_ERR_STATE, std::string("replace_residual") + kProjSpent);
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = step_not_capturing(s, "replace_residual")) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t vs = dtype_size(s->dtype), vbytes = (size_t)s->n * s->nrhs * vs;
    if (int rc = enter_until_mode(s, st)) return rc;        // d = beta d + r of the OLD residual is part of the direction that is kept
    if (ldr != s->n) {
        CG_HIP(hipMemsetAsync(s->r, 0, vbytes, st));        // the padding rows
        CG_HIP(hipMemcpy2DAsync(s->r, (size_t)s->n * vs, r_new, (size_t)ldr * vs, (size_t)s->n_user * vs, (size_t)s->nrhs, hipMemcpyDeviceToDevice, st));
    } else {
        CG_HIP(hipMemcpyAsync(s->r, r_new, vbytes, hipMemcpyDeviceToDevice, st));
    }
    CG_HIP(hipMemsetAsync(s->x, 0, vbytes, st));
    // delta0 (rho0) by the launches of set_rhs, in their order; d is read and written by none of them
    int rc;
    if (s->pre.mdiag) {     // z = m .* r lands in q, which is dead between iterations
        if ((rc = launch_pcg_axpy2_dot2(s->dtype, true, s->n, s->q, s->x, s->q, s->r, s->pre.mdiag, s->n, nullptr, s->nrhs, s->part_rz, s->part_rr,
                                        s->vgrid, st, m_pitch(s)))) return rc;
        if ((rc = launch_pcg_delta0(s->dtype, s->part_rz, s->part_rr, s->vgrid, s->nrhs, s->sc, s->pre.rho2, st))) return rc;
    } else {
        if ((rc = launch_dot_partials(s->dtype, s->n, s->r, s->r, s->n, s->nrhs, s->part_rr, s->vgrid, st))) return rc;
        if ((rc = launch_cg_delta0(s->dtype, s->part_rr, s->vgrid, s->nrhs, s->sc, st))) return rc;
    }
    s->iters = 0;
    s->until_stopped = s->stop.armed = false;
    return CGAMD_OK;
}
int cgamd_solver_replace_residual(cgamd_solver *s, const void *r_new) {
    if (!s || !r_new) return fail(CGAMD_ERR_INVALID, "replace_residual: null argument");
    return replace_residual_impl(s, r_new, s->n_user);
}

// Per-right-hand-side tolerance stop ON THE DEVICE for the launched loops (include/cgamd.h): every right-hand side stops in the
// first iteration whose sqrt|r.r| fails >= tol[r] and is frozen there while the others run on -- the reference's sub-domain loop
// `r[p] = CG(P[0], z[p].ravel(), tol=CGtol, maxit=CGMaxIT)` (p_h-PY_C-CL.py:1916-1921, 1338-1369) as ONE batched solve.  The
// host enqueues chunks of checkEvery iterations and, after each, an asynchronous read of the record's active count; it waits for
// the count of chunk c - 1 only once chunk c is in the stream, so the device never idles on the host, and it never waits per
// iteration.  Iterations enqueued after the last stop change nothing on the device (stop_device.h), so the result does not depend
// on checkEvery, and until(a); until(b) leaves the bits of until(a + b).
int cgamd_solver_iterate_until(cgamd_solver *s, int maxIterations, const double *tol, int nTol, int checkEvery, int *iterations_run) {
    // (what can be judged without the handle comes first)
    if (maxIterations < 0 || checkEvery < 0) return fail(CGAMD_ERR_INVALID, "iterate_until: negative maxIterations or checkEvery");
    if (nTol < 1) return fail(CGAMD_ERR_INVALID, "iterate_until: nTol must be 1 or nRHS");
    if (!s || !tol || !iterations_run) return fail(CGAMD_ERR_INVALID, "iterate_until: NULL solver, tol or iterations_run");
    if (nTol != 1 && nTol != s->nrhs) return fail(CGAMD_ERR_INVALID, "iterate_until: nTol must be 1 or nRHS");
    for (int i = 0; i < nTol; ++i)
        if (!(tol[i] > 0.)) return fail(CGAMD_ERR_INVALID, "iterate_until: every tolerance must be positive");
    TuneScope ts(&s->tune);
    if (!s->rhs_set) return fail(CGAMD_ERR_STATE, "iterate_until: call set_rhs first");
    if (s->rm) return fail(CGAMD_ERR_STATE, "iterate_until: the handle keeps its right-hand sides interleaved (row-major layout)");
    if (s->flags & CGAMD_UNFUSED) return fail(CGAMD_ERR_STATE, "iterate_until: CGAMD_UNFUSED replays the reference's kernel sequence, which has no guarded form");
    if (s->proj.spent) return fail(CGAMD_ERR_STATE, std::string("iterate_until") + kProjSpent);
    const int nr = s->nrhs;
    if (maxIterations == 0) {
        for (int r = 0; r < nr; ++r) iterations_run[r] = (s->stop.armed && s->stop.stopped[r]) ? s->stop.stopped[r] : s->iters;
        return CGAMD_OK;
    }
    CG_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (int rc = stop_run_alloc(s->stop, nr)) return rc;
    if (int rc = ensure_history(s, s->iters + maxIterations + 1)) return rc;
    if (int rc = enter_until_mode(s, st)) return rc;
    if (int rc = stop_run_arm(s->stop, tol, nTol, st)) return rc;
    const int chunk = checkEvery ? checkEvery : 8;
    const bool use_graph = !(s->flags & CGAMD_NO_GRAPH) && !s->graph_failed;
    // a whole chunk is one captured graph (gT), replayed by every later call with the same checkEvery; the tail is plain launches
    auto enqueue = [&](int len) -> int {
        if (use_graph && !s->graph_failed && len == chunk) {
            if (s->gT && s->gT_len != chunk) {
                (void)hipGraphExecDestroy(s->gT); (void)hipGraphDestroy(s->gTg);
                s->gT = nullptr; s->gTg = nullptr;
            }
            if (!s->gT) {
                if (capture(s, 0, chunk, &s->gTg, &s->gT, true) == CGAMD_OK) s->gT_len = chunk;
                else { s->graph_failed = true; destroy_graphs(s); }
            }
            if (s->gT) {
                CG_HIP(hipGraphLaunch(s->gT, st));
                return CGAMD_OK;
            }
        }
        for (int i = 0; i < len; ++i)
            if (int rc = enqueue_iteration(s, i, st, 1, &s->stop.view)) return rc;
        return CGAMD_OK;
    };
    if (int rc = stop_run_chunks(s->stop, maxIterations, chunk, st, enqueue)) {
        (void)hipStreamSynchronize(st);     // part of an iteration may be in the stream: the handle demands a fresh set_rhs
        s->rhs_set = false;
        return rc;
    }
    // (columns may have stopped in different iterations: the count comes from the device, not from what was enqueued)
    CG_HIP(hipMemcpyAsync(s->stop.pin + 2, s->sc.iter, sizeof(int), hipMemcpyDeviceToHost, st));
    if (int rc = stop_run_read(s->stop, st)) return rc;
    CG_HIP(hipStreamSynchronize(st));
    s->iters = s->stop.pin[2];
    for (int r = 0; r < nr; ++r) {
        if (s->stop.stopped[r]) s->until_stopped = true;
        iterations_run[r] = s->stop.stopped[r] ? s->stop.stopped[r] : s->iters;
    }
    return CGAMD_OK;
}

// nIterations plain-launch iterations of the SAME launch sequence cgamd_solver_iterate replays (enqueue_iteration), with a
// HIP event pair around every SpMV launch on the solver's stream: the in-loop duration of the dominant kernel
// (bench.py's roofline).  Synchronises.
int cgamd_solver_iterate_timed(cgamd_solver *s, int nIterations, float *spmv_ms_avg, float *iter_ms_avg) {
    if (!s || !spmv_ms_avg) return fail(CGAMD_ERR_INVALID, "iterate_timed: null argument");
    TuneScope ts(&s->tune);
    if (!s->rhs_set) return fail(CGAMD_ERR_STATE, "iterate_timed: call set_rhs first");
    if (nIterations < 1) return fail(CGAMD_ERR_INVALID, "iterate_timed: needs >= 1 iteration");
    if (s->until_stopped) return fail(CGAMD_ERR_STATE, "iterate_timed: iterate_until has stopped a right-hand side: go on with iterate_until, or call set_rhs");
    if (s->proj.spent) return fail(CGAMD_ERR_STATE, std::string("iterate_timed") + kProjSpent);
    CG_HIP(hipSetDevice(s->ctx->device));
    if (int rc = ensure_history(s, s->iters + nIterations + 1)) return rc;
    hipStream_t st = s->ctx->stream;
    std::vector<hipEvent_t> ev((size_t)2 * nIterations + 2, nullptr);
    int rc = CGAMD_OK, done = 0;
    hipError_t e = hipSuccess;
    for (auto &x : ev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    if (e == hipSuccess) e = hipEventRecord(ev[(size_t)2 * nIterations], st);
    for (int i = 0; i < nIterations && e == hipSuccess && !rc; ++i) {
        s->ev_pair = &ev[(size_t)2 * i];
        rc = enqueue_iteration(s, s->iters + i, st);
        ++done;
    }
    s->ev_pair = nullptr;
    s->iters += done;       // whatever was enqueued counts, also on the error paths below
    if (e == hipSuccess && !rc) e = hipEventRecord(ev[(size_t)2 * nIterations + 1], st);
    if (e == hipSuccess && !rc && fused2_now(s)) rc = launch_cg_tail(s->dtype, s->part_rr, s->vgrid, s->nrhs, s->sc, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    double sum = 0.0;
    float total = 0.f;
    for (int i = 0; i < nIterations && e == hipSuccess && !rc; ++i) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ev[(size_t)2 * i], ev[(size_t)2 * i + 1]);
        sum += ms;
    }
    if (e == hipSuccess && !rc) e = hipEventElapsedTime(&total, ev[(size_t)2 * nIterations], ev[(size_t)2 * nIterations + 1]);
    for (auto &x : ev)
        if (x) (void)hipEventDestroy(x);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("iterate_timed: ") + hipGetErrorString(e));
    *spmv_ms_avg = (float)(sum / nIterations);
    if (iter_ms_avg) *iter_ms_avg = total / nIterations;
    return CGAMD_OK;
}

int cgamd_solver_get_x(cgamd_solver *s, void *x, int on_device) {
    if (!s || !x) return fail(CGAMD_ERR_INVALID, "get_x: null argument");
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    const size_t vbytes = (size_t)s->n * s->nrhs * dtype_size(s->dtype);
    const void *src = s->x;
    if (s->rm) {    // back to the caller's RHS-major layout; q is dead between iterations (recomputed first thing in the next)
        if (int rc = launch_transpose(s->dtype, s->n, s->nrhs, s->x, s->q, s->ctx->stream)) return rc;
        src = s->q;
    }
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (s->n != s->n_user) {
        const size_t vs = dtype_size(s->dtype);
        CG_HIP(hipMemcpy2DAsync(x, (size_t)s->n_user * vs, src, (size_t)s->n * vs, (size_t)s->n_user * vs, (size_t)s->nrhs, kind, s->ctx->stream));
    } else {
        CG_HIP(hipMemcpyAsync(x, src, vbytes, kind, s->ctx->stream));
    }
    if (!on_device) CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

int cgamd_solver_iterations_done(cgamd_solver *s) { return s ? s->iters : -CGAMD_ERR_INVALID; }

int cgamd_solver_history(cgamd_solver *s, void *history, int max_entries) {
    if (!s || !history) { fail(CGAMD_ERR_INVALID, "history: null argument"); return -CGAMD_ERR_INVALID; }
    if (!s->rhs_set) { fail(CGAMD_ERR_STATE, "history: no right-hand side set"); return -CGAMD_ERR_STATE; }
    thread_hip_setup();
    if (hipSetDevice(s->ctx->device) != hipSuccess) return -CGAMD_ERR_NO_DEVICE;
    const int entries = std::min(std::min(s->iters + 1, s->sc.history_cap), max_entries);
    hipError_t e = hipMemcpyAsync(history, s->sc.history, (size_t)entries * s->nrhs * dtype_size(s->dtype),
                                  hipMemcpyDeviceToHost, s->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
    if (e != hipSuccess) { fail(CGAMD_ERR_HIP, std::string("history: ") + hipGetErrorString(e)); return -CGAMD_ERR_HIP; }
    return entries;
}

int cgamd_solver_ld(cgamd_solver *s) { return s ? s->n : -CGAMD_ERR_INVALID; }

void *cgamd_solver_vector(cgamd_solver *s, int which) {
    if (!s) return nullptr;
    // (d ping-pongs only while the two-launch loop runs: with a preconditioner set the direction is in the one buffer)
    switch (which) { case 0: return s->x; case 1: return s->r; case 2: return fused2_now(s) ? dbuf(s, s->iters) : s->d; case 3: return s->q; default: return nullptr; }
}

int cgamd_solver_solve(cgamd_solver *s, const void *b, void *x, int nIterations, void *history) {
    if (!s || !b || !x) return fail(CGAMD_ERR_INVALID, "solve: null argument");
    int rc;
    if ((rc = cgamd_solver_set_rhs(s, b, x, 0))) return rc;   // x is in/out: initial guess (clcg.c:210)
    if ((rc = cgamd_solver_iterate(s, nIterations))) return rc;
    if ((rc = cgamd_solver_get_x(s, x, 0))) return rc;
    if (history) {
        const int got = cgamd_solver_history(s, history, nIterations + 1);
        if (got < 0) return -got;
    }
    return CGAMD_OK;
}

int cgamd_solver_spmv(cgamd_solver *s, const void *x, void *y, int fused_dot) {
    if (!s || !x || !y) return fail(CGAMD_ERR_INVALID, "solver_spmv: null argument");
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    // the caller's vectors have the caller's stride; the plan fits both sizes (same row blocks, the appended rows are empty)
    return handle_spmv(s, s->n_user, x, s->n_user, y, s->n_user, fused_dot ? x : nullptr, fused_dot ? s->part_dq : nullptr, s->ctx->stream);
}

int cgamd_last_spmv_form(int *out, int n_out) {
    if (!out || n_out < 1) return -fail(CGAMD_ERR_INVALID, "last_spmv_form: null or empty output");
    last_spmv_form(out, n_out);
    return n_out < kSpmvFormFields ? n_out : kSpmvFormFields;
}

int cgamd_solver_dot_partials(cgamd_solver *s, void *out_host, long long cap_values, int *per_rhs) {
    if (!s || !out_host || !per_rhs) return fail(CGAMD_ERR_INVALID, "dot_partials: null argument");
    const int P = s->rm ? s->rm_nwg : s->plan.n_partials;      // a row-major handle: one partial per work-group of the SpMM sweep
    *per_rhs = P;
    if (cap_values < (long long)P * s->nrhs) return fail(CGAMD_ERR_INVALID, "dot_partials: output holds fewer than nRHS * partials values");
    CG_HIP(hipSetDevice(s->ctx->device));
    CG_HIP(hipMemcpyAsync(out_host, s->part_dq, acc_size(s->dtype) * (size_t)P * s->nrhs, hipMemcpyDeviceToHost, s->ctx->stream));
    CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

// ---- test-facing record of the vector and scalar steps (tests/test_gpu_cg_steps.py) ------------------------------------------------
// Neither entry launches a kernel or changes the handle.  Both refuse a handle whose stream is being captured: a copy or a
// synchronisation there would end the capture with an error.
// Row-major and tridiagonal handles launch their vector and scalar steps with grids of their own (rm_nwg / rm_vgrid, tri.grid); the
// tridiagonal ones keep their partials elsewhere (tri_part).  step_plan describes neither and refuses both; step_state serves a handle
// that is row-major now (rm_ok: the state of a handle that will be row-major after its next set_rhs is nobody's) and refuses the rest
static int step_launched_rhs_major(cgamd_solver *s, const char *who, bool serve_rm = false) {
    if (serve_rm && s->rm) return CGAMD_OK;
    if (s->rm || (s->rm_ok && !precond_set(s)) || tri_on(s) || s->pre.mg)
        return fail(CGAMD_ERR_INVALID, std::string(who) + ": not recorded for row-major and tridiagonal handles");
    if (s->herm) return fail(CGAMD_ERR_INVALID, std::string(who) + ": not recorded for CGAMD_HERMITIAN handles (steps of their own, hermitian.hip)");
    return CGAMD_OK;
}

// What enqueue_iteration / cgamd_solver_set_rhs pass to the launchers of vector.hip NOW, read from the fields and through the
// functions they read them from: s->n (size and leading dimension of every launch), s->vgrid, plan.n_partials, sc.kdq / sc.krr,
// fold_alpha_ok (the folded alpha), the condition of alpha_impl for the two-level cg_alpha2 (vector.hip: stage && ticket &&
// grid >= 16384, the grid being plan.n_partials in every loop but the UNFUSED one, whose d.q partials are the vgrid of
// dot_partials), vec_ok on the handle's vectors (and the diagonal of a Jacobi handle, as launch_pcg_* ask), the vec_nt the
// launchers resolve, x_lag_now.
constexpr int kStepPlanFields = 11;
int cgamd_solver_step_plan(cgamd_solver *s, int *out, int n_out) {
    if (!s || !out || n_out < 1) return -fail(CGAMD_ERR_INVALID, "step_plan: null or empty output");
    TuneScope ts(&s->tune);
    if (int rc = step_not_capturing(s, "step_plan")) return -rc;
    if (int rc = step_launched_rhs_major(s, "step_plan")) return -rc;
    // the branches of enqueue_iteration that are left: the diagonal preconditioner first, then the UNFUSED flag (eight launches, alpha
    // from the vgrid partials of dot_partials), else the folded or the separate alpha on the SpMV's d.q partials
    const bool unfused = (s->flags & CGAMD_UNFUSED) && !s->pre.mdiag;
    const int alpha_grid = unfused ? s->vgrid : s->plan.n_partials;
    const bool fold = !unfused && !s->pre.mdiag && fold_alpha_ok(s->plan.n_partials, s->plan.fold_max);
    bool vec = vec_ok(s->dtype, s->n, s->nrhs, {s->x, s->r, s->d, s->q});
    if (s->pre.mdiag) vec = vec && aligned16(s->pre.mdiag) && ((m_pitch(s) * (long long)dtype_size(s->dtype)) & 15) == 0;
    const int f[kStepPlanFields] = {s->n, s->n, s->vgrid, s->plan.n_partials, s->sc.kdq, s->sc.krr, fold ? 1 : 0,
                                    (!fold && s->sc.stage && s->sc.ticket && alpha_grid >= 16384) ? 1 : 0, vec ? 1 : 0,
                                    tune().vec_nt >= 0 ? tune().vec_nt : s->plan.vec_nt, x_lag_now(s)};
    const int k = n_out < kStepPlanFields ? n_out : kStepPlanFields;
    for (int i = 0; i < k; ++i) out[i] = f[i];
    return k;
}

// which: 0 r.r partials [nRHS][vgrid], 1 r.z partials [nRHS][vgrid] (a Jacobi handle), in the accumulator type; 2 alpha (slot 0),
// 3 beta, 4 delta [nRHS], 5 the rho parity buffer [2][nRHS], in the value type; 6 the iteration counter (one int)
int cgamd_solver_step_state(cgamd_solver *s, int which, void *out_host, long long cap_values, long long *count) {
    if (!s || !out_host || !count) return fail(CGAMD_ERR_INVALID, "step_state: null argument");
    if (int rc = step_not_capturing(s, "step_state")) return rc;
    if (int rc = step_launched_rhs_major(s, "step_state", true)) return rc;
    const void *src = nullptr;
    size_t each = dtype_size(s->dtype);
    long long values = s->nrhs;
    const int vgrid = s->rm ? s->rm_vgrid : s->vgrid;      // the grid of the rm_* vector launches; they form no r.z partials, no rho
    switch (which) {
    case 0: src = s->part_rr; each = acc_size(s->dtype); values = (long long)vgrid * s->nrhs; break;
    case 1: src = s->rm ? nullptr : s->part_rz; each = acc_size(s->dtype); values = (long long)vgrid * s->nrhs; break;
    case 2: src = s->sc.alpha; break;
    case 3: src = s->sc.beta; break;
    case 4: src = s->sc.delta; break;
    case 5: src = s->rm ? nullptr : s->pre.rho2; values = 2LL * s->nrhs; break;
    case 6: src = s->sc.iter; each = sizeof(int); values = 1; break;
    default: return fail(CGAMD_ERR_INVALID, "step_state: which is 0 .. 6");
    }
    if (!src) return fail(CGAMD_ERR_INVALID, "step_state: the handle has no such buffer (r.z partials and the rho buffer need a diagonal preconditioner)");
    *count = values;
    if (cap_values < values) return fail(CGAMD_ERR_INVALID, "step_state: output holds fewer values than the state has");
    CG_HIP(hipSetDevice(s->ctx->device));
    CG_HIP(hipMemcpyAsync(out_host, src, each * (size_t)values, hipMemcpyDeviceToHost, s->ctx->stream));
    CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

// What enqueue_iteration / set_rhs_impl pass to the launchers of rowmajor.hip NOW (include/cgamd.h), through the functions they launch
// through: spmm_rm_plan is rm_instance + rm_grid_for as launch_spmm_rm calls them (fused: with s->part_dq; unfused: set_rhs and
// cgamd_solver_spmm_rowmajor), rm_vec_nt the rule of rm_axpy_dot_impl / rm_aypx_x_impl; s->rm_vgrid, sc.kdq / sc.krr are the fields
constexpr int kRowmajorPlanFields = 17;
int cgamd_solver_rowmajor_plan(cgamd_solver *s, int *out, int n_out) {
    if (!s || !out || n_out < 1) return -fail(CGAMD_ERR_INVALID, "rowmajor_plan: null or empty output");
    TuneScope ts(&s->tune);
    if (int rc = step_not_capturing(s, "rowmajor_plan")) return -rc;
    if (!s->rm) return -fail(CGAMD_ERR_INVALID, "rowmajor_plan: the handle does not keep its right-hand sides row-major now (cgamd_solver_layout)");
    int fu[6], un[6], lead = 0;
    if (int rc = spmm_rm_plan(s->dtype, s->nrhs, s->n, s->plan.max_quad, true, s->rm_pace != nullptr, fu, &lead)) return -rc;
    if (int rc = spmm_rm_plan(s->dtype, s->nrhs, s->n, s->plan.max_quad, false, s->rm_pace != nullptr, un, &lead)) return -rc;
    const long long total = (long long)s->n * s->nrhs;
    const int f[kRowmajorPlanFields] = {s->n, fu[0], fu[1], fu[2], un[2], fu[3], fu[4], un[4], s->rm_vgrid, rm_vec_nt(2, total, s->dtype) ? 1 : 0,
                                        rm_vec_nt(1, total, s->dtype) ? 1 : 0, s->sc.kdq, s->sc.krr, fu[5], un[5], lead, s->rm_nwg};
    const int k = n_out < kRowmajorPlanFields ? n_out : kRowmajorPlanFields;
    for (int i = 0; i < k; ++i) out[i] = f[i];
    return k;
}

// alpha and beta of a CGAMD_HERMITIAN handle (step_state describes the other loops' steps and refuses these handles)
int cgamd_solver_hermitian_scalars(cgamd_solver *s, void *alpha_host, void *beta_host) {
    if (!s) return fail(CGAMD_ERR_INVALID, "hermitian_scalars: solver is NULL");
    if (!s->herm) return fail(CGAMD_ERR_STATE, "hermitian_scalars: the handle does not run the conjugated recurrence (use cgamd_solver_step_state)");
    if (int rc = step_not_capturing(s, "hermitian_scalars")) return rc;
    CG_HIP(hipSetDevice(s->ctx->device));
    const size_t bytes = dtype_size(s->dtype) * (size_t)s->nrhs;
    if (alpha_host) CG_HIP(hipMemcpyAsync(alpha_host, s->sc.alpha, bytes, hipMemcpyDeviceToHost, s->ctx->stream));
    if (beta_host) CG_HIP(hipMemcpyAsync(beta_host, s->sc.beta, bytes, hipMemcpyDeviceToHost, s->ctx->stream));
    CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

int cgamd_solver_spmm_rowmajor(cgamd_solver *s, const void *x, void *y, int nRHS) {
    if (!s || !x || !y) return fail(CGAMD_ERR_INVALID, "spmm_rowmajor: null argument");
    if (s->nsys) return fail(CGAMD_ERR_STATE, "spmm_rowmajor: the handle is batched (a matrix of its own per right-hand side)");
    TuneScope ts(&s->tune);
    CG_HIP(hipSetDevice(s->ctx->device));
    return launch_spmm_rm(s->dtype, s->n_user, s->nnz, s->vals, s->ptr, s->cols, x, y, nRHS, nullptr, s->plan.max_quad, s->rm_pace, s->ctx->stream);
}

int cgamd_solver_layout(cgamd_solver *s) { return s ? (s->rm ? 1 : 0) : -CGAMD_ERR_INVALID; }
int cgamd_solver_loop_launches(cgamd_solver *s) {
    if (!s) return -CGAMD_ERR_INVALID;
    TuneScope ts(&s->tune);
    // preconditioned block CG: the six below, the partials of W^T Z, and what z = M^-1 w launches (a diagonal M: nothing)
    if (s->blk_want && s->blk_pcg) return 7 + (s->pre.mg ? mg_cost(s->pre.mg).launches : tri_on(s) ? (s->pre.tri.longform ? 3 : 1) : 0);
    if (s->blk_want) return 6;                           // block CG: SpMV, Gram, the G step, x / w update, the W step, q / p update, whatever s
    if (s->herm) return 4;                               // SpMV, herm_alpha, herm_axpy_dot, herm_aypx_beta_x under every flag
    if (s->pre.mg) return 5 + mg_cost(s->pre.mg).launches;       // SpMV, cg_alpha, r update, the V-cycle's chain, r.z, update
    if (tri_on(s)) return s->pre.tri.longform ? 6 : 4;      // launched loop only: SpMV, cg_alpha, the sweep (3 launches in the long form), update
    if (s->nsys && s->pre.mdiag) return 4;                   // a batched handle's PCG loop is the same four launches under every flag
    if (s->flags & CGAMD_UNFUSED) return 8;
    if (s->rm) return 5;
    if (s->pre.mdiag) return (s->resw.ok && !s->rm && !(s->flags & (CGAMD_NO_GRAPH | CGAMD_UNFUSED))) ? 1 : 4;
    // shifts in force: the three / four-launch loop, then the shift scalar step and ONE vector launch whatever the number of shifts
    if (nshifts(s)) return (fold_alpha_ok(s->plan.n_partials, s->plan.fold_max) ? 3 : 4) + 2;
    if (fused2_now(s) && s->res_ok && !(s->flags & CGAMD_NO_GRAPH)) return 0;
    if (s->resw.ok && !(s->flags & CGAMD_NO_GRAPH)) return 1;       // chip-wide resident group (same bits as the launched loops of this handle)
    if (fused2_now(s)) return 2;
    return fold_alpha_ok(s->plan.n_partials, s->plan.fold_max) ? 3 : 4;
}

int cgamd_solver_x_lag(cgamd_solver *s) {
    if (!s) return -CGAMD_ERR_INVALID;
    return x_lag_now(s);
}

int cgamd_solver_index_codes(cgamd_solver *s) { return s ? s->n_offsets : -CGAMD_ERR_INVALID; }

// value arrays the byte models count, each once (a batched handle: one per system), beside the indices, which are counted once
static long long value_arrays(const cgamd_solver *s) { return s->nsys ? s->nsys : 1; }
long long cgamd_solver_spmv_bytes(cgamd_solver *s) {
    if (!s) return 0;
    const long long V = (long long)dtype_size(s->dtype);
    return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + 2LL * s->n_user * V * s->nrhs;
}
// vector passes of the tridiagonal loop, counted once per right-hand side and once for the factors all of them share: SpMV
// (p, q) 2 + sweep (r, q in; r, z out) 4 + update (z, p, x in; x, p out) 5 = 11 per RHS and nl, ne, w = 3; the long form reads
// r again and writes z from a second sweep launch (+2 per RHS) and reads the factors twice (+3).  The strided form (one thread per
// segment) stores w y in the forward walk and reads it and r back in the backward walk: sweep (r, q in; r, w y out; w y, r in; z
// out) 7, so 14 per RHS, and each factor once
// (a batched handle has factors of its own per right-hand side)
// the multigrid loop: SpMV (p, q) 2 + r update (q, r in; r out) 3 + r.z (r, z) 2 + update (z, p, x in; x, p out) 5 = 12 passes per RHS,
// and the V-cycle: its fine-level SpMVs at the price of this handle's SpMV, everything else as multigrid_setup.cpp counts it
static long long mg_bytes(const cgamd_solver *s, long long spmv_bytes) {
    const MgCost c = mg_cost(s->pre.mg);
    return 12LL * s->n_user * (long long)dtype_size(s->dtype) * s->nrhs + c.spmv0 * spmv_bytes + c.bytes;
}
// the shift vector launch: r read once, x_j and d_j of every shift read and written
static long long shift_bytes(const cgamd_solver *s) { return nshifts(s) ? (4LL * nshifts(s) + 1) * s->n_user * (long long)dtype_size(s->dtype) * s->nrhs : 0; }
// the block loop: SpMV (P in, AP out) 2 + Gram (P, AP) 2 + x / w update (P, AP, X, Q in; X, Q out) 6 + q / p update (Q, P in and out) 4
constexpr long long kBlockPasses = 14;
static long long tri_passes(const cgamd_solver *s) {
    const long long f = value_arrays(s);
    if (s->pre.tri.stride > 1) return 14LL * s->nrhs + 3 * f;
    return s->pre.tri.longform ? 13LL * s->nrhs + 6 * f : 11LL * s->nrhs + 3 * f;
}
// the preconditioned block loop, beside the matrix: the block loop's SpMV 2 + Gram 2 + x / w update 6, then
//   a diagonal M    the weighted Gram (W) 1 + the q / p update (Q, P in and out; z formed in registers) 4 = 15 per right-hand side, and m
//                   read by both launches
//   a line M or a   Gram (W, Z) 2 + the q / p update (Q, Z, P in; Q, P out) 5 = 17 per right-hand side, and z = M^-1 w at the price the
//   V-cycle         scalar loops' models give it: the V-cycle as mg_bytes counts it; the sweep without the r update (r in, z out: 2,
//                   the long form reads r twice: 3, the strided form stores and reads back w y: 5) and the factors it reads
static long long block_pcg_bytes(const cgamd_solver *s, long long spmv_bytes) {
    const long long V = (long long)dtype_size(s->dtype), col = (long long)s->n_user * V;
    if (s->pre.mdiag) return 15 * col * s->nrhs + 2 * col;
    if (s->pre.mg) {
        const MgCost c = mg_cost(s->pre.mg);
        return 17 * col * s->nrhs + c.spmv0 * spmv_bytes + c.bytes;
    }
    const long long sweep = s->pre.tri.stride > 1 ? 5LL * s->nrhs + 3 : s->pre.tri.longform ? 3LL * s->nrhs + 6 : 2LL * s->nrhs + 3;
    return (17LL * s->nrhs + sweep) * col;
}
long long cgamd_solver_iter_bytes(cgamd_solver *s, int fused) {
    if (!s) return 0;
    const long long V = (long long)dtype_size(s->dtype);
    if (s->blk_want && s->blk_pcg) return s->nnz * (V + 4) + ((long long)s->n_user + 1) * 4 + block_pcg_bytes(s, cgamd_solver_spmv_bytes(s));
    if (s->blk_want) return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + kBlockPasses * s->n_user * V * s->nrhs;
    if (s->pre.mg) return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + mg_bytes(s, cgamd_solver_spmv_bytes(s));
    if (tri_on(s)) return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + tri_passes(s) * s->n_user * V;
    // the conjugated recurrence: the launched loop's 10 passes (12 with a diagonal M) and conj(d), written by the d step and read by the SpMV's dot
    if (s->herm) return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + (s->pre.mdiag ? 14LL : 12LL) * s->n_user * V * s->nrhs;
    if (s->nsys && s->pre.mdiag) return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + 12LL * s->n_user * V * s->nrhs;
    return s->nnz * (value_arrays(s) * V + 4) + ((long long)s->n_user + 1) * 4 + (fused ? 11LL : 14LL) * s->n_user * V * s->nrhs + shift_bytes(s);
}

// What the handle's own kernels MOVE (the physical byte model the roofline fraction is priced on): index bytes per non-zero as
// the SpMV really reads them (1 with the one-byte column codes, 2 with 16-bit block-relative columns, else 4) and the vector
// passes of the launched loop the handle runs (10 with the deferred x update, 11 without, 12 preconditioned, 14 for the
// reference's op structure; the tridiagonal M: tri_passes).  Handles whose iterate() runs a resident loop report the launched loop
// they fall back to.
static long long long_rows_scratch_traffic(const cgamd_solver *s) { return s->plan.lr.on ? 2LL * (long long)s->plan.lr.scratch_bytes : 0; }
// The form the SpMV of the handle's launched loop takes: the decision of the launcher itself (spmv_form.cpp), asked with the call
// enqueue_spmv makes through launch_spmv -- the handle's own arrays, the direction d in, q out, the d.q partials unless the handle
// sums them in a launch of its own.  Every accessor and byte model below is read off this form.  (Handles whose loop SpMV is another
// launcher's -- launch_spmv_batched, the row-major SpMM, the two-launch loop -- have none of the codes, and are priced on aValues
// and aCols as before.)
// (the block loop forms its Gram matrix in a launch of its own: its SpMV carries no dot)
static bool loop_fused(const cgamd_solver *s) { return !s->blk_want && !((s->flags & CGAMD_UNFUSED) && !tri_on(s) && !(s->nsys && s->pre.mdiag)); }
static SpmvCall loop_call(const cgamd_solver *s, bool fused) {
    SpmvCall c;
    c.value_bytes = (int)dtype_size(s->dtype); c.acc_bytes = (int)acc_size(s->dtype); c.n = s->n; c.nrhs = s->nrhs;
    c.vec = aligned16(s->vals) && aligned16(s->cols);
    c.codes_for = s->plan.codes_for == s->cols; c.vcodes_for = s->plan.vcodes_for == s->vals; c.rcodes_for = s->plan.rcodes_for == s->ptr;
    c.fuse = fused;
    c.x16 = aligned16(s->d); c.y16 = aligned16(s->q); c.d16 = aligned16(s->herm ? s->d2 : s->d);
    return c;
}
static SpmvForm loop_form(const cgamd_solver *s) { return choose_spmv_form(s->plan, s->tune, loop_call(s, loop_fused(s))); }
static bool row_coded(const SpmvForm &f) { return f.family == 7 || f.family == 8; }
// bytes of the matrix one SpMV of that form reads: one code byte per row (no per-non-zero bytes, no row pointers), or per non-zero
// the index as encoded (aCols 4, 8-bit codes 1, 16-bit codes 2) and the value (joint and row codes: none beside the index byte; value
// codes: 1; else aValues of every system) and the row pointers
static long long matrix_moved_bytes(const cgamd_solver *s, const SpmvForm &f) {
    if (row_coded(f)) return (long long)s->n_user;
    const long long value_bytes = f.venc >= 2 ? 0 : f.venc == 1 ? 1 : (long long)dtype_size(s->dtype) * value_arrays(s);
    return s->nnz * (value_bytes + (f.ienc == 8 ? 1 : f.ienc == 16 ? 2 : 4)) + ((long long)s->n_user + 1) * 4;
}
long long cgamd_solver_spmv_moved_bytes(cgamd_solver *s) {
    if (!s) return 0;
    // the matrix, x read, y written
    // (CGAMD_SPLIT_LONG_ROWS: the body's bytes and the heavy blocks' entries once are the matrix once; the piece scratch is written and read)
    return matrix_moved_bytes(s, loop_form(s)) + 2LL * s->n_user * (long long)dtype_size(s->dtype) * s->nrhs + long_rows_scratch_traffic(s);
}
int cgamd_solver_spmv_form(cgamd_solver *s, int fused, int *inputs, int n_inputs, int *form, int n_form) {
    if (!s || !form || n_form < 1) return -fail(CGAMD_ERR_INVALID, "spmv_form: null or empty output");
    const SpmvCall c = loop_call(s, fused != 0);
    int in[kSpmvFormInputs], out[kSpmvFormFields];
    spmv_form_pack(s->plan, s->tune, c, in);
    choose_spmv_form(s->plan, s->tune, c).record(out);
    for (int i = 0; inputs && i < n_inputs && i < kSpmvFormInputs; ++i) inputs[i] = in[i];
    const int k = n_form < kSpmvFormFields ? n_form : kSpmvFormFields;
    for (int i = 0; i < k; ++i) form[i] = out[i];
    return k;
}
int cgamd_solver_long_rows(cgamd_solver *s, int *out, int n_out) {
    if (!s || !out || n_out < 1) return -fail(CGAMD_ERR_INVALID, "solver_long_rows: null or empty output");
    const LongRows &lr = s->plan.lr;
    const int f[6] = {lr.on ? lr.n_heavy : 0, lr.on ? lr.n_seg : 0, lr.on ? lr.seg_len : 0, lr.on ? lr.body_kind : 0,
                      lr.on ? (lr.body_kind == 7 ? lr.body_lpr : lr.body_kind == 5 ? 1 : 0) : 0, lr.on ? (int)lr.scratch_bytes : 0};
    for (int i = 0; i < n_out && i < 6; ++i) out[i] = f[i];
    return n_out < 6 ? n_out : 6;
}
int cgamd_solver_value_codes(cgamd_solver *s) { return s ? s->n_values : -CGAMD_ERR_INVALID; }
int cgamd_solver_joint_codes(cgamd_solver *s) { return s ? (loop_form(s).venc >= 2 ? s->n_pairs : 0) : -CGAMD_ERR_INVALID; }
int cgamd_solver_row_codes(cgamd_solver *s) { return s ? (row_coded(loop_form(s)) ? s->n_user_patterns : 0) : -CGAMD_ERR_INVALID; }
int cgamd_solver_row_pairs(cgamd_solver *s) { return s ? (loop_form(s).family == 8 ? s->n_pair_patterns : 0) : -CGAMD_ERR_INVALID; }
int cgamd_solver_spmv_schedule(cgamd_solver *s, int *kind, int *grid, long long *unit_rows) {
    if (!s) return fail(CGAMD_ERR_INVALID, "spmv_schedule: solver is NULL");
    const SpmvForm f = loop_form(s);
    if (kind) *kind = row_coded(f) && f.table ? 1 : 0;
    if (unit_rows) *unit_rows = row_coded(f) ? s->sched_unit : 0;
    if (grid) *grid = row_coded(f) ? f.grid : 0;
    return CGAMD_OK;
}
int cgamd_solver_row_pipe(cgamd_solver *s) {
    if (!s) return -CGAMD_ERR_INVALID;
    const SpmvForm f = loop_form(s);
    return row_coded(f) ? f.depth : 0;
}
long long cgamd_solver_iter_moved_bytes(cgamd_solver *s) {
    if (!s) return 0;
    const long long V = (long long)dtype_size(s->dtype);
    const long long passes = s->herm ? (s->pre.mdiag ? 14 : 12) : (s->nsys && s->pre.mdiag) ? 12 : (s->flags & CGAMD_UNFUSED) ? 14 : s->pre.mdiag ? 12 : 10;
    const long long lag = x_lag_now(s);
    const long long matrix = matrix_moved_bytes(s, loop_form(s)) + long_rows_scratch_traffic(s);
    if (s->blk_want && s->blk_pcg) return matrix + block_pcg_bytes(s, cgamd_solver_spmv_moved_bytes(s));
    if (s->blk_want) return matrix + kBlockPasses * s->n_user * V * s->nrhs;
    if (s->pre.mg) return matrix + mg_bytes(s, cgamd_solver_spmv_moved_bytes(s));
    if (tri_on(s)) return matrix + tri_passes(s) * s->n_user * V;
    // the deferred x update: the d steps of a group of L iterations move 4 L + 1 vectors instead of 5 L, the steady state of a
    // handle iterated in multiples of U: (9 L + 1) / L passes per iteration
    if (lag >= 2) return matrix + (9 * lag + 1) * s->n_user * V * s->nrhs / lag;
    return matrix + passes * s->n_user * V * s->nrhs + shift_bytes(s);
}


// ---- solution projection (include/cgamd.h "Solution projection"; kernels: projection.hip) -----------------------------------------
static unsigned proj_held_mask(const cgamd_solver *s) { return s->proj.m >= 32 ? 0xffffffffu : ((1u << s->proj.m) - 1u); }
// what every entry checks first: the handle, no capture in progress
static int proj_entry(cgamd_solver *s, const char *who) {
    if (!s) return fail(CGAMD_ERR_INVALID, std::string(who) + ": solver is NULL");
    CG_HIP(hipSetDevice(s->ctx->device));
    return step_not_capturing(s, who);
}
static int proj_refuses(const cgamd_solver *s, const char *who) {
    if (s->rm || (s->rm_ok && !precond_set(s)))
        return fail(CGAMD_ERR_STATE, std::string(who) + ": the handle keeps its right-hand sides interleaved (row-major layout)");
    if (s->herm) return herm_refuses(who, "whose conjugated projection is a later change");
    return CGAMD_OK;
}

int cgamd_solver_projection_enable(cgamd_solver *s, int capacity, double drop_tol) {
    if (!s) return fail(CGAMD_ERR_INVALID, "projection_enable: solver is NULL");
    if (capacity < 0 || capacity > kProjMaxSlots) return fail(CGAMD_ERR_INVALID, "projection_enable: capacity runs 0 ... 32");
    if (!(drop_tol >= 0.) || !std::isfinite(drop_tol)) return fail(CGAMD_ERR_INVALID, "projection_enable: drop_tol must be finite and >= 0");
    TuneScope ts(&s->tune);
    if (int rc = proj_entry(s, "projection_enable")) return rc;
    if (capacity == 0) {
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        proj_free(s);
        return CGAMD_OK;
    }
    if (int rc = proj_refuses(s, "projection_enable")) return rc;
    const int nr = s->nrhs;
    const size_t vs = dtype_size(s->dtype), as = acc_size(s->dtype), block = (size_t)s->n * nr * vs;
    cgamd_solver::Projection p;
    p.cap = capacity;
    p.drop_tol = drop_tol;
    p.grid = proj_dots_grid(s->dtype, s->n);
    // alpha | c | t (values), then eq | nu | nus (accumulators, 16-byte aligned), then the flags
    const size_t n_val = ((size_t)2 * capacity * nr + nr) * vs, at_acc = (n_val + 15) & ~(size_t)15, n_acc = (size_t)4 * nr * as;
    const size_t scal_bytes = at_acc + n_acc + (size_t)nr * sizeof(int);
    const size_t part_bytes = as * (size_t)capacity * nr * p.grid;
    int rc = dmalloc(&p.W, block * capacity, "projection basis");
    if (!rc) rc = dmalloc(&p.x0, block, "projection guess");
    if (!rc) rc = dmalloc(&p.scal, scal_bytes, "projection scalars");
    if (!rc) rc = dmalloc(&p.partials, part_bytes, "projection partials");
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(p.W, 0, block * capacity, s->ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(p.x0, 0, block, s->ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(p.scal, 0, scal_bytes, s->ctx->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
    if (rc || e != hipSuccess) {        // the handle keeps what it had
        for (void *q : {p.W, p.x0, p.scal, p.partials})
            if (q) (void)hipFree(q);
        return rc ? rc : fail(CGAMD_ERR_HIP, std::string("projection_enable: ") + hipGetErrorString(e));
    }
    char *base = static_cast<char *>(p.scal);
    p.alpha = base;
    p.c = base + (size_t)capacity * nr * vs;
    p.t = base + (size_t)2 * capacity * nr * vs;
    p.eq = base + at_acc;
    p.nu = base + at_acc + (size_t)nr * as;
    p.nus = base + at_acc + (size_t)2 * nr * as;
    p.added = reinterpret_cast<int *>(base + at_acc + n_acc);
    proj_free(s);
    s->proj = p;
    return CGAMD_OK;
}

int cgamd_solver_projection_count(cgamd_solver *s) { return s ? (s->proj.cap ? s->proj.m : 0) : -CGAMD_ERR_INVALID; }

int cgamd_solver_projection_clear(cgamd_solver *s) {
    if (int rc = proj_entry(s, "projection_clear")) return rc;
    proj_clear(s);
    return CGAMD_OK;
}

int cgamd_solver_set_rhs_projected(cgamd_solver *s, const void *b, int on_device) {
    if (!s || !b) return fail(CGAMD_ERR_INVALID, "set_rhs_projected: null argument");
    TuneScope ts(&s->tune);
    if (int rc = proj_entry(s, "set_rhs_projected")) return rc;
    if (int rc = shifts_refuse(s, "set_rhs_projected", false)) return rc;      // (the shifted systems start from x0 = 0; block CG takes any x0)
    if (!s->proj.cap) return fail(CGAMD_ERR_STATE, "set_rhs_projected: call cgamd_solver_projection_enable first");
    if (int rc = proj_refuses(s, "set_rhs_projected")) return rc;
    hipStream_t st = s->ctx->stream;
    const int dt = s->dtype, n = s->n, nr = s->nrhs;
    const size_t vs = dtype_size(dt), vbytes = (size_t)n * nr * vs;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    s->rhs_set = false;         // b changes under the handle: only a completed set_rhs makes it usable again
    s->proj.projected = s->proj.spent = false;
    // b as cgamd_solver_set_rhs places it (the padding rows stay 0)
    if (n != s->n_user) CG_HIP(hipMemcpy2DAsync(s->b, (size_t)n * vs, b, (size_t)s->n_user * vs, (size_t)s->n_user * vs, (size_t)nr, kind, st));
    else CG_HIP(hipMemcpyAsync(s->b, b, vbytes, kind, st));
    // the guess: alpha_j = <w_j, b>, x0 = sum_j alpha_j w_j
    const unsigned held = proj_held_mask(s);
    const long long pitch = (long long)n * nr;
    if (s->proj.m > 0) {
        if (int rc = launch_proj_dots(dt, n, n, s->proj.cap, held, s->proj.W, pitch, s->b, nr, s->proj.partials, s->proj.grid, s->proj.alpha, st)) return rc;
        if (int rc = launch_proj_combine(dt, n, n, s->proj.cap, held, s->proj.W, pitch, nullptr, nullptr, s->proj.alpha, +1, s->proj.x0, nr, st)) return rc;
    } else {
        CG_HIP(hipMemsetAsync(s->proj.x0, 0, vbytes, st));
    }
    CG_HIP(hipMemcpyAsync(s->x, s->proj.x0, vbytes, hipMemcpyDeviceToDevice, st));
    // everything after the guess is cgamd_solver_set_rhs(b, x0): b and x are in place
    if (int rc = set_rhs_impl(s, nullptr, nullptr, on_device, s->n_user)) return rc;
    s->proj.projected = true;
    return CGAMD_OK;
}

int cgamd_solver_projection_update(cgamd_solver *s, int *added) {
    if (!s) return fail(CGAMD_ERR_INVALID, "projection_update: solver is NULL");
    TuneScope ts(&s->tune);
    if (int rc = proj_entry(s, "projection_update")) return rc;
    if (!s->proj.cap) return fail(CGAMD_ERR_STATE, "projection_update: call cgamd_solver_projection_enable first");
    if (!s->rhs_set || !s->proj.projected)
        return fail(CGAMD_ERR_STATE, "projection_update: the right-hand side in force did not come through cgamd_solver_set_rhs_projected");
    if (s->proj.spent) return fail(CGAMD_ERR_STATE, "projection_update: already updated from this solve");
    hipStream_t st = s->ctx->stream;
    cgamd_solver::Projection &p = s->proj;
    const int dt = s->dtype, n = s->n, nr = s->nrhs, cap = p.cap;
    const long long pitch = (long long)n * nr;
    const int retired = p.m == cap ? p.head : -1;       // a full ring: the oldest slot takes no part and receives the new vector
    const unsigned held = proj_held_mask(s), live = retired >= 0 ? held & ~(1u << retired) : held;
    void *e = s->d;             // the direction is dead from here on: iterate* refuse until the next set_rhs
    p.spent = true;
    int rc;
    // e = x - x0, plus what the retired slot carried of the guess (alpha_ret w_ret), so that the vector that takes its place keeps it:
    // e is what the solve found beyond the span of the slots that STAY.  Then q = A e ; c_j = <w_j, q> ; <e, q>
    if ((rc = launch_proj_combine(dt, n, n, cap, retired >= 0 ? 1u << retired : 0u, p.W, pitch, s->x, p.x0, p.alpha, +1, e, nr, st))) return rc;
    if ((rc = handle_spmv(s, n, e, n, s->q, n, nullptr, nullptr, st))) return rc;
    if ((rc = launch_proj_dots(dt, n, n, cap, live, p.W, pitch, s->q, nr, p.partials, p.grid, p.c, st))) return rc;
    if ((rc = launch_dot_partials(dt, n, e, s->q, n, nr, p.partials, p.grid, st))) return rc;
    if ((rc = launch_reduce_to_acc(dt, p.partials, p.grid, nr, p.eq, st))) return rc;
    // e' = e - sum_j c_j w_j ; q' = A e' ; nu = <e', q'>
    if (live && (rc = launch_proj_combine(dt, n, n, cap, live, p.W, pitch, e, nullptr, p.c, -1, e, nr, st))) return rc;
    if ((rc = handle_spmv(s, n, e, n, s->q, n, nullptr, nullptr, st))) return rc;
    if ((rc = launch_dot_partials(dt, n, e, s->q, n, nr, p.partials, p.grid, st))) return rc;
    if ((rc = launch_reduce_to_acc(dt, p.partials, p.grid, nr, p.nu, st))) return rc;
    if ((rc = launch_proj_decide(dt, nr, cap, live, live, p.alpha, p.c, p.eq, p.nu, p.drop_tol, p.nus, p.t, p.added, st))) return rc;
    std::vector<int> flags((size_t)nr, 0);
    CG_HIP(hipMemcpyAsync(flags.data(), p.added, sizeof(int) * (size_t)nr, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    bool any = false;
    for (int f : flags) any = any || f != 0;
    if (any) {          // one slot for all columns: a refused column stores zeros
        const int slot = retired >= 0 ? retired : p.m;
        void *w = static_cast<char *>(p.W) + (size_t)slot * pitch * dtype_size(dt);
        if ((rc = launch_proj_store(dt, n, e, n, p.t, p.added, w, nr, st))) return rc;
        if (retired >= 0) p.head = (p.head + 1) % cap;
        else ++p.m;
    }
    if (added)
        for (int r = 0; r < nr; ++r) added[r] = flags[(size_t)r];
    return CGAMD_OK;
}

int cgamd_solver_projection_state(cgamd_solver *s, int which, int slot, void *out_host) {
    if (!s || !out_host) return fail(CGAMD_ERR_INVALID, "projection_state: null argument");
    if (int rc = proj_entry(s, "projection_state")) return rc;
    const cgamd_solver::Projection &p = s->proj;
    if (!p.cap) return fail(CGAMD_ERR_STATE, "projection_state: call cgamd_solver_projection_enable first");
    hipStream_t st = s->ctx->stream;
    const int nr = s->nrhs;
    const size_t vs = dtype_size(s->dtype), row = (size_t)s->n_user * vs;
    switch (which) {
    case 0:
        if (slot < 0 || slot >= p.cap) return fail(CGAMD_ERR_INVALID, "projection_state: slot runs 0 ... capacity - 1");
        CG_HIP(hipMemcpy2DAsync(out_host, row, static_cast<const char *>(p.W) + (size_t)slot * s->n * nr * vs, (size_t)s->n * vs, row, (size_t)nr,
                                hipMemcpyDeviceToHost, st));
        break;
    case 1: CG_HIP(hipMemcpy2DAsync(out_host, row, p.x0, (size_t)s->n * vs, row, (size_t)nr, hipMemcpyDeviceToHost, st)); break;
    case 2: CG_HIP(hipMemcpyAsync(out_host, p.alpha, (size_t)p.cap * nr * vs, hipMemcpyDeviceToHost, st)); break;
    case 3: CG_HIP(hipMemcpyAsync(out_host, p.c, (size_t)p.cap * nr * vs, hipMemcpyDeviceToHost, st)); break;
    case 4: CG_HIP(hipMemcpyAsync(out_host, p.nus, (size_t)2 * nr * acc_size(s->dtype), hipMemcpyDeviceToHost, st)); break;
    default: return fail(CGAMD_ERR_INVALID, "projection_state: which is 0 .. 4");
    }
    CG_HIP(hipStreamSynchronize(st));
    return CGAMD_OK;
}

// ---- multi-shift CG (include/cgamd.h "Multi-shift CG"; kernels: shifts.hip) ------------------------------------------------------
// what every entry checks first: the handle, no capture in progress
static int shift_entry(cgamd_solver *s, const char *who) {
    if (!s) return fail(CGAMD_ERR_INVALID, std::string(who) + ": solver is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(s->ctx->device));
    return step_not_capturing(s, who);
}

int cgamd_solver_set_shifts(cgamd_solver *s, const void *sigma, int nShifts) {
    const std::string who = "set_shifts";
    if (int rc = shift_entry(s, "set_shifts")) return rc;
    if (nShifts < 0 || nShifts > kShiftMax) return fail(CGAMD_ERR_INVALID, who + ": nShifts runs 0 ... 16");
    TuneScope ts(&s->tune);
    hipStream_t st = s->ctx->stream;
    if (!sigma || nShifts == 0) {       // removal: the next set_rhs starts a handle that never had shifts
        if (!nshifts(s)) return CGAMD_OK;
        CG_HIP(hipStreamSynchronize(st));
        shifts_free(s);
        destroy_graphs(s);
        s->rhs_set = false;
        s->until_mode = s->until_stopped = false;       // (the loop the shifts asked for; set_rhs decides anew)
        return CGAMD_OK;
    }
    if (int rc = block_refuses(s, "set_shifts")) return rc;
    if (s->nsys) return fail(CGAMD_ERR_STATE, who + ": the handle is batched (a matrix of its own per right-hand side)");
    if (s->herm) return herm_refuses("set_shifts", "which the shifted recurrence does not serve yet");
    if (s->flags & CGAMD_UNFUSED) return fail(CGAMD_ERR_STATE, who + ": CGAMD_UNFUSED replays the reference's kernel sequence");
    if (s->rm_ok) return fail(CGAMD_ERR_STATE, who + ": the handle keeps its right-hand sides interleaved (row-major layout)");
    if (precond_set(s)) return fail(CGAMD_ERR_STATE, who + ": a preconditioner is in force, and a preconditioned operator is not a shift of anything; remove it first");
    // sigma in the accumulator type, as the scalar step reads it
    const bool cplx = s->dtype == CGAMD_C64 || s->dtype == CGAMD_C128, single = s->dtype == CGAMD_F32 || s->dtype == CGAMD_C64;
    const int parts = cplx ? 2 : 1;
    std::vector<double> sig((size_t)nShifts * parts);
    for (size_t i = 0; i < sig.size(); ++i) {
        sig[i] = single ? (double)static_cast<const float *>(sigma)[i] : static_cast<const double *>(sigma)[i];
        if (!std::isfinite(sig[i])) return fail(CGAMD_ERR_INVALID, who + ": shift " + std::to_string(i / parts) + " is not finite");
    }
    // everything is allocated before the handle changes
    const int nr = s->nrhs;
    const size_t vs = dtype_size(s->dtype), as = acc_size(s->dtype), pairs = (size_t)nShifts * nr;
    const size_t scal_bytes = as * (size_t)nShifts + 4 * as * pairs + 3 * vs * pairs;
    cgamd_solver::Shifts nw;
    int rc = dmalloc(&nw.vec, 2 * pairs * (size_t)s->n * vs, "shifted solutions and directions");
    if (!rc) rc = dmalloc(&nw.scal, scal_bytes, "shift scalars");
    if (!rc) rc = dmalloc(&nw.view.history, (size_t)s->sc.history_cap * pairs * vs, "shift history");
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(nw.scal, sig.data(), as * (size_t)nShifts, hipMemcpyHostToDevice, st);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);       // (sig goes away; work of the old shifts has drained)
    if (!rc && e != hipSuccess) rc = fail(CGAMD_ERR_HIP, who + ": " + hipGetErrorString(e));
    if (rc) {
        for (void *p : {nw.vec, nw.scal, nw.view.history})
            if (p) (void)hipFree(p);
        return rc;
    }
    char *p = static_cast<char *>(nw.scal);
    ShiftScalars &v = nw.view;
    v.S = nShifts;
    v.history_cap = s->sc.history_cap;
    v.sigma = p; p += as * (size_t)nShifts;
    v.theta = p; p += as * pairs;
    v.zeta = p; p += as * pairs;
    v.aprev = p; p += as * pairs;
    v.bprev = p; p += as * pairs;
    v.alpha_s = p; p += vs * pairs;
    v.beta_s = p; p += vs * pairs;
    v.zeta_s = p;
    shifts_free(s);
    s->sh = nw;
    destroy_graphs(s);      // another loop from the next set_rhs on
    s->rhs_set = false;
    return CGAMD_OK;
}

int cgamd_solver_shifts(cgamd_solver *s) { return s ? nshifts(s) : -CGAMD_ERR_INVALID; }

// what the entries below ask for: shifts in force and a right-hand side they have started from
static int shifts_running(cgamd_solver *s, const std::string &who) {
    if (!nshifts(s)) return fail(CGAMD_ERR_STATE, who + ": no shifts are in force (cgamd_solver_set_shifts)");
    if (!s->rhs_set) return fail(CGAMD_ERR_STATE, who + ": call set_rhs first");
    return CGAMD_OK;
}

int cgamd_solver_get_x_shifted(cgamd_solver *s, int j, void *x, int on_device) {
    if (int rc = shift_entry(s, "get_x_shifted")) return rc;
    if (!x) return fail(CGAMD_ERR_INVALID, "get_x_shifted: x is NULL");
    if (int rc = shifts_running(s, "get_x_shifted")) return rc;
    if (j < 0 || j >= nshifts(s)) return fail(CGAMD_ERR_INVALID, "get_x_shifted: j runs 0 ... shifts - 1");
    const size_t vs = dtype_size(s->dtype), row = (size_t)s->n_user * vs;
    const char *src = static_cast<const char *>(shift_xs(s)) + (size_t)j * s->nrhs * s->n * vs;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    CG_HIP(hipMemcpy2DAsync(x, row, src, (size_t)s->n * vs, row, (size_t)s->nrhs, kind, s->ctx->stream));
    if (!on_device) CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

int cgamd_solver_shift_history(cgamd_solver *s, void *out, int max_entries) {
    if (int rc = shift_entry(s, "shift_history")) return -rc;
    if (!out) return -fail(CGAMD_ERR_INVALID, "shift_history: out is NULL");
    if (int rc = shifts_running(s, "shift_history")) return -rc;
    const ShiftScalars &v = s->sh.view;
    const int entries = std::max(0, std::min(std::min(s->iters + 1, v.history_cap), max_entries));
    hipError_t e = hipMemcpyAsync(out, v.history, (size_t)entries * v.S * s->nrhs * dtype_size(s->dtype), hipMemcpyDeviceToHost, s->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
    if (e != hipSuccess) return -fail(CGAMD_ERR_HIP, std::string("shift_history: ") + hipGetErrorString(e));
    return entries;
}

// which: 0 theta, 1 zeta (double / complex double), 2 alpha_j, 3 beta_j (value type); shifts x nRHS values at [j * nRHS + r]
int cgamd_solver_shift_scalars(cgamd_solver *s, int which, void *out_host) {
    if (int rc = shift_entry(s, "shift_scalars")) return rc;
    if (!out_host) return fail(CGAMD_ERR_INVALID, "shift_scalars: out_host is NULL");
    if (int rc = shifts_running(s, "shift_scalars")) return rc;
    const ShiftScalars &v = s->sh.view;
    if (which < 0 || which > 3) return fail(CGAMD_ERR_INVALID, "shift_scalars: which is 0 .. 3");
    const void *src = which == 0 ? v.theta : which == 1 ? v.zeta : which == 2 ? v.alpha_s : v.beta_s;
    const size_t each = which < 2 ? acc_size(s->dtype) : dtype_size(s->dtype);
    CG_HIP(hipMemcpyAsync(out_host, src, each * (size_t)v.S * s->nrhs, hipMemcpyDeviceToHost, s->ctx->stream));
    CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

// ---- block CG (include/cgamd.h "Block CG"; kernels: block_cg.hip) -----------------------------------------------------------------
int cgamd_solver_set_block(cgamd_solver *s, int on) {
    const std::string who = "set_block";
    if (int rc = shift_entry(s, "set_block")) return rc;
    TuneScope ts(&s->tune);
    if (s->blk_pcg) return fail(CGAMD_ERR_STATE, who + ": preconditioned block CG is on (cgamd_solver_set_block_pcg); the two modes exclude each other: turn it off there");
    if (!on) {          // the next set_rhs starts a handle that never had it
        if (!s->blk_want && !s->blk_on) return CGAMD_OK;
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        block_drop(s);
        return CGAMD_OK;
    }
    if (s->dtype != CGAMD_F32 && s->dtype != CGAMD_F64)
        return fail(CGAMD_ERR_STATE, who + ": block CG serves the real value types (the unconjugated block recurrence diverged on complex symmetric operators; the Hermitian form is a later piece of work)");
    if (s->nsys) return fail(CGAMD_ERR_STATE, who + ": the handle is batched (a matrix of its own per right-hand side: no common Krylov space)");
    if (s->flags & CGAMD_UNFUSED) return fail(CGAMD_ERR_STATE, who + ": CGAMD_UNFUSED replays the reference's kernel sequence");
    if (s->rm_ok) return fail(CGAMD_ERR_STATE, who + ": the handle keeps its right-hand sides interleaved (row-major layout)");
    if (s->nrhs < 2 || s->nrhs > kBlockMax) return fail(CGAMD_ERR_STATE, who + ": the block is the handle's nRHS right-hand sides, 2 ... 16 of them");
    if (precond_set(s)) return fail(CGAMD_ERR_STATE, who + ": a preconditioner is in force; remove it first");
    if (nshifts(s)) return fail(CGAMD_ERR_STATE, who + ": shifts are in force (cgamd_solver_set_shifts); remove them first");
    if (s->blk_want) return CGAMD_OK;
    if (int rc = block_alloc(&s->blk, s->nrhs, s->n)) return rc;
    s->blk_want = true;     // (blk_on, and with it the loop, changes at the next set_rhs)
    return CGAMD_OK;
}

// Preconditioned block CG (include/cgamd.h "Preconditioned block CG"; block_pcg.hip): legal only WITH a preconditioner in force, which
// becomes part of the block's state -- every set_preconditioner* entry refuses the handle while the mode is on
int cgamd_solver_set_block_pcg(cgamd_solver *s, int on) {
    const std::string who = "set_block_pcg";
    if (int rc = shift_entry(s, "set_block_pcg")) return rc;
    TuneScope ts(&s->tune);
    if (s->blk_want && !s->blk_pcg) return fail(CGAMD_ERR_STATE, who + ": block CG is on (cgamd_solver_set_block); the two modes exclude each other: turn it off there");
    if (!on) {          // the next set_rhs starts the scalar PCG handle it was
        if (!s->blk_pcg) return CGAMD_OK;
        CG_HIP(hipStreamSynchronize(s->ctx->stream));
        block_drop(s);
        return CGAMD_OK;
    }
    if (s->dtype != CGAMD_F32 && s->dtype != CGAMD_F64)
        return fail(CGAMD_ERR_STATE, who + ": block CG serves the real value types");
    if (s->nsys) return fail(CGAMD_ERR_STATE, who + ": the handle is batched (a matrix of its own per right-hand side: no common Krylov space)");
    if (s->herm) return herm_refuses("set_block_pcg", "which the block recurrence does not serve");
    if (s->flags & CGAMD_UNFUSED) return fail(CGAMD_ERR_STATE, who + ": CGAMD_UNFUSED replays the reference's kernel sequence");
    if (s->rm_ok) return fail(CGAMD_ERR_STATE, who + ": the handle keeps its right-hand sides interleaved (row-major layout)");
    if (s->nrhs < 2 || s->nrhs > kBlockMax) return fail(CGAMD_ERR_STATE, who + ": the block is the handle's nRHS right-hand sides, 2 ... 16 of them");
    if (nshifts(s)) return fail(CGAMD_ERR_STATE, who + ": shifts are in force (cgamd_solver_set_shifts); remove them first");
    if (!precond_set(s)) return fail(CGAMD_ERR_STATE, who + ": no preconditioner is in force; install one first (cgamd_solver_set_block runs the unpreconditioned block)");
    if (s->blk_pcg) return CGAMD_OK;
    if (int rc = block_alloc(&s->blk, s->nrhs, s->n)) return rc;
    if (int rc = block_pcg_alloc(&s->blk)) { block_free(&s->blk); return rc; }
    s->blk_want = s->blk_pcg = true;    // (blk_on, and with it the loop, changes at the next set_rhs)
    return CGAMD_OK;
}

int cgamd_solver_block_status(cgamd_solver *s, int *info, double *min_pivot_ratio) {
    if (int rc = shift_entry(s, "block_status")) return rc;
    if (!info) return fail(CGAMD_ERR_INVALID, "block_status: info is NULL");
    info[0] = s->blk_want ? (s->blk_pcg ? 2 : 1) : 0; info[1] = 0; info[2] = 0; info[3] = s->nrhs;
    if (min_pivot_ratio) *min_pivot_ratio = INFINITY;
    if (!s->blk_on || !s->rhs_set) return CGAMD_OK;
    struct { int rec[4]; double ratio; } img;
    int it = 0;
    hipStream_t st = s->ctx->stream;
    CG_HIP(hipMemcpyAsync(&img, s->blk.dev.rec, sizeof(img), hipMemcpyDeviceToHost, st));
    CG_HIP(hipMemcpyAsync(&it, s->sc.iter, sizeof(int), hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    info[1] = img.rec[0]; info[2] = img.rec[1];
    if (min_pivot_ratio) *min_pivot_ratio = img.ratio;
    if (img.rec[0]) s->iters = it;      // a breakdown froze the loop there, whatever was enqueued behind it
    return CGAMD_OK;
}

// which: 0 xi, 1 G = P^T A P, 2 alpha = G^-1, 3 tau, 4 W^T W (R0^T R0 after set_rhs), 5 tau^-1, 6 M = alpha xi; s x s doubles, row-major
// the preconditioned mode alone: 7 W^T Z (R0^T Z0 after set_rhs) as summed
int cgamd_solver_block_state(cgamd_solver *s, int which, void *out_host) {
    if (int rc = shift_entry(s, "block_state")) return rc;
    if (!out_host) return fail(CGAMD_ERR_INVALID, "block_state: out_host is NULL");
    if (!s->blk_on || !s->rhs_set) return fail(CGAMD_ERR_STATE, "block_state: block CG is not running (cgamd_solver_set_block, then set_rhs)");
    if (which < 0 || which > (s->blk_pcg ? 7 : 6)) return fail(CGAMD_ERR_INVALID, s->blk_pcg ? "block_state: which is 0 .. 7" : "block_state: which is 0 .. 6");
    const BlockDev &d = s->blk.dev;
    const double *src[] = {d.xi, d.G, d.alpha, d.tau, d.C, d.tau_inv, d.M, d.CZ};
    CG_HIP(hipMemcpyAsync(out_host, src[which], sizeof(double) * (size_t)s->nrhs * s->nrhs, hipMemcpyDeviceToHost, s->ctx->stream));
    CG_HIP(hipStreamSynchronize(s->ctx->stream));
    return CGAMD_OK;
}

}  // extern "C"

// ---- what the mixed-precision solve (mixed.cpp) needs of its two handles beyond the C ABI (cgamd_internal.h) ----
namespace cgamd {
const void *solver_matrix(cgamd_solver *s, const int **ptr, const int **cols) {
    *ptr = s->ptr; *cols = s->cols;
    return s->vals;
}
int solver_restart(cgamd_solver *s) {
    if (!s->rhs_set) return fail(CGAMD_ERR_STATE, "mixed_solve: the outer handle has no right-hand side");
    return set_rhs_impl(s, nullptr, nullptr, 1, s->n);
}
int solver_set_rhs_ld(cgamd_solver *s, const void *b, long long ldb) { return set_rhs_impl(s, b, nullptr, 1, ldb); }
int solver_replace_residual_ld(cgamd_solver *s, const void *r_new, long long ldr) { return replace_residual_impl(s, r_new, ldr); }
bool solver_block_on(const cgamd_solver *s) { return s->blk_want; }
int solver_replace_planned(cgamd_solver *s) {
    TuneScope ts(&s->tune);
    return replace_refuses(s, true);
}
}  // namespace cgamd
