// The single-GPU handle (single and batched) and the helpers its files share: solver.cpp (creation, the matrix life cycle, the loops,
// the accessors) and solver_precond.cpp (the preconditioner entries).  Private to those two files.
#pragma once
#include <string>
#include <vector>

#include "cgamd_internal.h"
#include "precond_state.h"

struct cgamd_solver {
    cgamd::Tuning tune;            // configuration this handle was created under (installed per call: TuneScope)
    cgamd_ctx *ctx = nullptr;
    int dtype = 0, n = 0, nrhs = 1, flags = 0;
    // n is the size every kernel of the handle works on; n_user the caller's.  They differ when `size` is not a whole number of
    // 16-byte packs (odd sizes in fp64 / complex64, not a multiple of 4 in fp32): the system is then carried with 1-3 EMPTY rows
    // appended (row pointers repeated, b = x0 = 0 there, so r, d, q and x stay exactly 0 in them and every sum gains exact zeros),
    // which keeps every right-hand side's vectors 16-byte aligned: the vectorised multi-RHS kernels and the resident loops apply
    // to any size.  The caller's arrays keep their own stride (strided copies in set_rhs / get_x).
    int n_user = 0;
    // cgamd_solver_create_batched: nsys systems on one pattern, the values of system r at vals + r * nnz and right-hand side r its
    // own; 0 = every other handle (one matrix for all right-hand sides).  A batched handle has nrhs == nsys, runs the launched loops
    // only (no resident loop, no row-major layout, no codes) and launches its SpMV through launch_spmv_batched.  Its preconditioner is
    // one M per system (cgamd_solver_set_preconditioner_batched*): mdiag holds nsys diagonals at stride n, tri the factors of every
    // system at tri.fpitch on one segment plan.
    int nsys = 0;
    // CGAMD_HERMITIAN on a complex value type (hermitian.hip): the conjugated recurrence, on a four-launch loop of its own -- no
    // resident, chip-wide or two-launch loop, no row-major layout, no deferred x update.  dc = conj(d), the vector of the SpMV's fused
    // dot, lives in the d2 slot, which those loops alone use.  Never set for the real types: the flag changes nothing there.
    bool herm = false;
    bool own_ptr = false;   // a borrowed device matrix whose row pointers were copied to append the padding rows
    long long nnz = 0;
    void *vals = nullptr;
    int *ptr = nullptr, *cols = nullptr;
    bool own_matrix = false;
    std::vector<int> ptr_host;   // own_matrix: the row pointers as uploaded (cgamd_solver_reload_matrix compares against them)
    cgamd::SpmvPlan plan;
    int vgrid = 1;
    void *x = nullptr, *r = nullptr, *d = nullptr, *q = nullptr, *b = nullptr;
    void *slab = nullptr;   // backing store of x, r, d, q, b
    void *part_dq = nullptr, *part_rr = nullptr;
    size_t part_dq_cap = 0;      // entries per RHS
    // the preconditioner in force (precond_state.h): what M is (pre.kind decides the loop family), what it was built from and so what
    // cgamd_solver_reload_matrix / _refresh_values build again (pre.built), and the memory that belongs to it.  A batched handle keeps
    // one M per system in the same fields.  z lives in q's storage for the line sweeps and the V-cycle (q is dead between the r update
    // and the next SpMV).  part_rz: the r.z partials of the diagonal and multigrid loops, sized like part_rr (part_rr_cap per RHS),
    // allocated at the first such M and kept; the line sweeps have partials of their own grid (pre.tri_part)
    cgamd::Precond pre;
    void *part_rz = nullptr;
    cgamd::CgScalars sc;
    bool rhs_set = false;
    int iters = 0;  // iterations enqueued since set_rhs
    // captured iteration sequences, per parity of the iteration count they start at (the two-launch loop ping-pongs d)
    hipGraphExec_t g1[2] = {nullptr, nullptr}, gU[2] = {nullptr, nullptr};
    hipGraph_t g1g[2] = {nullptr, nullptr}, gUg[2] = {nullptr, nullptr};
    int U = 8;
    bool graph_failed = false;
    // row-major multi-RHS path (rowmajor.hip): x, r, d, q, b hold [n][nrhs]; rm_ok is decided at creation, `rm` per set_rhs
    bool rm_ok = false, rm = false;
    int rm_nwg = 0, rm_vgrid = 0;
    size_t part_rr_cap = 0;
    int *rm_pace = nullptr;     // progress counters of the paced SpMM sweep (kSpmmPaceInts, zero between launches)
    // event hooks around the SpMV launch of enqueue_iteration (cgamd_solver_iterate_timed)
    hipEvent_t *ev_pair = nullptr;
    // two-launch loop (small systems): d of iteration k lives in dbuf[k & 1] (dbuf[0] = d, the initial r); decided at creation
    bool fused2 = false;
    void *d2 = nullptr;
    // x brought up to date once per x_lag iterations inside a captured U-iteration graph of the three / four-launch loop (vector.hip):
    // direction buffer 0 = d, 1 = d2, 2 .. x_lag - 1 in dlag.  Decided by setup_x_lag; 1 = x updated in every iteration
    int x_lag = 1;
    void *dlag = nullptr;
    size_t dlag_pitch = 0;
    int dlag_bufs = 0;
    // resident loop (resident.hip): iterate() calls of a small system in ONE launch; decided with fused2
    bool res_ok = false;
    cgamd::ResidentPlan res;
    void *res_sync = nullptr;
    int n_cus = 0;
    // wide resident loop: one chip-wide group for a single right-hand side (resident.hip)
    cgamd::ResidentWidePlan resw;
    void *resw_sync = nullptr;
    unsigned char *codes = nullptr;   // one-byte column codes of the single-RHS SpMV (build_index_codes), with their dictionary
    int *dict = nullptr;
    int n_offsets = 0;                // distinct (column - row) offsets behind the codes; 0 = the SpMV reads aCols
    unsigned char *vcodes = nullptr;  // one-byte value codes on top of the one-byte column codes (build_value_codes), with their dictionary
    void *vdict = nullptr;
    int n_values = 0;                 // distinct matrix entries behind the value codes; 0 = the SpMV reads aValues
    unsigned char *jcodes = nullptr;  // one-byte joint (offset, value) codes where at most 256 pairs occur (build_joint_codes)
    int *jdict_off = nullptr;
    void *jdict_val = nullptr;
    int n_pairs = 0;
    unsigned char *rcodes = nullptr;  // one-byte row-pattern codes where at most 256 patterns of at most 7 entries occur (build_row_codes)
    void *rdict = nullptr;            // their dictionary: values, byte offsets, lengths (row_dict_bytes)
    unsigned char *pcodes = nullptr;  // one byte per PAIR of rows on top of the row codes (build_row_pairs), and their dictionary
    void *pdict = nullptr;
    int n_pair_patterns = 0;
    int n_patterns = 0, n_user_patterns = 0;     // dictionary entries; patterns of the caller's rows (the appended empty rows may add one)
    int *sched = nullptr;             // plane-matched XCD schedule of the row- / pair-coded SpMV (setup_xcd_schedule): plan.sched_grid ints
    long long sched_unit = 0;         // the largest |column - row| among the row dictionary's entries, in rows (0: no row codes)
    // cgamd_solver_iterate_tol: tolerance of the device-side stop for the call in progress (0 = none), and what it reported
    double tol_req = 0.;
    bool tol_served = false, tol_stopped = false;
    // cgamd_solver_iterate_until: the per-right-hand-side stop (StopRun: allocated at the first call, armed once per set_rhs) and the
    // captured chunk of guarded iterations.  until_mode: since the first call after set_rhs the handle runs its three / four-launch
    // loop only (d in one buffer, updated at the end of every iteration); until_stopped: a right-hand side has stopped, so the columns
    // are at different iterations and only iterate_until goes on.
    cgamd::StopRun stop;
    bool until_mode = false, until_stopped = false;
    hipGraphExec_t gT = nullptr;
    hipGraph_t gTg = nullptr;
    int gT_len = 0;
    int last_refresh = 0;           // what the last cgamd_solver_refresh_values did (cgamd_solver_last_refresh)
    // solution projection (cgamd_solver_projection_enable; projection.hip): `cap` slots of nrhs vectors at stride n each, `m` of them
    // held; once m == cap the slots form a ring and `head` is the oldest.  One allocation `scal` holds alpha and c (cap x nrhs values
    // each), t (nrhs values), <e, q>, nu and the (nu, s) record (accumulators) and the added flags.  projected: the right-hand side in
    // force came through cgamd_solver_set_rhs_projected; spent: its update has run (q and d hold the update's vectors: set_rhs is next)
    struct Projection {
        int cap = 0, m = 0, head = 0, grid = 0;
        double drop_tol = 0.;
        void *W = nullptr, *x0 = nullptr, *scal = nullptr, *partials = nullptr;
        void *alpha = nullptr, *c = nullptr, *t = nullptr, *eq = nullptr, *nu = nullptr, *nus = nullptr;
        int *added = nullptr;
        bool projected = false, spent = false;
    } proj;
    int captures = 0;               // graphs captured since creation (cgamd_solver_graph_captures)
    // multi-shift CG (cgamd_solver_set_shifts; shifts.hip): view.S shifted systems ride on the seed recurrence.  vec = x_j then d_j,
    // [2][S][nrhs][n] values; scal = sigma, the state and the coefficients behind `view`; view.history = zeta_k, grown with the seed's
    // history (ensure_history).  While view.S > 0 every set_rhs puts the handle into until_mode: the three / four-launch loop alone,
    // d in one buffer, x updated in every iteration, and behind its d step the two launches of shifts.hip
    struct Shifts {
        cgamd::ShiftScalars view;
        void *vec = nullptr, *scal = nullptr;
    } sh;
    // block CG (cgamd_solver_set_block; block_cg.hip): the nrhs right-hand sides share one Krylov space.  blk_want: what the caller
    // asked for, in force from the next set_rhs; blk_on: the right-hand side in force runs the block loop -- x = X, r = Q, d = P,
    // q = A P, the SpMV and five launches per iteration, until_mode like every loop with d in one buffer.  blk: the small matrices,
    // the record and the Gram partials (allocated by set_block, no n-sized buffer)
    cgamd::BlockState blk;
    // blk_pcg (cgamd_solver_set_block_pcg; block_pcg.hip): the block loop is the preconditioned one -- the M in force sits inside the
    // recurrence, q also holds Z = M^-1 W, and blk carries W^T Z and its partials; set and cleared with blk_want
    bool blk_want = false, blk_on = false, blk_pcg = false;
};

namespace cgamd {

// a preconditioner is set: what decides the loop family
inline bool precond_set(const cgamd_solver *s) { return s->pre.kind != Precond::kNone; }
inline bool tri_on(const cgamd_solver *s) { return s->pre.kind == Precond::kTri; }
void destroy_graphs(cgamd_solver *s);
void apply_wide_order(cgamd_solver *s);
int setup_resident_wide_plan(cgamd_solver *s);
// refusals made before anything on the handle changes
int batched_refuses(const char *who);
int herm_refuses(const char *who, const char *why);
// block_too: the entry does not serve block CG either (cgamd_solver_set_block), which is every caller but set_rhs_projected
int shifts_refuse(const cgamd_solver *s, const char *who, bool block_too = true);
int block_refuses(const cgamd_solver *s, const char *who);
// block CG off, plain or preconditioned (the stream is idle): state freed, graphs gone, set_rhs next
void block_drop(cgamd_solver *s);
// (solver_precond.cpp) the matrix behind a preconditioner built from it has changed: build it again -- or, where that fails, remove
// it (the new values are in force, the old factors belong to the old ones) and fail with the build's status and text
int rebuild_or_remove(cgamd_solver *s, const char *who);
// the same removal where the values' own follow-up failed with status rc, whose text is in cgamd_last_error()
int remove_and_fail(cgamd_solver *s, int rc);

}  // namespace cgamd
