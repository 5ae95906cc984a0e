// Host-side internal interfaces between the kernel launchers (spmv.hip, vector.hip, p2p.hip, cg1.hip, index_codes.hip, rowmajor.hip, resident.hip, slab.hip, multigrid.hip), the solver
// (solver.cpp), the C ABI (api.cpp) and the multi-GPU loop (dist.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cgamd.h"
#include "mg_params.h"
#include "spmv_form.h"

namespace cgamd {

// ---- error plumbing ---------------------------------------------------------
void set_error(const std::string &msg);
int fail(int status, const std::string &msg);
#define CG_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return ::cgamd::fail(e__ == hipErrorNoDevice || e__ == hipErrorInvalidDevice     \
                                     ? CGAMD_ERR_NO_DEVICE : CGAMD_ERR_HIP,                  \
                                 std::string(#expr) + ": " + hipGetErrorString(e__));        \
    } while (0)

// hipMalloc (16 bytes at least) with the library's error text (precond_state.cpp)
int dmalloc(void **p, size_t bytes, const char *what);
inline size_t dtype_size(int dt) { return dt == 0 ? 4 : dt == 1 ? 8 : dt == 2 ? 8 : dt == 3 ? 16 : 0; }
inline size_t acc_size(int dt) { return (dt == 0 || dt == 1) ? 8 : 16; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Launch geometry of the persistent streaming kernels (kBlock, kSuperRows: spmv_plan.h).
constexpr int kMaxGrid = 2048;       // 256 CUs x 8 resident work-groups
constexpr int kQuadsPerThread = 2;   // SpMV: 2 x 4 non-zeros per thread per chunk -> 2048 nnz / chunk

// (LongRows, SpmvPlan, Tuning and the rules the SpMV form decision reads: spmv_plan.h)
SpmvPlan make_spmv_plan(int n);
// ---- CGAMD_SPLIT_LONG_ROWS (long_rows.hip) ----
constexpr int kLongRowSegment = 4 * kQuadsPerThread * kBlock;     // default segment: the stream kernel's chunk, 2048 entries
constexpr int kLongRowPiece = 64;             // a row's piece inside a segment of up to this many entries is summed by one lane, a longer one by a wave
constexpr size_t kLongRowMaxLds = 128 * 1024; // a segment's values and columns in LDS: the segment length is clamped to fit
// Marks the heavy row blocks (an 8-row slice spanning more than heavy_entries entries, measured 4-aligned as spmv_span_kernel does),
// builds the lists of `out` (count, scan, fill; no atomics) and the spans of the REGULAR blocks (spans[0..5]: 256 ... 8-row slices,
// spans[7]: longest row).  cycle: the row-block schedule's.  Synchronises `st`.  out->n_heavy == 0: no list was allocated
int build_long_rows(int n, const int *ptr_dev, int row_blocks, int heavy_entries, int seg_len, size_t value_bytes, int cycle, hipStream_t st,
                    LongRows *out, int spans[8]);
void free_long_rows(LongRows *lr);
// the heavy blocks of y = A x (and their d.q partials, partials[rb], when partials != nullptr): segment launch, then combine launch
int launch_long_rows(int dtype, const LongRows &lr, bool nt, int n, long long nnz, const void *vals, const int *ptr, const int *cols,
                     const void *x, void *y, const void *dvec, void *partials, hipStream_t st);
// fills plan->max_span / chunk_span from the matrix structure; synchronises `st`; scratch_dev: >= 32 bytes
int compute_spmv_plan(const int *ptr_dev, const int *cols_dev, int n, int *scratch_dev, hipStream_t st, SpmvPlan *plan);
// device-resident CSR (and an optional device index list with entries in [0, index_bound)): CGAMD_ERR_INVALID on a bad
// pointer array or an out-of-range column / index; synchronises `st`; scratch_dev: >= 4 bytes
int validate_csr_device(int n, long long nnz, int ncols, const int *ptr_dev, const int *cols_dev, const int *index_dev, int n_index,
                        int index_bound, int *scratch_dev, hipStream_t st);
// Column indices as one-byte codes into a dictionary of the matrix's distinct (column - row) offsets: 4 -> 1 byte per
// non-zero of index traffic for every matrix with at most 256 distinct offsets (stencils and FE matrices on structured grids:
// 5 to 27).  Exact: the kernel rebuilds the very same column, so results do not change by a bit.  On success *codes_out
// (nnz + 64 bytes) and *dict_out (256 ints) are device allocations the caller frees; both null when the matrix has more
// offsets than that.  Synchronises `st`.
int build_index_codes(int n, long long nnz, const int *ptr_dev, const int *cols_dev, hipStream_t st, unsigned char **codes_out,
                      int **dict_out, int *distinct_out);
// 16-bit columns relative to the first column of every 256-row block, for matrices with more offsets than the dictionary holds
// whose row blocks span fewer than 65 536 columns: *codes_out 2 nnz + 64 bytes, *base_out one int per row block; null when not codable
int build_joint_codes(int dtype, long long nnz, const unsigned char *codes, const unsigned char *vcodes, const int *dict, const void *vdict,
                      hipStream_t st, unsigned char **jcodes_out, int **joff_out, void **jval_out, int *n_pairs);
// one byte per ROW naming its pattern (index_codes.hip "ROW-PATTERN codes"), from the joint codes and the row pointers of a matrix whose
// longest row has at most 7 entries.  *rcodes_out: n + 64 bytes; *rdict_out: ONE allocation of row_dict_bytes, values [256][8] first,
// then the byte offsets [256][8] (row_dict_off_at), then the lengths [256] (row_dict_len_at); both null beyond 256 patterns
constexpr size_t row_dict_off_at(size_t value_size) { return 256 * 8 * value_size; }
constexpr size_t row_dict_len_at(size_t value_size) { return row_dict_off_at(value_size) + 256 * 8 * sizeof(int); }
constexpr size_t row_dict_bytes(size_t value_size) { return row_dict_len_at(value_size) + 256 * sizeof(int); }
// behind what the SpMV reads, for refresh_value_dicts only: the joint code of every pattern slot [256][8], one byte each; likewise the
// joint dictionary *joff_out holds 512 ints, [256 + c] = the value code of pair c
constexpr size_t row_dict_jmap_at(size_t value_size) { return row_dict_bytes(value_size); }
constexpr size_t row_dict_alloc_bytes(size_t value_size) { return row_dict_jmap_at(value_size) + 256 * 8; }
// n rows, the first n_user the caller's (the rest appended and empty): *n_patterns = dictionary entries, *n_user_patterns = patterns of
// the caller's rows
int build_row_codes(int dtype, int n, int n_user, const int *ptr_dev, const unsigned char *jcodes, const int *joff, const void *jval, hipStream_t st,
                    unsigned char **rcodes_out, void **rdict_out, int *n_patterns, int *n_user_patterns);
// ROW-PAIR patterns (index_codes.hip "ROW-PAIR codes", row_pairs.cpp): one byte per pair of rows (2p, 2p + 1) names the pair's union of
// slots, so that the SpMV serves both rows of a slot from ONE 16-byte load.  The dictionary is ONE allocation holding np entries:
// val0 [np][8] | val1 [np][8] | byte offsets [np][8] | masks [np] (bits 0..7: the slots row 2p uses, bits 8..15: row 2p + 1) -- what
// the kernel stages, pair_dict_stage_bytes -- then, for refresh_pair_dict only, the index into rdict_val every value came from
// (unsigned short [np][16]: row 2p's eight slots, then row 2p + 1's; 0xffff = slot not used by that row); pair_dict_*: spmv_plan.h
// the LDS the staged pair dictionary may take: with it eight work-groups of the pair kernel still fit a CU (160 KB), the occupancy
// the row form is measured at; a handle with more pair patterns than fit keeps the row form
constexpr size_t kPairDictLdsCap = 16 * 1024;
// *pcodes_out ((n + 1) / 2 + 64 bytes) and *pdict_out are device allocations the caller frees; both null (the handle keeps the row
// form) beyond 256 pair patterns, beyond kPairDictLdsCap, or where a pair's union needs more than 8 slots.  With odd n the last row
// pairs with an empty partner.  Synchronises `st`.
int build_row_pairs(int dtype, int n, const unsigned char *rcodes, const void *rdict, int n_patterns, hipStream_t st,
                    unsigned char **pcodes_out, void **pdict_out, int *n_pair_patterns, int *max_slots);
// after refresh_value_dicts kept the codes: the pair dictionary's values from the rewritten rdict, IN PLACE
int refresh_pair_dict(int dtype, int n_pair_patterns, const void *rdict, void *pdict, hipStream_t st);
int build_value_codes(int dtype, long long nnz, const void *vals_dev, hipStream_t st, unsigned char **vcodes_out, void **vdict_out, int *n_values);
// the values changed in place on the same pattern: one pass checks that every equal-value class of the codes is still one and, if so
// (*kept), rewrites vdict and -- where given -- jval (behind joff) and the values of rdict IN PLACE; else nothing is written and the
// caller rebuilds (index_codes.hip "REFRESH").  Synchronises `st`.
int refresh_value_dicts(int dtype, long long nnz, const void *vals_dev, const unsigned char *vcodes, void *vdict, int n_pairs, const int *joff,
                        void *jval, int n_patterns, void *rdict, hipStream_t st, bool *kept);
int build_index_codes16(int n, long long nnz, const int *ptr_dev, const int *cols_dev, hipStream_t st, unsigned char **codes_out, int **base_out);
void finalize_spmv_plan(SpmvPlan *plan, int dtype, int nrhs, int n, long long nnz, const void *vals, const int *cols);
constexpr int kChunkBytes = 32 * 1024;      // kind 7: preferred LDS chunk slice (4-5 work-groups per CU)
constexpr int kMaxChunkBytes = 48 * 1024;   //         largest accepted, with 8 lanes per row (3 work-groups per CU)
constexpr int kMaxSpmmSliceBytes = 64 * 1024;   // SpMM forms (nRHS > 1, row-major matrix-core op): largest 256-row LDS slice
constexpr int kMaxSliceBytes = 40 * 1024;   // variant 5: largest 256-row LDS slice (4 work-groups per CU); denser rows -> chunked kernel.
                                            // 27-point f32 (55 KB): 114 us one lane per row, 91 us chunked; 7-point c128 (36 KB): 314 vs 357

// (struct Tuning: spmv_plan.h)  g_tune is the process-wide configuration cgamd_tune edits (under a mutex).  Nothing on a compute path reads it
// directly: every solver / distributed handle copies it at creation (tune_snapshot()), and each C-ABI entry installs the
// handle's copy for the calling thread (TuneScope) -- launches of a handle always run with the configuration it was
// created under, whatever other threads set meanwhile (reference threading model: one thread per device, each with its own
// context and solver, p_h-PY_C-CL-multi-GPU.py:2149-2179).  tune() = the installed copy, or a per-thread snapshot of the
// global one for handle-less entries.
// whether a row- or pair-coded handle whose largest stride is unit_rows rows runs the plane-matched schedule under dev.spmv_plane =
// `knob`: 1 whenever it has a stride at all, a stride of one row included, and whatever the table looks like (below 8 super blocks per
// stride some XCDs sit out parts of a plane, below one the blocks are scattered, at exactly one super block EVERY block lands on one
// XCD and the grid is 8 x the super blocks: correct and slow, a development knob and what the tests run), 0 never, anything else the
// default rule, as measured (profiles/xcd_plane/): strides of at least 8 super blocks -- every XCD busy in every
// eighth of a plane: 3-D grids -- on matrices above 256 MB, the smallest size measured (the threshold of the pair form), for 4- and
// 8-byte values alike, AND only where the table built loads the XCDs evenly (xcd_schedule_balanced, checked by setup_xcd_schedule).
// The gain is 0.8 to 1.7 % of an iteration, not the third of the SpMV its saved traffic would be
constexpr size_t kPlaneMinMatrixBytes = (size_t)256 << 20;
inline bool spmv_plane_wanted(int knob, long long unit_rows, int rows_per_super, size_t matrix_bytes) {
    if (knob == 0 || unit_rows < 1) return false;
    if (knob == 1) return true;
    return unit_rows >= 8LL * rows_per_super && matrix_bytes > kPlaneMinMatrixBytes;
}
extern Tuning g_tune;
Tuning tune_snapshot();
const Tuning &tune();
} // namespace cgamd
#include <functional>
namespace cgamd {
void tune_set(const std::function<void(Tuning &)> &edit);
// the calling thread's next row-block SpMV launch records pair[0] / pair[1] on the dispatch itself (kernel duration)
void set_kernel_event_pair(hipEvent_t *pair);
void thread_hip_setup();      // once per thread: stream-capture interaction mode "relaxed" (see tune.cpp)
struct TuneScope {
    const Tuning *prev;
    explicit TuneScope(const Tuning *t);
    ~TuneScope();
};
int vec_grid(long long n_elems_per_rhs, int dtype, int nrhs = 1);

// ---- kernel launchers (all asynchronous on `st`) ------------------------------
// y = A x for nrhs vectors; x has leading dimension ldx (>= number of columns), y has ldy.
// If partials != nullptr also writes per-work-group partial sums of dvec.y (unconjugated),
// laid out partials[r * plan.grid + wg] in accumulator precision.
void last_spmv_form(int *out, int n_out);      // what this thread's last launch_spmv launched (spmv.hip: the SpmvForm it launched from)
void record_spmv_form(const int *fields);      // kSpmvFormFields ints of an SpMV launcher outside spmv.hip (batched.hip: family 6)
int launch_spmv(int dtype, const SpmvPlan &plan, int n, long long nnz, const void *vals, const int *ptr,
                const int *cols, const void *x, long long ldx, void *y, long long ldy, int nrhs,
                const void *dvec, void *partials, hipStream_t st, const int *rb_list = nullptr, int rb_count = 0);
// nsys systems on one pattern (batched.hip): y_r = A_r x_r with the values of system r at vals + r * nnz (vals: nsys * nnz entries, any
// alignment), x_r = x + r * ldx, y_r = y + r * ldy.  partials != nullptr: the d.q partials of 256-row blocks, partials[r * plan.n_partials
// + block] (plan.n_partials >= plan.row_blocks), the dot being dvec_r.y_r with dvec_r = dvec + r * ldx.  Uses the plan's row_blocks,
// max_span, max_row, n_partials and nt only
int launch_spmv_batched(int dtype, const SpmvPlan &plan, int n, long long nnz, int nsys, const void *vals, const int *ptr, const int *cols,
                        const void *x, long long ldx, void *y, long long ldy, const void *dvec, void *partials, hipStream_t st);
// flag[rb] = 1 when row block rb references a column >= n_local (needs the halo); kBlock rows per block
int launch_halo_flags(int n, const int *ptr, const int *cols, int n_local, int row_blocks, int *flag, hipStream_t st);
// partial sums of a.b -> partials[r*grid + wg]
int launch_dot_partials(int dtype, int n, const void *a, const void *b, long long ld, int nrhs, void *partials,
                        int grid, hipStream_t st);
// result[r] = sum partials (value type)
int launch_reduce_to_value(int dtype, const void *partials, int grid, int nrhs, void *result, hipStream_t st);
int launch_axpy(int dtype, int n, const void *x, void *y, long long ld, const void *a, int sign, int nrhs, hipStream_t st);
struct CgStop;
// (stop: the guarded form of the row-partitioned loops, cgamd_dist_iterate_until -- y is left alone once live[r] is cleared)
int launch_aypx(int dtype, int n, const void *x, void *y, long long ld, const void *a, int nrhs, hipStream_t st, const CgStop *stop = nullptr);
int launch_sub(int dtype, int n, const void *a, const void *b, void *res, long long ld, int nrhs, hipStream_t st);
// fused x += alpha d ; r -= alpha q ; partials(r.r)
int launch_axpy2_dot(int dtype, int n, const void *d, void *x, const void *q, void *r, long long ld,
                     const void *alpha, int nrhs, void *partials, int grid, hipStream_t st, int vec_nt = 3, const CgStop *stop = nullptr);

// device-resident scalar state of one CG run
struct CgScalars {
    void *alpha = nullptr;     // T[nrhs]
    void *beta = nullptr;      // T[nrhs]
    void *delta = nullptr;     // T[nrhs]   current delta_new
    void *history = nullptr;   // T[cap][nrhs]
    int *iter = nullptr;       // iterations completed
    int history_cap = 0;
    void *stage = nullptr;     // optional, two-level cg_alpha: acc[nrhs][32] part sums
    unsigned *ticket = nullptr;   //          and one zero-initialised ticket counter per RHS
    // order of the prologue sums over the d.q / r.r partials: 0 = thread-strided; K > 0 = member-blocked (reduce_device.h
    // thread_partials): handles the chip-wide resident loop can take over, K = 256-row (256-pack) blocks of one resident member
    int kdq = 0, krr = 0;
    // chip-wide resident loop only: the diagonal preconditioner and the rho parity buffer of a handle that runs the PCG recurrence
    const void *pcg_m = nullptr;
    void *pcg_rho2 = nullptr;
};
// Per-right-hand-side stop of cgamd_solver_iterate_until and cgamd_dist_iterate_until (stop_device.h): one device record per handle.  Launchers that take a
// `const CgStop *` run the guarded instantiation of their kernel when it is given and the unguarded one -- the code of
// cgamd_solver_iterate -- when it is NULL.
struct CgStop {
    int *nactive = nullptr;         // right-hand sides still iterating: the word the host reads back after every chunk
    const double *tol = nullptr;    // double[nrhs], in device memory so that captured launches serve every call
    int *stop = nullptr;            // int[nrhs]: the iteration right-hand side r stopped in, 0 = still iterating.  Written by the
                                    // beta launch only and read as an exit condition by every OTHER launch
    int *live = nullptr;            // int[nrhs]: 0 once the alpha step of a later iteration has seen stop[r]: the exit condition of
                                    // the beta launch, which must not read the word it writes
};
// Host side of the stop (stop_run.cpp), one per handle: the record, the pinned words the host reads while the device runs on, and
// the driver of a call.  A call is alloc, arm, chunks, read, then the owner's stream synchronise; the owner clears `armed` in set_rhs.
// (Hidden: the libraries export what they exported before these functions were shared.)
#pragma GCC visibility push(hidden)
struct StopRun {
    void *rec = nullptr;            // the device record: [nactive, pad x3] [tol: nr doubles] [stop: nr ints] [live: nr ints]
    CgStop view;                    // pointers into it: what the guarded launchers take
    int nr = 0;
    int *pin = nullptr;             // pinned: [0..1] the active counts of the chunks in flight, [2] free for a word the owner reads
                                    // back with stop[], then `stopped` and the image the record is armed from
    int *stopped = nullptr;         // int[nr] in the pinned block: stop[] as the last call read it, 0 again once armed anew
    hipEvent_t ev[2] = {nullptr, nullptr};      // behind the two active counts
    bool armed = false;
    int enqueued = 0;               // what the last stop_run_chunks left: iterations it put into the stream (also when it failed),
    bool active = true;             // and false once it has seen an active count of 0
};
// the record for nr right-hand sides, the pinned block and the events, whatever of them the handle does not have yet
int stop_run_alloc(StopRun &sr, int nr);
// arms the record once per set_rhs (everything active, nothing stopped); later calls only bring their tolerances.  nTol: 1 or nr
int stop_run_arm(StopRun &sr, const double *tol, int nTol, hipStream_t st);
// Chunks of `chunk` iterations, at most maxIterations in all: enqueue(len) puts len guarded iterations into the stream; after each
// chunk the active count is read back asynchronously, and the host waits for the count of chunk c - 1 only once chunk c is in the
// stream, so the device never idles on the host.  Leaves sr.enqueued and sr.active
int stop_run_chunks(StopRun &sr, int maxIterations, int chunk, hipStream_t st, const std::function<int(int)> &enqueue);
// stop[] into sr.stopped, asynchronously: valid after the owner's stream synchronise
int stop_run_read(StopRun &sr, hipStream_t st);
void stop_run_free(StopRun &sr);
#pragma GCC visibility pop
// ten-vector-pass iteration (x update deferred into the aypx launch): see vector.hip
int launch_axpy_dot(int dtype, int n, const void *q, void *r, long long ld, const void *alpha, int nrhs, void *partials, int grid,
                    hipStream_t st, int vec_nt = 3, const CgStop *stop = nullptr);
int launch_axpy_dot_alpha(int dtype, int n, const void *q, void *r, long long ld, const void *part_dq, int P, const CgScalars &sc,
                          int nrhs, void *partials, int grid, hipStream_t st, const CgStop *stop = nullptr);
int launch_aypx_beta_x(int dtype, int n, const void *x, void *y, void *xs, long long ld, const void *partials, int P, int nrhs,
                       const CgScalars &sc, hipStream_t st, int vec_nt = 3, const CgStop *stop = nullptr);
// x brought up to date once per group of `lag` iterations (vector.hip): the d step of every group iteration but the last,
// d_out = beta d_in + r with d_in kept, and the group's last step, x += alpha_0 dirs[0] + ... + alpha_{lag-1} dirs[lag-1] in
// iteration order, dirs[0] = beta dirs[lag-1] + r.  lag 2, 4 or 8.  sc.alpha is the ring of kLagMax * nrhs values; group
// iteration j keeps its alpha in slot lag_alpha_slot(j, lag), so that a group's last iteration leaves it where every other
// loop does (slot 0)
constexpr int kLagMax = 8;
constexpr int lag_alpha_slot(int j, int lag) { return (j + 1) % lag; }
int launch_aypx_beta_out(int dtype, int n, const void *r, const void *d_in, void *d_out, long long ld, const void *partials, int P,
                         int nrhs, const CgScalars &sc, hipStream_t st, int vec_nt = 3);
int launch_aypx_beta_xlag(int dtype, int n, int lag, const void *r, void *const *dirs, void *xs, long long ld, const void *partials, int P,
                          int nrhs, const CgScalars &sc, hipStream_t st, int vec_nt = 3);
// small systems: alpha = delta / sum(part_dq) in the prologue (three-launch iteration); fold_alpha_ok says when
bool fold_alpha_ok(int n_partials, int fold_max = 0);      // fold_max 0 = the default limit (2048 partials)
// two-launch iteration (spmv.hip "Two-launch iteration"): the SpMV launch computes beta and d_new = beta d_old + r on the
// fly; d_old / d_new are different buffers.  fused2_ok: the plan's row-block kernels apply and the system is small enough
bool fused2_ok(const SpmvPlan &plan, int dtype, int nrhs, const void *vals, const int *cols);
int launch_spmv_fused(int dtype, const SpmvPlan &plan, int n, long long nnz, const void *vals, const int *ptr, const int *cols,
                      const void *d_old, void *d_new, const void *r, void *q, int nrhs, void *part_dq, const void *part_rr, int P,
                      const CgScalars &sc, hipStream_t st);
// delta / beta / history[iter] of the last iteration of an iterate() call of that loop
int launch_cg_tail(int dtype, const void *part_rr, int P, int nrhs, const CgScalars &sc, hipStream_t st);
int launch_axpy2_dot_alpha(int dtype, int n, const void *d, void *x, const void *q, void *r, long long ld, const void *part_dq,
                           int P, const CgScalars &sc, int nrhs, void *partials, int grid, hipStream_t st);
// delta[r] = sum partials ; history[0][r] = delta[r] ; *iter = 0
int launch_cg_delta0(int dtype, const void *partials, int grid, int nrhs, const CgScalars &s, hipStream_t st);
// alpha[r] = delta[r] / sum partials_dq
int launch_cg_alpha(int dtype, const void *partials, int grid, int nrhs, const CgScalars &s, hipStream_t st, const CgStop *stop = nullptr);
// dn = sum partials_rr ; beta = dn/delta ; delta = dn ; history[++iter] = dn
int launch_cg_beta(int dtype, const void *partials, int grid, int nrhs, const CgScalars &s, hipStream_t st, const CgStop *stop = nullptr);

// d = beta d + r with beta = (sum of the P r.r partials) / history[iter-1] computed in every work-group's prologue;
// work-group 0 records delta, beta and history[iter] (the cg_beta launch folded into aypx)
int launch_aypx_beta(int dtype, int n, const void *x, void *y, long long ld, const void *partials, int P, int nrhs,
                     const CgScalars &sc, hipStream_t st);

// partials -> accumulator-precision scalar per RHS (all-reduce input); halo pack out[k] = v[index[k]]
int launch_reduce_to_acc(int dtype, const void *partials, int grid, int nrhs, void *out, hipStream_t st);
int launch_pack(int dtype, int count, const int *index, const void *v, void *out, hipStream_t st);

// ---- row-major multi-RHS path (rowmajor.hip): the RHS block is X[n][nrhs], element (i, r) at i*nrhs + r ----------------
// Y = A X on the matrix cores (+ per-RHS d.q partials [nrhs][spmm_rm_grid(n)] in accumulator precision when partials != 0,
// the dot being x.y); f64 with 16 / 32 right-hand sides, f32 with 16 / 32 / 64, complex64 with 16 / 32; any CSR matrix
bool spmm_rm_supported(int dtype, int nrhs, int n);
// work-groups (= fused-dot partials per RHS) the launch will use for this problem
int spmm_rm_grid(int dtype, int nrhs, int n, int max_quad, bool dot);
// max_quad: most non-zeros in 4 consecutive rows (SpmvPlan::max_quad; 0 = unknown), picks the fp64 kernel's K-steps per quad
// pace: kSpmmPaceInts zeroed ints owned by the caller and used by ONE stream at a time, always for the same problem (the sweep's
// per-wave progress words, cumulative over launches; one set for the launches with partials, one for those without), or null =
// unpaced sweep
int launch_spmm_rm(int dtype, int n, long long nnz, const void *vals, const int *ptr, const int *cols, const void *x, void *y,
                   int nrhs, void *partials, int max_quad, int *pace, hipStream_t st);
constexpr int kSpmmPaceInts = 2 * 8 * 256 / 4;
// what launch_spmm_rm will launch for this problem, from the functions it launches through: out = real columns, values per lane (NH),
// K-steps per quad and round (TQ), strips, work-groups, XCDs whose sweep paces itself (have_pace: the caller passes progress words)
int spmm_rm_plan(int dtype, int nrhs, int n, int max_quad, bool dot, bool have_pace, int out[6], int *lead);
// the streaming form of rm_axpy_dot (mask 2) / rm_aypx_x (mask 1) on a block of `total` values
bool rm_vec_nt(int mask, long long total, int dtype);
// vector kernels with per-column scalars; partials[r * grid + wg]
int rm_vec_grid(long long total_elems, int dtype);
int launch_rm_dot(int dtype, int n, int nrhs, const void *a, const void *b, void *partials, int grid, hipStream_t st);
int launch_rm_axpy_dot(int dtype, int n, int nrhs, const void *q, void *r, const void *alpha, void *partials, int grid, hipStream_t st);
int launch_rm_aypx_x(int dtype, int n, int nrhs, const void *r, void *d, void *x, const void *alpha, const void *beta, int grid,
                     hipStream_t st);
// ---- resident loop (resident.hip): every iteration of an iterate() call of a small system inside ONE launch ---------------
struct ResidentPlan {
    int G = 0;          // work-groups (of 1024 rows) per right-hand side
    int cap = 0;        // LDS entries of the largest 1024-row matrix slice
    int wcap = 0;       // LDS entries for the per-iteration window of beta d + r (0 = every non-zero gathers from L2)
    int unroll = 8;     // gathers in flight per row walk round
    int local = 1;      // a group lives on one XCD (plain stores, sc1 loads); 0: write-through stores (groups wider than an XCD)
    int lg = 0;         // groups per ticket counter (per XCD when local)
    int slots = 0;      // group slots the sync words cover
    size_t lds_bytes = 0, sync_bytes = 0;
};
// false = the loop does not apply (size, alignment, LDS, partial-sum structure of the two-launch loop); ptr_host: n + 1 row pointers
// max_window: resident_max_window()'s answer (0 = unknown: no LDS window)
bool resident_plan(int dtype, int n, int vgrid, int row_blocks, int n_cus, const int *ptr_host, int max_window, ResidentPlan *out);
int resident_max_window(int dtype, int n, const int *ptr_dev, const int *cols_dev, int *scratch_dev, hipStream_t st, int *out);
// K iterations (number it0 + 1 ... it0 + K) of every right-hand side; state in and out is the two-launch loop's (x, r, d of
// iteration k in (k & 1 ? d1 : d0), r.r partials, delta / beta / alpha / history / iter), bit for bit.  Synchronises `st`;
// sync: rp.sync_bytes of device memory.
int run_cg_resident(int dtype, const ResidentPlan &rp, int n, int nrhs, const void *vals, const int *ptr, const int *cols, void *x, void *r,
                    void *d0, void *d1, void *part_rr, int P_rr, int row_blocks, const CgScalars &sc, int it0, int K, void *sync,
                    int n_cus, hipStream_t st, bool *untouched = nullptr, double tol = 0., int *stopped_at = nullptr);

// serialises resident launches per GPU (resident.hip); held() == false: not obtained within wait_ms -- fall back, touch nothing
struct ResidentLock {
    ResidentLock(int device, int wait_ms);
    ~ResidentLock();
    ResidentLock(const ResidentLock &) = delete;
    ResidentLock &operator=(const ResidentLock &) = delete;
    bool held() const { return held_; }
private:
    void *mutex_ = nullptr;
    int fd_ = -1;
    bool held_ = false;
};

// wide resident loop (resident.hip): chip-wide groups (one right-hand side each at a time), matrix rows in registers
constexpr int kResWideBlocksPerRpt = 2;     // 256-row blocks of a chip-wide resident member per row of a thread (512 threads: resident_device.h)
struct ResidentWidePlan {
    bool ok = false;
    int rpt = 0, unroll = 0, G = 0, NG = 1, wcap = 0;      // NG concurrent groups of G work-groups
    size_t lds_bytes = 0, sync_bytes = 0;
};
int resident_wide_plan(int dtype, int n, long long nnz, int nrhs, int n_cus, const int *ptr_dev, const int *cols_dev, int *scratch_dev,
                       hipStream_t st, ResidentWidePlan *out, bool small_ok = false);
// state in and out: x, r, d of iteration k in (k & 1 ? d1 : d0), delta / beta / alpha / history / iter; d_ready: on entry d is
// already beta d + r (three / four-launch loops); on exit d is always the direction of the last iteration (two-launch
// convention) and the launched loops' r.r partials are NOT maintained -- the caller converts / rebuilds
int run_cg_resident_wide(int dtype, const ResidentWidePlan &wp, int n, int nrhs, const void *vals, const int *ptr, const int *cols, void *x,
                         void *r, void *d0, void *d1, bool d_ready, const CgScalars &sc, int it0, int K, void *sync, int n_cus, hipStream_t st,
                         bool *untouched = nullptr, double tol = 0., int *stopped_at = nullptr);

// slab loop (slab.hip): every iteration of a call in one launch, vectors in registers, matrix streamed; systems of up to ~3M rows
struct SlabPlan {
    bool ok = false;
    int rows_m = 0, G = 0, nsteps = 0, cap = 0, ccap = 0, unroll = 8;      // rows_m / nsteps: of the largest member
    size_t lds_bytes = 0, sync_bytes = 0;
    const int *mstart = nullptr, *gmember = nullptr;      // device arrays of a non-uniform partition (slab_partition), owned by the caller
    const unsigned char *vcodes = nullptr;                // one-byte value codes of the matrix and their dictionary (build_value_codes), owned by
    const void *vdict = nullptr;                          // the caller; null = the members stream the values
};
bool slab_plan(int dtype, int n, int n_cus, const SpmvPlan &plan, bool coded, SlabPlan *out);
int slab_partition(const SlabPlan &sp, int n, const std::vector<char> &boundary, int trim, int max_members, std::vector<int> *mstart,
                   std::vector<int> *gmember);
size_t slab_sync_bytes(int G);
// row-partitioned run of the slab loop: the peer-to-peer mailboxes of the handle (device arrays as in P2pExchange) and, per peer and
// buffer parity, where this rank's boundary entries land in the PEER's published-d buffer
struct SlabComm {
    int n_halo = 0, nranks = 1, rank = 0, n_peers = 0;
    char *const *mailbox = nullptr;
    const int *peer_rank = nullptr, *send_off = nullptr, *send_count = nullptr, *recv_count = nullptr, *send_index = nullptr;
    void *const *push_dst = nullptr;                // device [2][n_peers]
    unsigned long long *halo_epoch = nullptr, *red_seq = nullptr;
};
// state in and out: x, r, din = d (already beta d + r), delta / beta / alpha / history / iter of the three / four-launch loops; ds0 / ds1:
// n + n_halo values each, where the iterations publish d; codes / dict: the one-byte column codes of the matrix (required)
int run_cg_slab(int dtype, const SlabPlan &sp, int n, long long nnz, const void *vals, const int *ptr, const unsigned char *codes,
                const int *dict, void *x, void *r, void *din, void *ds0, void *ds1, const SlabComm *cm, const CgScalars &sc, int it0, int K,
                void *sync, hipStream_t st, bool *untouched = nullptr);

// [rows][cols] -> [cols][rows]: RHS-major (the reference ABI) <-> row-major
int launch_transpose(int dtype, int rows, int cols, const void *in, void *out, hipStream_t st);

// ---- peer-to-peer backend (p2p.hip "Peer-to-peer communication over xGMI") ----------------------------
constexpr size_t kMailboxHeader = 16384;  // slots + flags + error word + single-reduction slots; halo entries follow
struct P2pExchange {
    char *const *mailbox = nullptr;   // device array [nranks] of mapped mailbox bases
    int rank = 0, n_peers = 0, n_local = 0;
    const int *peer_rank = nullptr, *send_off = nullptr, *send_count = nullptr, *dst_off = nullptr, *recv_off = nullptr,
              *recv_count = nullptr;  // device arrays [n_peers]
    const int *send_index = nullptr;
    unsigned long long *epoch = nullptr;
    unsigned *counters = nullptr;     // device, zero-initialised: [0] unpack, [1 + p] push of peer p
    int max_count = 0;                // largest send/recv count over the peers
    const void *my_halo = nullptr;    // halo area of MY mailbox (entry h = column n_local + h)
};
int p2p_push_chunks(const P2pExchange &e);
// diagonally preconditioned CG (helmFE_var.py:546-586 with a diagonal M): see vector.hip.  m_pitch: values between the diagonals of
// consecutive right-hand sides (a batched handle: m_r belongs to system r), 0 = one m shared by all
int launch_pcg_axpy2_dot2(int dtype, bool init, int n, const void *d, void *x, const void *q, void *r, const void *m,
                          long long ld, const void *alpha, int nrhs, void *part_rz, void *part_rr, int grid, hipStream_t st,
                          long long m_pitch = 0, const CgStop *stop = nullptr);
int launch_pcg_aypx_beta(int dtype, int n, const void *r, void *p, const void *m, long long ld, const void *part_rz,
                         const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2, void *xs, hipStream_t st,
                         long long m_pitch = 0, const CgStop *stop = nullptr);
int launch_pcg_p_update(int dtype, int n, const void *r, void *p, const void *m, long long ld, const void *beta, int nrhs, hipStream_t st);
int launch_pcg_delta0(int dtype, const void *part_rz, const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2, hipStream_t st);
// ---- CGAMD_HERMITIAN handles (hermitian.hip): CG with <a, b> = sum conj(a_i) b_i, complex value types only.  dc = conj(d) is kept
// beside d, so that the fused dot of every SpMV kernel yields d^H q; alpha, beta, delta and rho are real (imaginary part +0).
// m == nullptr: no preconditioner; else z = m .* r with m at pitch m_pitch per right-hand side (0 = shared), rho = Re(r^H z) kept
// in sc.delta and in the parity buffer rho2, part_rz its partials.  history holds r^H r in both cases.
// set_rhs: d = r (d = m .* r), dc = conj(d), partials of r^H r (and r^H z); then delta0 / rho0, history[0], iter = 0
int launch_herm_init(int dtype, int n, const void *r, void *d, void *dc, const void *m, long long m_pitch, long long ld, int nrhs,
                     void *part_rz, void *part_rr, int grid, hipStream_t st);
int launch_herm_delta0(int dtype, bool pre, const void *part_rz, const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2,
                       hipStream_t st);
// alpha = delta / Re(sum of the d^H q partials); advances the counter (guarded: the alpha-step duties of stop_device.h)
int launch_herm_alpha(int dtype, const void *part_dq, int P, int nrhs, const CgScalars &sc, hipStream_t st, const CgStop *stop = nullptr);
// r -= alpha q ; partials of r^H r (and of r^H (m .* r))
int launch_herm_axpy_dot(int dtype, int n, const void *q, void *r, const void *m, long long m_pitch, long long ld, const void *alpha,
                         int nrhs, void *part_rz, void *part_rr, int grid, hipStream_t st, const CgStop *stop = nullptr);
// beta, delta, history[iter] and the stop decision in the prologue; x += alpha d ; d = beta d + r (d = beta d + m .* r) ; dc = conj(d)
int launch_herm_aypx_beta_x(int dtype, int n, const void *r, void *d, void *dc, void *xs, const void *m, long long m_pitch, long long ld,
                            const void *part_rz, const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2, hipStream_t st,
                            const CgStop *stop = nullptr);
// tridiagonal M (precond.hip): the factors of cgamd_solver_set_preconditioner_tridiag and the chunk plan, device arrays
struct TriLaunch {
    const void *nl = nullptr, *ne = nullptr, *w = nullptr;   // -l_i, -w_i c_i, w_i = 1/u_i: n values each
    long long fpitch = 0;                                    // a batched handle: right-hand side r reads the factors of system r at r * fpitch
                                                             // values into each array; 0 = one M shared by all right-hand sides
    const int *cstart = nullptr;                             // nchunks + 1 chunk boundaries (rows)
    int nchunks = 0, grid = 0;                               // grid = work-groups = r.z / r.r partials per RHS
    bool longform = false;                                   // a segment is longer than a chunk: maps, carry, apply (3 launches)
    void *maps = nullptr;                                    // longform: tri_maps_values(nchunks, nrhs) values
    // strided form (precond_strided.hip, stride > 1): M couples rows i and i +- stride; the plan is the segment list, not chunks
    int stride = 1;
    const int *segs = nullptr;                               // nsegs pairs (first row, length), ordered by first row
    int nsegs = 0;
};
int tri_chunk_rows(int dtype);              // C: rows a chunk may span, from the first pack-aligned row of its work-group
int tri_maps_values(int nchunks, int nrhs);
// r -= alpha q (update; r.r partials) ; z = M^-1 r (r.z partials).  z may be q (in place).  update = false: set_rhs (z0 of r0)
int launch_pcg_tri(int dtype, const TriLaunch &t, bool update, const void *q, void *r, void *z, long long ld, const void *alpha, int nrhs,
                   void *part_rz, void *part_rr, hipStream_t st, const CgStop *stop = nullptr);
// the same for the strided form: one thread per segment, a single launch for segments of any length
int tri_strided_grid(int nsegs);            // work-groups = r.z / r.r partials per RHS (at most 1024)
int launch_pcg_tri_strided(int dtype, const TriLaunch &t, bool update, const void *q, void *r, void *z, long long ld, const void *alpha,
                           int nrhs, void *part_rz, void *part_rr, hipStream_t st, const CgStop *stop = nullptr);
// preconditioners built from the matrix on the device (precond_build.hip); n_user = the caller's rows, n = with the padding rows.
// lower / diag / upper <- the CSR entries at column - row = -stride / 0 / +stride, entries at the same column summed (n_user values)
// (only columns below col_limit count: the halo columns of a row-partitioned matrix are numbered from n_local on and are no line
// neighbours, whatever their distance from the row)
int launch_line_extract(int dtype, int n_user, int stride, const void *vals, const int *ptr, const int *cols, int col_limit, void *lower,
                        void *diag, void *upper, hipStream_t st);
// m[i] = 1 / A[i][i]; *err (preset to all ones) <- the smallest row with a zero, missing or non-finite diagonal
int launch_jacobi_extract(int dtype, int n_user, const void *vals, const int *ptr, const int *cols, void *m, unsigned long long *err,
                          hipStream_t st);
// flags[i] = i < stride or x[i] and y[i - stride] are both exactly zero (x, y: n values)
int launch_line_flags(int dtype, int n, int stride, const void *x, const void *y, unsigned char *flags, hipStream_t st);
// *longest (preset to 0) <- rows of the longest run first, first + stride, ... between flags; a walk gives up at cap rows (the word
// then holds a value in [cap, cap + 8))
int launch_line_longest(int n, int stride, const unsigned char *flags, int cap, int *longest, hipStream_t st);
// Thomas factors -l, -w c, w of every pre-segment, one thread each; *err (preset to all ones) <- (row << 2) | kind of the smallest
// failing row: kind 0 non-finite entry, 1 zero or non-finite pivot, 2 pivot too small
int launch_line_factor(int dtype, int n_user, int stride, const unsigned char *pre, const void *lower, const void *diag,
                       const void *upper, void *nl, void *ne, void *w, unsigned long long *err, hipStream_t st);
// the same passes over nsys matrices on one pattern (the values of system r at vals + r * nnz; every per-row array of system r at
// r * pitch values): one launch each whatever nsys.  The flags are AND-ed over the systems; the error words name the smallest
// system, then the smallest row in it: Jacobi (system << 32) | row, factor (system << kBatchedErrSystemShift) | (row << 2) | kind
constexpr int kBatchedErrSystemShift = 34;
int launch_batched_line_extract(int dtype, int n_user, int stride, int nsys, long long nnz, const void *vals, const int *ptr, const int *cols,
                                void *lower, void *diag, void *upper, long long pitch, hipStream_t st);
int launch_batched_jacobi_extract(int dtype, int n_user, int nsys, long long nnz, const void *vals, const int *ptr, const int *cols, void *m,
                                  long long pitch, unsigned long long *err, hipStream_t st);
int launch_batched_line_flags(int dtype, int n, int stride, int nsys, const void *x, const void *y, long long pitch, unsigned char *flags,
                              hipStream_t st);
int launch_batched_line_factor(int dtype, int n_user, int stride, int nsys, const unsigned char *pre, const void *lower, const void *diag,
                               const void *upper, void *nl, void *ne, void *w, long long pitch, unsigned long long *err, hipStream_t st);
// count: line_count_ints(n) ints <- the flagged rows before every 256-row block, the total in its last entry
int line_count_ints(int n);
int launch_line_count(int n, const unsigned char *flags, int *count, hipStream_t st);
// the flagged rows in order: out[k] = row, or with pairs out[2 k] = row, out[2 k + 1] = rows up to the chain's next flag
int launch_line_emit(int n, int stride, bool pairs, const unsigned char *flags, const int *block_off, int *out, hipStream_t st);
// ---- preconditioner setup shared by the single-GPU and the row-partitioned handle (precond_setup.cpp) ----
// a factored tridiagonal M on the device: coef = 3 x pitch values (-l, -w c, w); plan = count + 1 chunk boundaries (stride 1) or
// count (first row, length) pairs (stride > 1).  Both allocations belong to the caller.  nsys > 0 (tri_build_from_matrix_batched): one
// M per system on ONE plan, coef = 3 arrays of nsys x pitch values.
struct TriBuilt {
    void *coef = nullptr;
    size_t pitch = 0;
    int *plan = nullptr;
    int stride = 1, count = 0;
    bool longform = false;
    int source = 0;         // 2 = factored on the device, 3 = extracted on the device and factored by the host route
    int nsys = 0;
};
void tri_built_free(TriBuilt *b);
// from M's three arrays (nu values each, host or device), factored and planned on the host; n >= nu: rows with the padding
int tri_build_host(hipStream_t st, int dt, int nu, int n, const std::string &who, int stride, const void *lower, const void *diag,
                   const void *upper, int on_device, TriBuilt *out);
// from the CSR entries at column - row in {-stride, 0, +stride} with column < col_limit, on the device; route: Tuning::dev_line_host_route
int tri_build_from_matrix(hipStream_t st, int dt, int nu, int n, int route, const std::string &who, int stride, const void *vals,
                          const int *ptr, const int *cols, int col_limit, TriBuilt *out);
// the lines of nsys matrices on one pattern, every system factored on the device, ONE segment plan (a row starts a segment when it
// does in every system); errors name the system and the row.  A constant number of launches and synchronisations whatever nsys
int tri_build_from_matrix_batched(hipStream_t st, int dt, int nu, int n, int nsys, long long nnz, const std::string &who, int stride,
                                  const void *vals, const int *ptr, const int *cols, TriBuilt *out);
// m_r[i] = 1 / A_r[i][i] at m + r * pitch (m: nsys * pitch device values of the caller); level >= 0: the matrices are a level of a
// multigrid hierarchy and the error names "system R level L row I"
int jacobi_build_from_matrix_batched(hipStream_t st, int dt, int nu, int nsys, long long nnz, const std::string &who, const void *vals,
                                     const int *ptr, const int *cols, void *m, long long pitch, int level = -1);
// m[i] = 1 / A[i][i] (m: nu device values of the caller); CGAMD_ERR_INVALID names the smallest bad row
int jacobi_build_from_matrix(hipStream_t st, int dt, int nu, const std::string &who, const void *vals, const int *ptr, const int *cols,
                             void *m);
// ---- aggregation multigrid preconditioner on grid systems (multigrid.hip, multigrid_setup.cpp) ----
// a grid numbered x fastest and the grid of its 2 x 2 x 2 aggregates: fine node (x, y, z) -> coarse node (x >> 1, y >> 1, z >> 1)
struct MgGrid { int nx = 1, ny = 1, nz = 1, cnx = 1, cny = 1, cnz = 1; };
constexpr int kMgMaxRow = 64;       // most distinct columns of a coarse row
constexpr int kMgMaxLevels = 16;
// count[I] <- distinct coarse columns of coarse row I (nc rows); *err (preset to all ones) <- the smallest row with more than kMgMaxRow
int launch_mg_count(const MgGrid &g, int nc, const int *ptr, const int *cols, int *count, unsigned long long *err, hipStream_t st);
// n counts -> n + 1 row pointers in place (one work-group); *overflow (preset to 0) <- 1 when the total does not fit an int
int launch_mg_scan(int n, int *counts_to_ptr, int *overflow, hipStream_t st);
// the coarse columns (ascending) and values: fine rows ascending, entries in stored order, summed in the accumulator type, rounded once
int launch_mg_fill(int dtype, const MgGrid &g, int nc, const void *vals, const int *ptr, const int *cols, const int *ptrc, int *colsc,
                   void *valsc, hipStream_t st);
// *out (preset to 0) <- the bits of max_i |dinv_i| sum_j |a_ij| (double)
int launch_mg_gershgorin(int dtype, int n, const void *vals, const int *ptr, const void *dinv, unsigned long long *out, hipStream_t st);
// one Chebyshev step on n rows of nrhs vectors at stride ld (mode 0: from x = 0, 1: first step from x != 0, 2: a later step; w = A x)
int launch_mg_cheb(int dtype, int mode, int n, long long ld, int nrhs, const void *dinv, const void *b, const void *w, void *d, void *x,
                   double c0, double c1, bool store_d, hipStream_t st);
// bc = P^T (b - w), then the coarse level's first smoothing step from zero: xc = (dc =) c1 dinvc bc
int launch_mg_restrict(int dtype, const MgGrid &g, int nc, long long ldf, long long ldc, int nrhs, const void *b, const void *w, void *bc,
                       const void *dinvc, void *xc, void *dc, double c1, bool store_d, hipStream_t st);
// x += omega P e on the nf rows of the fine grid
int launch_mg_prolong(int dtype, const MgGrid &g, int nf, long long ldf, long long ldc, int nrhs, const void *e, void *x, double omega,
                      hipStream_t st);
// ---- the per-system forms for nsys systems on one pattern (multigrid_batched.hip): values of system r at vals + r * nnz, dinv at
// dinv + r * ld, the Chebyshev coefficients of a step as device arrays of nsys values of the real type.  The prolongation is shared
// the coarse columns once and every system's values (fine at vals + r * nnzf, coarse at valsc + r * nnzc), by the rules of launch_mg_fill
int launch_mg_fill_batched(int dtype, const MgGrid &g, int nc, int nsys, long long nnzf, long long nnzc, const void *vals, const int *ptr,
                           const int *cols, const int *ptrc, int *colsc, void *valsc, hipStream_t st);
// out[r] (nsys words preset to 0) <- the bits of max_i |dinv_r[i]| sum_j |a_r[i][j]| (double)
int launch_mg_gershgorin_batched(int dtype, int n, int nsys, long long nnz, long long pitch, const void *vals, const int *ptr,
                                 const void *dinv, unsigned long long *out, hipStream_t st);
int launch_mg_cheb_batched(int dtype, int mode, int n, long long ld, int nsys, const void *dinv, const void *b, const void *w, void *d,
                           void *x, const void *c0, const void *c1, bool store_d, hipStream_t st);
int launch_mg_restrict_batched(int dtype, const MgGrid &g, int nc, long long ldf, long long ldc, int nsys, const void *b, const void *w,
                               void *bc, const void *dinvc, void *xc, void *dc, const void *c1, bool store_d, hipStream_t st);
// The hierarchy of one handle.  Level 0 borrows the handle's matrix and the plan of its SpMV (codes included: build again whenever
// they change); the coarse levels own theirs.  nu = the caller's rows, n = with the padding rows (z = 0 there)
// ---- algebraic aggregates (amg.hip): handshake matching from the matrix, then the same Galerkin sums and V-cycle through stored maps
constexpr int kAmgWidth = 8;        // most members of an aggregate (2^passes); the stride of the member lists
constexpr int kAmgMaxRounds = 32;   // matching rounds of a pass
// smax[i] <- the largest s_ij = -Re(a_ij) > 0 over the stored entries j != i of row i, 0 without one
int launch_amg_smax(int dtype, int n, const void *vals, const int *ptr, const int *cols, double *smax, hipStream_t st);
// pick[i] <- the best strong unmatched neighbour of every unmatched row (-1: none), from the matching as it stands
int launch_amg_pick(int dtype, int n, double theta, const void *vals, const int *ptr, const int *cols, const double *smax, const int *match,
                    int *pick, hipStream_t st);
// match[i] <- j where pick[i] == j and pick[j] == i; *formed (preset to 0) <- 1 when there was such a pair
int launch_amg_handshake(int n, const int *pick, int *match, int *formed, hipStream_t st);
// flag[i] <- 1 for the smallest member of every aggregate
int launch_amg_roots(int n, const int *match, int *flag, hipStream_t st);
// rank = the flags scanned: pmap[i] <- the coarse id of row i; pairs[2 I], pairs[2 I + 1] <- root and partner (-1) of aggregate I
int launch_amg_number(int n, const int *match, const int *rank, int *pmap, int *pairs, hipStream_t st);
// agg_out[i] <- pmap[agg_in[i]] (agg_in == nullptr: pmap[i]); in place serves
int launch_amg_compose(int n, const int *pmap, const int *agg_in, int *agg_out, hipStream_t st);
// out <- the member lists (kAmgWidth per aggregate, ascending, -1 behind the last) of the pairs' members' lists merged (old == nullptr:
// the members themselves)
int launch_amg_members(int nc, const int *pairs, const int *old, int *out, hipStream_t st);
// launch_mg_count / launch_mg_fill with the rows of coarse row I from mem[I * width ...] (-1 ends the list) and the coarse column agg[col]
int launch_amg_count(int nc, int width, const int *mem, const int *agg, const int *ptr, const int *cols, int *count, unsigned long long *err,
                     hipStream_t st);
int launch_amg_fill(int dtype, int nc, int width, const int *mem, const int *agg, const void *vals, const int *ptr, const int *cols,
                    const int *ptrc, int *colsc, void *valsc, hipStream_t st);
// launch_mg_restrict / launch_mg_prolong through the member lists (kAmgWidth per coarse row) / the map
int launch_amg_restrict(int dtype, int nc, const int *mem, long long ldf, long long ldc, int nrhs, const void *b, const void *w, void *bc,
                        const void *dinvc, void *xc, void *dc, double c1, bool store_d, hipStream_t st);
int launch_amg_prolong(int dtype, int nf, const int *agg, long long ldf, long long ldc, int nrhs, const void *e, void *x, double omega,
                       hipStream_t st);
struct MgHierarchy;
// (struct MgParams and the range checks of the entries that fill it: mg_params.h)
// nsys > 0 (a batched handle, nrhs == nsys): one hierarchy per system on shared aggregates and patterns, vals = nsys * nnz values
int mg_build(hipStream_t st, int dt, int nu, int n, int nrhs, int nsys, const SpmvPlan &plan0, long long nnz, const void *vals,
             const int *ptr, const int *cols, const MgParams &p, const std::string &who, MgHierarchy **out);
void mg_free(MgHierarchy *h);
// z = M^-1 r: nrhs vectors of n rows at stride n each, the padding rows of r zero; a linear chain of launches on st
int mg_vcycle(const MgHierarchy *h, const void *r, void *z, hipStream_t st);
// the same on caller vectors without the padding rows (nrhs * n_user device values each), through padded buffers; synchronises
int mg_apply_padded(MgHierarchy *h, hipStream_t st, int dtype, int n, int n_user, int nrhs, const void *r_dev, void *z_dev, const char *who);
// what one V-cycle launches and moves: kernels, fine-level SpMVs (priced by the handle), and the bytes of everything else
struct MgCost { int launches = 0, spmv0 = 0; long long bytes = 0; };
MgCost mg_cost(const MgHierarchy *h);
int mg_levels(const MgHierarchy *h);
// info: rows, nnz, nx, ny, nz, the bits of the double lmax
int mg_level_info(const MgHierarchy *h, int level, long long info[6]);
// lmax[r] of the level for r < count (count <= the systems of a batched hierarchy, else 1)
int mg_level_bounds(const MgHierarchy *h, int level, double *lmax, int count);
// (a batched hierarchy: vals takes nsys * nnz values, system-major)
int mg_level_matrix(const MgHierarchy *h, int level, int *ptr, int *cols, void *vals, hipStream_t st);
// the map level -> level + 1 to the host (rows of the level ints; the box map of a grid hierarchy), *n_coarse = rows of level + 1
int mg_aggregates(const MgHierarchy *h, int level, int *agg_host, int *n_coarse, hipStream_t st);
// which: 0 five ints (n, nu, ld, steps, algebraic), 1 dinv (n values), 2 / 3 c0 / c1 (steps doubles), 4 the member lists (kAmgWidth
// ints per row of level + 1); *count is set even when cap_values is too small.  Synchronises.  A batched hierarchy: dinv is nsys * ld
// values (system r at r * ld), c0 / c1 steps * nsys doubles indexed (step, system)
int mg_level_state(const MgHierarchy *h, int level, int which, void *out_host, long long cap_values, long long *count, hipStream_t st);
// w = A_level x as the cycle launches it (the level's plan and leading dimension, the hierarchy's nrhs); synchronises
int mg_level_spmv(const MgHierarchy *h, int level, const void *x, void *w, hipStream_t st);
// ---- the cut matrix of a rank of the row-partitioned handle (dist_cut.hip): its rows without the entries at columns >= col_limit
// count[i] <- kept entries of row i < nu, 0 for the padding rows nu <= i < n (launch_mg_scan makes the row pointers)
int launch_cut_count(int nu, int n, int col_limit, const int *ptr, const int *cols, int *count, hipStream_t st);
// the kept columns and values of every row behind ptrc[row], in stored order
int launch_cut_fill(int dtype, int nu, int col_limit, const void *vals, const int *ptr, const int *cols, const int *ptrc, int *colsc,
                    void *valsc, hipStream_t st);
// the values alone, on the pattern a launch_cut_fill left
int launch_cut_refill(int dtype, int nu, int col_limit, const void *vals, const int *ptr, const int *cols, const int *ptrc, void *valsc,
                      hipStream_t st);
// ---- PCG of the row-partitioned loop (vector.hip, p2p.hip): z lives in q's storage for every preconditioner; part = [2][P] partials
// (r.z, then r.r); rho2 = two-entry parity buffer of rho = r.z (entry iter & 1), delta holds rho for cg_alpha
// r -= alpha q ; z = m .* r (stored over q) ; partials of r.z and r.r
int launch_pcg_jacobi_z(int dtype, int n, void *q_z, void *r, const void *m, const void *alpha, void *part_rz, void *part_rr, int grid,
                        hipStream_t st, const CgStop *stop = nullptr);
// red = {r.z, r.r} summed over all ranks (accumulator type).  mode 1: delta = rho2[0] = rho, history[0] = r.r, iter = 0;
// mode 3: beta = rho / rho2[(iter - 1) & 1], delta = rho2[iter & 1] = rho, history[iter] = r.r
int launch_pcg_scalars(int dtype, int mode, const void *red, const CgScalars &sc, void *rho2, hipStream_t st, const CgStop *stop = nullptr);
// x += alpha d ; d = z + beta d (alpha, beta from the device scalars)
int launch_pcg_xd_update(int dtype, int n, const void *z, void *d, void *x, const CgScalars &sc, hipStream_t st, const CgStop *stop = nullptr);
// peer-to-peer: the two sums in ONE round (slot set 1 carries r.r and the epoch, the kMbPcg area r.z), rank order, then the scalar
// step of launch_pcg_scalars (one work-group; advances *epoch)
int launch_pcg_allreduce2_p2p(int dtype, int mode, const void *part_rz, const void *part_rr, int P, char *const *mailbox, int rank,
                              int nranks, unsigned long long *epoch, const CgScalars &sc, void *rho2, hipStream_t st, const CgStop *stop = nullptr);
// four-launch loop: that round and the beta step in every work-group's prologue, then x += alpha d and d = z + beta d
int launch_pcg_aypx_beta_p2p(int dtype, int n, const void *z, void *d, void *x, const void *part_rz, const void *part_rr, int P,
                             char *const *mailbox, int rank, int nranks, const unsigned long long *epoch, const CgScalars &sc, void *rho2,
                             hipStream_t st, int vec_nt = 0, const CgStop *stop = nullptr);
// pcg_aypx_beta with p = z + beta p (z per right-hand side at stride ld), P thread-strided partials
int launch_pcg_aypx_beta_z(int dtype, int n, void *p, const void *z, long long ld, const void *part_rz, const void *part_rr, int P, int nrhs,
                           const CgScalars &sc, void *rho2, void *xs, hipStream_t st, const CgStop *stop = nullptr);
// four-launch peer-to-peer iteration (see p2p.hip): SpMV with the push and the wait inside, aypx with the beta all-reduce.
// halo_flag: device int per row block (1 = references a halo column); rotate: first row block of the visiting order
int launch_spmv_p2p(int dtype, const SpmvPlan &plan, int n, long long nnz, const void *vals, const int *ptr, const int *cols,
                    const void *d_ext, void *q, void *partials, const int *halo_flag, int rotate, const P2pExchange &e,
                    hipStream_t st);
int spmv_p2p_grid(const SpmvPlan &plan);
int launch_aypx_beta_p2p(int dtype, int n, const void *x, void *y, void *xs, const void *partials, int P, char *const *mailbox,
                         int rank, int nranks, int which, const unsigned long long *epoch, const CgScalars &sc, hipStream_t st,
                         int vec_nt = 0, const CgStop *stop = nullptr);
int launch_p2p_exchange(int dtype, const P2pExchange &e, void *v_ext, hipStream_t st);
// global sum (rank order) of the local sum of `partials`, followed in the same launch by the scalar step that consumes
// it: mode 1 = cg_delta0, 2 = cg_alpha, 3 = cg_beta; which in {0,1} selects the slot set
int launch_p2p_allreduce(int dtype, int mode, const void *partials, int grid, char *const *mailbox, int rank, int nranks,
                         int which, unsigned long long *epoch, const CgScalars &sc, hipStream_t st,
                         unsigned long long *bump0 = nullptr, unsigned long long *bump1 = nullptr, const CgStop *stop = nullptr);

// ---- single-reduction (Chronopoulos-Gear) loop of the row-partitioned solver (cg1.hip): w = A r with r.w and r.r partials
// ([2][row_blocks]); one global exchange per iteration in the prologue of the update launch
struct Cg1Update {
    int n = 0;
    void *r = nullptr, *p = nullptr, *s = nullptr, *x = nullptr;   // r: own part of the extended residual
    const void *w = nullptr;
    const void *red = nullptr;          // mailbox == null: accumulators {w.r, r.r} already summed over all ranks
    const void *partials = nullptr;     // mailbox != null: [2][P] local partials of the SpMV launch
    int P = 0;
    char *const *mailbox = nullptr;
    int rank = 0, nranks = 1;
    const unsigned long long *slot_epoch = nullptr;
    unsigned long long *halo_epoch = nullptr;
    void *state = nullptr;              // T[2][2] {gamma, alpha} by iteration parity
    CgScalars sc;
};
bool cg1_supported(const SpmvPlan &plan, const void *vals, const int *cols);
// e == nullptr: the halo is already in r_ext (RCCL backend, single rank); else push / wait inside the launch.  Bumps *iter and
// *slot_epoch (when non-null)
int launch_spmv_cg1(int dtype, const SpmvPlan &plan, int n, long long nnz, const void *vals, const int *ptr, const int *cols,
                    const void *r_ext, void *w, void *partials, const int *halo_flag, int rotate, const P2pExchange *e, int *iter,
                    unsigned long long *slot_epoch, hipStream_t st);
int launch_cg1_rowblock_rr(int dtype, int n, const void *r, void *partials, hipStream_t st);
int launch_cg1_update(int dtype, const Cg1Update &c, hipStream_t st, int vec_nt = 0);
// history[*iter] = r.r (no state of the recurrence changes); slot_epoch_rw: the slot epoch word (peer-to-peer form, advanced here)
int launch_cg1_tail(int dtype, const Cg1Update &c, unsigned long long *slot_epoch_rw, hipStream_t st);

// synthetic generators (device)
int launch_gen_laplace3d(int dtype, int nx, int ny, int nz, long long row_begin, long long row_end, void *vals,
                         int *ptr, int *cols, hipStream_t st);
long long laplace3d_ptr(long long i, int nx, int ny, int nz);
int launch_gen_poisson2d(int dtype, int N, void *vals, int *ptr, int *cols, hipStream_t st);
// generators.hip: variable = 1 helmFE_var (p0 = omega, p1 = rho; C_dev = wave speed per square or nullptr... never nullptr), 0 local_rect (p0 = k, p1 = eps, p2 = eta)
long long helm_fe_nnz(int Nh, int Nv);
int launch_gen_helm_fe(int dtype, int variable, int N, double p0, double p1, double p2, double L, const double *C_dev, int Nh, int Nv, void *vals,
                       int *ptr, int *cols, hipStream_t st);
long long poisson2d_ptr(long long i, int N);
// kind 0 rhs, 1 rhsL, 2 rhsA of helmFE_var.py:333-389 on an N x N node grid; b: N * N values of `dtype` (device)
int launch_gen_rhs(int dtype, int kind, int N, double k, void *b, hipStream_t st);

// ---- mixed-precision solve (mixed.hip, mixed.cpp): an fp32 / complex64 loop under an fp64 / complex128 x and true residual.
// dtype_hi: CGAMD_F64 (lo = float) or CGAMD_C128 (lo = float2).  n values per right-hand side, grid = (G, nrhs), every sum in fixed
// order; the two sides have leading dimensions of their own, both whole 16-byte packs where the 16-byte form is to run.
// x_hi[i] += scale[r] * HI(x_lo[i]) for the right-hand sides with mask[r] != 0; the others are not read or written.  scale: powers of two
int launch_mixed_accumulate(int dtype_hi, int n, void *x_hi, long long ld_hi, const void *x_lo, long long ld_lo, const double *scale,
                            const int *mask, int nrhs, hipStream_t st);
// r_lo[i] = LO(r_hi[i] * inv_scale[r]) for i < n, 0 for n <= i < ld_lo
int launch_mixed_round_down(int dtype_hi, int n, const void *r_hi, long long ld_hi, void *r_lo, long long ld_lo, const double *inv_scale,
                            int nrhs, hipStream_t st);
// out[r] = sum |v_i|^2 in double (conjugated); partials: mixed_norm2_grid(n) doubles per right-hand side
int mixed_norm2_grid(int dtype_hi, int n);
int launch_mixed_norm2(int dtype_hi, int n, const void *v, long long ld, int nrhs, double *partials, double *out, hipStream_t st);
// lo[j] = LO(hi[j]), count values: the inner handle's copy of the matrix
int launch_mixed_round_values(int dtype_hi, long long count, const void *hi, void *lo, hipStream_t st);

// ---- solution projection (projection.hip): W holds `slots` vectors per right-hand side, slot j of right-hand side r at
// W + j * slot_pitch + r * ld; live_mask names the slots that take part.  Scalars per (slot, right-hand side) live at [slot * nrhs + r]
// in the value type
constexpr int kProjMaxSlots = 32;
int proj_dots_grid(int dtype, long long n);     // work-groups (= partials per slot and right-hand side) of the dots pass
// out[slot * nrhs + r] = <w_slot, v_r> for the live slots (the others are not written); partials: slots * nrhs * grid accumulators
int launch_proj_dots(int dtype, int n, long long ld, int slots, unsigned live_mask, const void *W, long long slot_pitch, const void *v, int nrhs,
                     void *partials, int grid, void *out, hipStream_t st);
// y = base + sign * sum_j c_j w_j over the live slots, ascending; base = v - u, v (u == nullptr) or 0 (v == nullptr); y may be v
int launch_proj_combine(int dtype, int n, long long ld, int slots, unsigned live_mask, const void *W, long long slot_pitch, const void *v,
                        const void *u, const void *c, int sign, void *y, int nrhs, hipStream_t st);
// the scalar step of the update: s = sum alpha_j^2 + 2 sum alpha_j c_j + eq, acceptance, t = 1 / sqrt(nu) or 0, the flags;
// held: the slots of alpha, live: the slots of c; eq, nu: accumulators [nrhs]; out_nus: nu [nrhs], then s [nrhs]
int launch_proj_decide(int dtype, int nrhs, int slots, unsigned held, unsigned live, const void *alpha, const void *c, const void *eq,
                       const void *nu, double drop_tol, void *out_nus, void *t, int *added, hipStream_t st);
// w_r = e_r * t[r] where added[r], else zeros
int launch_proj_store(int dtype, int n, const void *e, long long ld, const void *t, const int *added, void *w, int nrhs, hipStream_t st);

// ---- multi-shift CG (shifts.hip): S shifted systems on the seed recurrence.  Scalars per (shift, right-hand side) live at
// [j * nrhs + r]: the state in the accumulator type, the coefficients of the vector pass and the history in the value type
constexpr int kShiftMax = 16;
struct ShiftScalars {
    int S = 0;
    const void *sigma = nullptr;                                // acc[S]
    void *theta = nullptr, *zeta = nullptr;                     // acc[S][nrhs]: zeta_k / zeta_{k-1} and zeta_k
    void *aprev = nullptr, *bprev = nullptr;                    // acc[S][nrhs]: alpha_{k-1}, beta_{k-1}, a copy per pair (no thread reads another's word)
    void *alpha_s = nullptr, *beta_s = nullptr, *zeta_s = nullptr;      // T[S][nrhs]: what the vector pass multiplies by
    void *history = nullptr;                                    // T[cap][S][nrhs]: zeta_k, row 0 all ones
    int history_cap = 0;
};
// theta = zeta = alpha_{-1} = 1, beta_{-1} = 0, history row 0
int launch_shift_init(int dtype, int nrhs, const ShiftScalars &sh, hipStream_t st);
// the scalar step of an iteration, from sc.alpha (slot 0), sc.beta and *sc.iter as the d step left them (stop: leaves on live[])
int launch_shift_scalars(int dtype, int nrhs, const ShiftScalars &sh, const CgScalars &sc, hipStream_t st, const CgStop *stop = nullptr);
// x_j += alpha_j d_j ; d_j = zeta_j r + beta_j d_j for all S shifts in ONE launch; r: [nrhs][ld], xs / ds: [S][nrhs][ld]
int launch_shift_update(int dtype, int n, long long ld, int nrhs, int S, const void *r, void *xs, void *ds, const void *alpha_s, const void *beta_s,
                        const void *zeta_s, hipStream_t st, int vec_nt = 0, const CgStop *stop = nullptr);

// ---- block CG (block_cg.hip): the s = nRHS right-hand sides of one real SPD matrix share one Krylov space.  The s x s matrices are
// row-major at pitch s
constexpr int kBlockMax = 16;
struct BlockDev {
    int *rec = nullptr;             // [0] status (0 fine, 1 G failed, 2 W^T W failed, 3 NaN), [1] the iteration of the event, [2] frozen
    double *min_ratio = nullptr;    // the smallest pivot ratio since set_rhs
    double *xi = nullptr, *G = nullptr, *alpha = nullptr, *tau = nullptr, *C = nullptr, *tau_inv = nullptr, *M = nullptr;
    void *M_T = nullptr, *alpha_T = nullptr, *tinv_T = nullptr, *tau_T = nullptr;      // what the vector launches multiply by, in the value type
    double *partials = nullptr;     // [s (s + 1) / 2][grid]
    // the preconditioned form (block_pcg.hip) alone: W^T Z as summed, and its partials beside those of W^T W
    double *CZ = nullptr, *partials_z = nullptr;
};
struct BlockState {
    int S = 0;                      // 0: off
    int grid = 0;                   // work-groups of the two launches that leave Gram partials
    void *mem = nullptr, *mem_pcg = nullptr;
    BlockDev dev;
};
int block_gram_grid(long long n);
int block_alloc(BlockState *b, int S, long long n);
void block_free(BlockState *b);
// frozen: the record's word every launch behind a breakdown or the stop leaves on (NULL: none)
int launch_block_gram(int dtype, int n, long long ld, int S, const void *a, const void *b, double *part, int grid, const int *frozen, hipStream_t st);
int launch_block_xw(int dtype, int n, long long ld, int S, const void *P, const void *AP, void *X, void *Q, const void *M, const void *AL, double *part,
                    int grid, const int *frozen, hipStream_t st);
int launch_block_qp(int dtype, int n, long long ld, int S, void *Q, void *P, const void *TI, const void *TA, bool init, const int *frozen, hipStream_t st);
// mode 0: set_rhs, 1: the G step, 2: the W step (stop: iterate_until's tolerances and words)
int launch_block_small(int dtype, int mode, const BlockState &b, const CgScalars &sc, const CgStop *stop, hipStream_t st);
// ---- block CG with a preconditioner inside the recurrence (block_pcg.hip): R = Q xi with Q^T M^-1 Q = I, Z = M^-1 W in q's storage
// the second allocation of a handle in that mode: W^T Z and its partials (b: allocated by block_alloc)
int block_pcg_alloc(BlockState *b);
// the partials of w^T diag(m) w: entry j (j + 1) / 2 + i = w_i . (m w_j), m w_j rounded once in the value type; m: n values, shared
int launch_block_gram_weighted(int dtype, int n, long long ld, int S, const void *w, const void *m, double *part, int grid, const int *frozen,
                               hipStream_t st);
// Q <- W tau^-1 ; P <- Z tau^-1 + P tau^T (init: P <- Z tau^-1).  Z: the block itself, or NULL and z_k = m w_k rounded once
int launch_block_qp_z(int dtype, int n, long long ld, int S, void *Q, void *P, const void *Z, const void *m, const void *TI, const void *TA, bool init,
                      const int *frozen, hipStream_t st);
// mode 0: set_rhs (partials: R0^T R0, partials_z: R0^T Z0), 2: the W step (W^T W, W^T Z)
int launch_block_pcg_small(int dtype, int mode, const BlockState &b, const CgScalars &sc, const CgStop *stop, hipStream_t st);

}  // namespace cgamd

// ---- what mixed.cpp needs of its two handles beyond the C ABI (solver.cpp) ----
#pragma GCC visibility push(hidden)
namespace cgamd {
const void *solver_matrix(cgamd_solver *s, const int **ptr, const int **cols);      // the device arrays the handle's SpMV reads
int solver_restart(cgamd_solver *s);        // set_rhs again from the b and the x the handle holds (x as written through cgamd_solver_vector)
int solver_set_rhs_ld(cgamd_solver *s, const void *b, long long ldb);                // set_rhs(b, NULL, on_device) with b at stride ldb
int solver_replace_residual_ld(cgamd_solver *s, const void *r_new, long long ldr);  // cgamd_solver_replace_residual, r_new at stride ldr
bool solver_block_on(const cgamd_solver *s);      // cgamd_solver_set_block is in force: the mixed solve does not serve it
int solver_replace_planned(cgamd_solver *s);        // would replace_residual refuse this handle after its next set_rhs?  (changes nothing)
}  // namespace cgamd
#pragma GCC visibility pop

// ---- context (shared by api.cpp / solver.cpp / dist.cpp) ---------------------------
struct cgamd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    void *partials = nullptr;   // workspace for the stand-alone vdot op
    size_t partials_bytes = 0;
};
